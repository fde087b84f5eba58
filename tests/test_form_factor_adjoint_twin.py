"""The adjoint of the raw 1-D form factor (tsff_form_factor_grad: k_form_factor_adj<NI, 0|2>, k_lbacc_reduce, k_ff2d_lines_adj,
k_sum_chunks and the f_e tail k_wgemm_t + k_fe_adjoint), entry by entry, against the oracle's torch twin -- each entry on its own scale.

For one lineout, a seed Pbar [G, npts, n_angles] and a leaf x_k (a physical slot or a node of f_e)

  g[k] = sum_(g,i,a) Pbar[g,i,a] dP[g,i,a]/dx_k,    A[k] = sum_(g,i,a) |Pbar[g,i,a] dP[g,i,a]/dx_k|

(oracle/tsadar_oracle_torch.py: ff1d_adjoint; d P / d x by forward mode of ``angular_twin.form_factor_fn``, the terms per point, the
chain not cut further: an f_e node's path through W and its direct path arrive summed).  A is the scale at which two float64
summations of the same terms may differ, the definition of tests/test_ff2d_adjoint_twin.py and test_loss_grad_entries.py.  The bound
is |device - twin| <= TOL * A for every (lineout, slot) and every (lineout, f_e node); where A is 0 -- the amplitudes, A_s, m, the
slots of species the deck does not have, a single species' fraction -- the device value is exactly 0.  max |R| over the slots is not
that scale (test_kernel_matrix._ff_case): against it Te_gradient, ne_gradient, ud, a minority species' Ti and the fractions are
pinned to percents (test_quiet_entries_are_present prints how quiet they are).

Every species is its own leaf in the twin (ti_same all zero): the device returns a tied species' share in its own slot.  The seed
is random normal over ALL points divided by mean |P| of the twin, also in the ARTS case (1024 x 241 points: one twin pass over all
of them took 5 s of CPU here, far from the two minutes above which a band of wavelength samples would have been seeded instead).
Lineouts: util.random_lineouts(seed = the case's draw, ud in (-1.5, 1.5), every species' Ti and Z drawn); f_e: per-lineout free
form (test_form_factor_jvp._free_form_fe); fractions: drawn per lineout in (0.1, 0.9), they do NOT sum to 1 (the form factor takes
them raw); ion-4 of the four-ion deck is a trace species at a fiftieth of its draw, which makes its T_i one of the quiet entries.
Not among the twin's slots: fract_1 of a one-ion deck.  A single species' fraction cancels out of fr / Zbar, the only way it enters;
its derivative is identically zero, the twin's forward mode gives exact zeros and its reverse mode a residue (4e-13 against terms
that are all 0: a rounding residue with no scale of its own).  The slot has A = 0 and the device must write an exact zero.
A draw that puts a seeded point on a kink, or on which the twin's two modes disagree beyond their bound, is replaced by another seed
of the draw, never by another bound: each case takes the first seed from 211 (test_form_factor_jvp's; the ARTS case from 5) that keeps
KINK and meets test_twin_terms_sum_to_reverse_mode with a factor of two to spare.  That rule cost the physical slots nothing (at most
6e-14 of A on every draw tried) and the f_e nodes many draws: the oracle takes d f_e / d v as the difference of neighbouring
wavelength samples, which lie 1e-4 apart in xi_e in the ion window, so one point's term is itself a cancelling difference known to
1e-12 of its size, and where the ion-acoustic peaks carry the sum nothing averages.  Of the base case's 30 draws tried, 4 met 1e-12
(seeds 213, 224, 230, 240; the others 1e-12 .. 2e-11, all from f_e nodes of the ion feature); ni2 took its second draw, ni4 and
nvx 320 their third, ARTS its second (the first lay on a kink).  The device bound, 1e-7 of A, is five decades above all of this.

CASES: name -> (n_ion, nvx, deck modifiers, B, ((feature, want_fe), ...), draw).  "shared": one table for every lineout
(fe_mode SHARED).  The tiled cases (uneven chunks, one chunk) repeat the base case's lineouts; "arts" is the fit's own geometry.

The CPU tests make the GPU cases worth what they claim: the twin's terms sum to its reverse mode (1e-12 A; largest measured
4.4e-13, an f_e node of the ion feature), no seeded point sits on a kink of the forward, the quiet entries are there, and the twin's
derivative along the slots no other test differences (fract_1, fract_2, Te_gradient, ne_gradient, Z_2, Ti_2) agrees with difference
quotients of the NumPy oracle.

Measured on an MI355X (profiles/form_factor_adjoint_pytest.txt), the largest |device - twin| / A against the bound of 1e-7: 1.7e-9
over the f_e nodes (ARTS; 5.9e-10 in ni1 and both tiled batches), 7.8e-10 over the physical slots (shared; at most 2.3e-10
elsewhere).  grad_fe of the repeats of a tiled member differed by up to 1.2e-12 of A (the order of its LDS atomic adds), grad_phys
not by a bit.  Every path was correct as found.  That the cases can fail was tried once on a library whose lines_adj_store swaps
the a_i partials of species 1 and 2: ni2_tied_G3, ni3_tied and ni4 failed, each naming Ti_1 of lineout 2."""
import functools
import os

import numpy as np
import pytest

import angular_twin as at
import decks
import test_form_factor_jvp as tff
import util
from oracle import tsadar_oracle as orc
from oracle import tsadar_oracle_torch as ot
from tsadar_amd import _lib as L
from test_kernel_matrix import _library_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "form_factor_adjoint_pytest.txt")
CSRC = os.path.join(ROOT, "tsadar_amd", "csrc")

TOL = 1e-7    # TOL of tests/test_ff2d_adjoint_twin.py and test_loss_grad_entries.py; a ceiling, not a fit
KINK = 1e-6   # cells: xi_e on the vx nodes, in-table xi_i on the Z' nodes
NPTS = 1024
ARTS = dict(ccd=(128, 256), start=10, end=110, n_angles=241)

# name -> (n_ion, nvx, deck modifiers, B, ((feature, want_fe), ...), seed of the draw)
CASES = {
    "ni1": (1, 64, (), 3, ((0, True), (1, True)), 230),
    "ni2_tied_G3": (2, 64, (tff._tie2, tff._grad3), 3, ((0, True), (1, True)), 212),
    "ni3_tied": (3, 64, (), 3, ((0, True), (1, False)), 211),
    "ni4": (4, 64, (), 3, ((0, False), (1, True)), 213),
    "ni1_nvx320": (1, 320, (), 2, ((0, True),), 213),
    "shared": (1, 64, (), 3, ((0, False), (1, False)), 211),
    "arts": (1, 64, (), 1, ((0, True),), 6),
}
TWINS = [(c, f) for c in CASES for f, _ in CASES[c][4]]


def record(key, text):
    """tests/test_form_factor_jvp.record into this file's own profile: one line per case, the case's previous line replaced"""
    saved = tff.RECORD
    tff.RECORD = RECORD
    try:
        tff.record(key, text)
    finally:
        tff.RECORD = saved


@functools.lru_cache(maxsize=None)
def _inputs(name):
    n_ion, nvx, mods, B, _, seed = CASES[name]
    if name == "arts":
        cfg = decks.deck_angular(1, nvx, ARTS["ccd"], ARTS["start"], ARTS["end"])
        sa = util._angular_sa(cfg)
        assert len(sa["sa"]) == ARTS["n_angles"]
    else:
        cfg = decks.deck_fit(nvx=nvx, n_ion=n_ion, active=("Te", "ne", "Ti", "Z", "Ti_same_3"))
        for m in mods:
            m(cfg)
        sa = util.sa_fit(B)
    assert cfg["other"]["npts"] == NPTS
    from tsadar_amd.params import SlotMap

    ti_same = SlotMap(cfg["parameters"], True).ti_same
    ranges = dict(ud=(-1.5, 1.5), Z_1=(4.0, 12.0), Z_2=(0.8, 2.0), Z_3=(4.0, 8.0), Z_4=(1.5, 3.0))
    ranges.update({f"Ti_{s}": (0.05, 0.5) for s in range(2, n_ion + 1) if not ti_same[s - 1]})
    normed = util.random_lineouts(cfg, B, seed=seed, ranges=ranges)
    X = util.normed_to_matrix(orc.physical_params(cfg["parameters"], normed, True), n_ion)
    if n_ion > 1:   # raw fractions of a lineout: their sum anywhere in (0.2, 3.6), never 1
        X[:, [util.slot_of(f"fract_{s + 1}") for s in range(n_ion)]] = np.random.default_rng(seed + 1).uniform(0.1, 0.9, (B, n_ion))
        if n_ion == 4:   # (ion-4 a trace species, a fiftieth of its draw: a minority T_i that is quiet on the case's scale)
            X[:, util.slot_of("fract_4")] *= 0.02
    fe = tff._free_form_fe(B, nvx, 9)
    if name == "shared":
        fe = np.repeat(fe[:1], B, axis=0)   # (the twin's view: every lineout reads table 0)
    G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
    names = [k for k in ot.phys_names_2d(n_ion) if n_ion > 1 or k != "fract_1"]   # (a single species' fraction: see the docstring)
    return dict(cfg=cfg, sa=sa, X=X, fe=fe, n_ion=n_ion, nvx=nvx, B=B, G=G, ti_same=ti_same, names=names)


def _fn(s, b, feature):
    A = [s["X"][b, L.P_ION0 + 4 * i + L.ION_A] for i in range(s["n_ion"])]
    return at.form_factor_fn(s["cfg"], s["sa"]["sa"], s["n_ion"], np.zeros(4), A, feature)


@functools.lru_cache(maxsize=None)
def _twin(name, feature):
    """Pbar [B, G, npts, n_angles] and the twin's (g, A) of every lineout: gp, Ap [B, NP] in the engine's slots (zero where the form
    factor reads nothing), gf, Af [B, nvx] or None.  Computed once per (case, feature), shared by the tests, never modified."""
    import torch

    s = _inputs(name)
    want_fe = dict(CASES[name][4])[feature]
    slots = [util.slot_of(k) for k in s["names"]]
    B, NP = s["X"].shape
    rng = np.random.default_rng(1000 * sorted(CASES).index(name) + feature)
    Pbar, gp, Ap, gf, Af = [], np.zeros((B, NP)), np.zeros((B, NP)), np.zeros((B, s["nvx"])), np.zeros((B, s["nvx"]))
    for b in range(B):
        f = _fn(s, b, feature)
        with torch.no_grad():
            P = f(ot._t(s["X"][b]), ot._t(s["fe"][b])).numpy()
        Pbar.append(rng.standard_normal(P.shape) / np.abs(P).mean())
        g, A, g2, A2 = ot.ff1d_adjoint(f, s["X"][b], s["fe"][b], Pbar[b], slots, want_fe=want_fe)
        gp[b, slots], Ap[b, slots] = g, A
        if want_fe:
            gf[b], Af[b] = g2, A2
    return dict(Pbar=np.array(Pbar), gp=gp, Ap=Ap, gf=gf if want_fe else None, Af=Af if want_fe else None)


def _ratio(err, A):
    return err / np.where(A > 0, A, 1.0)


def _assert_entries(what, s, dev_p, dev_f, t, tol):
    """|dev - twin| <= tol * A for every (lineout, slot) and (lineout, f_e node), none left out; exactly 0 where A is 0.
    -> the worst ratio per slot name and over the f_e nodes"""
    slot_names = {util.slot_of(k): k for k in s["names"]}
    worst = {}
    for kind, dev, g, A in (("phys", dev_p, t["gp"], t["Ap"]), ("fe", dev_f, t["gf"], t["Af"])):
        if g is None:
            assert dev is None, (what, kind)
            continue
        dev = np.asarray(dev)
        assert dev.shape == g.shape and np.all(np.isfinite(dev)), (what, kind, dev.shape, g.shape)
        err = np.abs(dev - g)
        r = _ratio(err, A)
        if kind == "phys":
            worst.update({k: float(r[:, c].max()) for c, k in sorted(slot_names.items())})
        else:
            worst["fe"] = float(r.max())
        assert np.all(dev[A == 0] == 0.0), (what, kind, "not exactly zero where A = 0", np.nonzero((A == 0) & (dev != 0)))
        b, c = np.unravel_index(np.argmax(err - tol * A), err.shape)
        where = slot_names.get(c, c) if kind == "phys" else f"fe[{c}]"
        assert np.all(err <= tol * A), (what, "lineout", b, where, "got", dev[b, c], "twin", g[b, c], "A", A[b, c], "ratio", r[b, c],
                                        {k: "%.2e" % v for k, v in worst.items()})
    print(what, "max |. - twin| / A:", {k: float("%.2e" % v) for k, v in worst.items()})
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,feature", TWINS)
def test_twin_terms_sum_to_reverse_mode(name, feature):
    """Every entry of g equals one backward of <Pbar, P> within 1e-12 of A (the bound of
    test_loss_grad_entries.test_twin_terms_sum_to_reverse_mode), and A >= |g|: no entry of any case is a rounding residue above its
    own scale.  (T_i beyond the Z' table, the residue test_loss_grad_entries.py's docstring names, does not arise: every seed covers
    the laser line, where the ion feature gives T_i a scale of its own also in the electron window.)"""
    s, t = _inputs(name), _twin(name, feature)
    rp, rf = np.zeros_like(t["gp"]), np.zeros((s["B"], s["nvx"]))
    for b in range(s["B"]):
        rp[b], rf[b] = ot.ff1d_reverse(_fn(s, b, feature), s["X"][b], s["fe"][b], t["Pbar"][b])
    off = np.ones(rp.shape[1], dtype=bool)
    off[[util.slot_of(k) for k in s["names"]]] = False
    assert not np.any(t["Ap"][:, off])
    if s["n_ion"] == 1:   # (the residue of a single species' fraction, see the docstring: no term stands behind it)
        rp[:, util.slot_of("fract_1")] = 0.0
    assert not np.any(rp[:, off])   # (the form factor reads no other slot)
    for g, A in ((t["gp"], t["Ap"]), (t["gf"], t["Af"])):
        if g is not None:
            assert np.all(np.isfinite(g)) and np.all(A >= np.abs(g) * (1 - 1e-12))
    _assert_entries(f"{name} feature {feature} reverse mode", s, rp, rf if t["gf"] is not None else None, t, 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_no_point_on_a_kink(name):
    """From the oracle's own positions: every seeded point's xi_e (all points are seeded) keeps KINK of a cell from the vx nodes, and
    every in-table xi_i from the Z' nodes, for every species, gradient point and feature of the case."""
    s = _inputs(name)
    vx = orc.velocity_grid(s["nvx"])
    _, xi2 = orc.xi_grids()
    worst = dict(xe=np.inf, xi=np.inf)
    for b in range(s["B"]):
        x = s["X"][b]
        p = {k: x[util.slot_of(k)] for k in ("Te", "ne", "lam", "ud", "Va", "Te_gradient", "ne_gradient")}
        for k in ("Ti", "A"):
            p[k] = [x[util.slot_of(f"{k}_{i + 1}")] for i in range(s["n_ion"])]
        for feature, _ in CASES[name][4]:
            for g in range(s["G"]):
                for i in range(s["n_ion"]):
                    xe, xi = util.positions(s["cfg"], s["sa"], p, feature, ion=i, grad_point=g if s["G"] > 1 else None)
                    inside = (xi > xi2[0]) & (xi < xi2[-1])
                    worst["xe"] = min(worst["xe"], util.node_distance(xe, vx).min())
                    if inside.any():
                        worst["xi"] = min(worst["xi"], util.node_distance(xi[inside], xi2).min())
    print(name, "nearest node, cells: xi_e on vx %.2e, xi_i on Z' %.2e" % (worst["xe"], worst["xi"]))
    assert worst["xe"] >= KINK and worst["xi"] >= KINK, (name, worst)


QUIET = ("Te_gradient", "ne_gradient", "ud", "fract", "minority Ti")


def test_quiet_entries_are_present():
    """What one maximum over the slots cannot see: in at least one case each of Te_gradient, ne_gradient, ud, a fraction and a
    minority species' Ti has an entry below 1e-3 of the case's largest |g_phys| whose |g| / A is above 1e-3 (a signal, not a residue)."""
    found = {k: [] for k in QUIET}
    for name, feature in TWINS:
        s, t = _inputs(name), _twin(name, feature)
        g, A = np.abs(t["gp"]), t["Ap"]
        rel, sig = g / g.max(), g / np.where(A > 0, A, 1.0)
        print(name, "feature", feature)
        for k in s["names"]:
            c = util.slot_of(k)
            print("   %-12s |g| / max |g| %s   |g| / A %s" % (k, " ".join("%.1e" % v for v in rel[:, c]), " ".join("%.1e" % v for v in sig[:, c])))
            kind = "fract" if k.startswith("fract_") else "minority Ti" if (k.startswith("Ti_") and k != "Ti_1") else k
            if kind in found and np.any((rel[:, c] < 1e-3) & (sig[:, c] > 1e-3)):
                found[kind].append((name, feature))
    print(found)
    assert all(found.values()), found


FD_SLOTS = ("fract_1", "fract_2", "Te_gradient", "ne_gradient", "Z_2", "Ti_2")


@pytest.mark.parametrize("feature", [0, 1])
def test_twin_matches_oracle_differences_new_slots(feature):
    """test_form_factor_jvp.test_twin_jvp_matches_oracle_differences' (h, h/2) ladder for unit directions of the slots no test has
    differenced, on the two-ion G = 3 case (lineout 1, every species its own leaf): per row (one angle's spectrum of one gradient
    point) the pair of steps whose quotients agree best with each other, held to 1e-5 of the row's largest entry.

    The ladder runs from 1e-3 of the slot's value, that test's first step, down to 4e-9 of it (19 steps instead of 8).  The Z' table
    is piecewise linear: a sample whose xi_i crosses a node inside the step gives the mean of two slopes whatever the step, and in the
    ion window, where a cell of the table holds two or three samples, steps of 1e-3 .. 1e-5 of T_i always catch some (Ti_2 missed by
    1e-4 .. 6e-4 there with the 8 steps).  At the small end a step moves xi_i by about KINK cells, which test_no_point_on_a_kink keeps
    free, and the quotient's rounding (1e-16 / 4e-9) stays far below 1e-5; the gradient slots, whose derivative is 1/200 of T_e's or
    n_e's, want the large end (3e-5 .. 4e-5 from steps of 1e-5 and below in the ion window: rounding).
    No slot needed tests/test_angular_postfit.FD_TOL.  The middle gradient point does not move with Te_gradient or ne_gradient: those
    rows are identically zero in the twin, and the quotient is held to 1e-5 of the largest entry of the angle's other gradient points."""
    import torch

    s = _inputs("ni2_tied_G3")
    b = 1
    x0, fe = s["X"][b], s["fe"][b]
    f = _fn(s, b, feature)
    vx = orc.velocity_grid(s["nvx"])
    other = s["cfg"]["other"]
    rng, shift = (other["lamrangE"], s["cfg"]["data"]["ele_lam_shift"]) if feature == 0 else (other["lamrangI"], 0.0)
    names = ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]

    def oracle(x):
        p = {n: x[util.slot_of(n)] for n in names}
        for k in ("Ti", "Z", "A", "fract"):
            p[k] = [x[util.slot_of(f"{k}_{i + 1}")] for i in range(2)]
        return orc.form_factor(rng, other["npts"], shift, s["sa"]["sa"], s["G"], p, vx, fe)[0]

    worst = {}
    for nm in FD_SLOTS:
        d = np.zeros_like(x0)
        d[util.slot_of(nm)] = 1.0
        _, Pd = torch.autograd.functional.jvp(f, (ot._t(x0), ot._t(fe)), (ot._t(d), torch.zeros(s["nvx"], dtype=ot.DT)))
        J = Pd.numpy().transpose(0, 2, 1)
        h0 = 1e-3 * max(abs(x0[util.slot_of(nm)]), 0.05)
        quot = [(oracle(x0 + h * d) - oracle(x0 - h * d)) / (2 * h) for h in (h0 / 2 ** i for i in range(19))]
        best = None
        for q0, q1 in zip(quot[:-1], quot[1:]):
            q0, q1 = q0.transpose(0, 2, 1), q1.transpose(0, 2, 1)
            gap = np.max(np.abs(q0 - q1), axis=-1)
            pick = q1 if best is None else np.where((gap < best[0])[..., None], q1, best[1])
            best = (gap if best is None else np.minimum(gap, best[0]), pick)
        scale = np.max(np.abs(J), axis=-1)   # [G, n_angles]
        assert np.all(scale > 0) or nm.endswith("_gradient"), nm
        scale = np.where(scale > 0, scale, scale.max(axis=0, keepdims=True))
        worst[nm] = float(np.max(np.max(np.abs(best[1] - J), axis=-1) / scale))
    print(f"feature {feature}: twin vs oracle quotients, max per row of the row's largest entry:", {k: "%.1e" % v for k, v in worst.items()})
    assert all(v < 1e-5 for v in worst.values()), worst


def angle_chunks(B, n_angles, ncu):
    """tsff_api.inc's angle_chunks"""
    return max(1, min(n_angles, (4 * ncu) // max(B, 1)))


def test_angle_chunks_is_the_plans():
    api = open(os.path.join(CSRC, "tsff_api.inc")).read()
    assert "const int want = 4 * h->ncu2d();" in api, "restate angle_chunks above"
    assert "return (unsigned)std::max(1, std::min(h->S.n_angles, want / std::max(B, 1)));" in api, "restate angle_chunks above"
    assert "p.nchunk = angle_chunks(h, B);" in api and "if (p.nchunk > 1) {" in api
    assert "for (int a = blockIdx.y; a < NA; a += gridDim.y) {" in open(os.path.join(CSRC, "k_form_factor.inc")).read()


def _kernels(n_ion, want_fe):
    k = (f"k_form_factor_adj<{n_ion}, {2 if want_fe else 0}>", "k_lbacc_reduce", f"k_ff2d_lines_adj<{n_ion}>")
    return k + (("k_wgemm_t", "k_fe_adjoint") if want_fe else ())


def test_named_kernels_are_in_the_library():
    from tsadar_amd import build

    build.build()
    shipped = _library_kernels(build.OUT)
    named = {k for n in range(1, 5) for w in (False, True) for k in _kernels(n, w)} | {"k_sum_chunks"}
    assert not sorted(named - shipped), sorted(named - shipped)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _engine(name):
    from tsadar_amd.engine import Engine

    s = _inputs(name)
    if name == "shared":
        eng = Engine(s["cfg"], s["sa"], fe_shared=s["fe"][0])
        assert eng.fe_mode == L.FE_SHARED
        return eng
    return Engine(s["cfg"], s["sa"], fe_mode=L.FE_PER_LINEOUT)


def _want(torch):
    return 4 * torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _launch_check(eng, s, want_fe, nchunk):
    got = eng.last_launch()
    missing = [k for k in _kernels(s["n_ion"], want_fe) if k not in got]
    assert not missing, f"expected {missing} among the launched kernels {got}"
    other = f"k_form_factor_adj<{s['n_ion']}, {0 if want_fe else 2}>"
    assert other not in got, got
    if not want_fe:
        assert "k_wgemm_t" not in got and "k_fe_adjoint" not in got and "k_sum_chunks" not in got, got
    else:   # the per-chunk table adjoints are summed only where there is more than one chunk: W, then H
        assert got.count("k_sum_chunks") == (2 if nchunk > 1 else 0), (nchunk, got)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_form_factor_grad_matches_twin(torch_mod, name):
    """Engine.form_factor_grad against ff1d_adjoint, every (lineout, slot) and (lineout, f_e node) within TOL of its own A.
    ni1: k_form_factor_adj<1, 2>, nchunk == n_angles, and the call without f_e (<1, 0>) whose grad_phys is the same bits;
    ni2_tied_G3: fractions, gradient points, the tied share in its own slot; ni3_tied / ni4: the instantiations only test_kernel_matrix
    reaches, one feature with f_e and one without; ni1_nvx320: the production grid and the largest LDS carve of GM = 2; shared: table 0
    read by every lineout, only <NI, 0> may launch and a call with f_e is refused with -2 before anything is enqueued; arts: the fit's
    own shape, 241 chunks of one angle, 964 partials per k_lbacc_reduce row."""
    s, eng = _inputs(name), _engine(name)
    B, NA = s["B"], len(s["sa"]["sa"])
    nchunk = angle_chunks(B, NA, _want(torch_mod) // 4)
    assert nchunk == NA, (name, "one angle per chunk", nchunk)   # (the regime of every untiled case: want // B >= n_angles)
    fe_arg = None if name == "shared" else s["fe"]
    worst = {}
    for feature, want_fe in CASES[name][4]:
        t = _twin(name, feature)
        gp, gf = eng.form_factor_grad(feature, s["X"], fe_arg, t["Pbar"], want_fe=want_fe)
        torch_mod.cuda.synchronize()
        _launch_check(eng, s, want_fe, nchunk)
        w = _assert_entries(f"{name} feature {feature} device", s, gp.cpu().numpy(), gf.cpu().numpy() if want_fe else None, t, TOL)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        gp2, gf2 = eng.form_factor_grad(feature, s["X"], fe_arg, t["Pbar"], want_fe=want_fe)
        assert torch_mod.equal(gp, gp2)   # two calls, the same bits: the lineout scalars are folded in a fixed order
        if want_fe:   # (the table adjoints are gathered by LDS atomic adds, whose order is not fixed: each call is held to the twin)
            _assert_entries(f"{name} feature {feature} device, second call", s, gp2.cpu().numpy(), gf2.cpu().numpy(), t, TOL)
        if want_fe:   # without the table adjoints: <NI, 0>, the lineout scalars bit for bit
            gp0, none = eng.form_factor_grad(feature, s["X"], fe_arg, t["Pbar"], want_fe=False)
            torch_mod.cuda.synchronize()
            _launch_check(eng, s, False, nchunk)
            assert none is None and torch_mod.equal(gp, gp0)
    if name == "shared":
        t = _twin(name, 0)
        gfe = torch_mod.empty((B, s["nvx"]), dtype=torch_mod.float64, device=eng.device)
        gph = torch_mod.empty((B, eng.NP), dtype=torch_mod.float64, device=eng.device)
        p = eng._ptr
        rc = eng.lib.tsff_form_factor_grad(eng.h, 0, p(eng.dev(s["X"])), p(None), B, p(eng.dev(t["Pbar"])), p(gph), p(gfe))
        assert rc == -2 and eng.last_launch() == [] and b"PER_LINEOUT" in eng.lib.tsff_last_error(eng.h)
    record(f"form_factor_grad[{name}]", f"max |device - twin| / A {max(worst.values()):.3e} (bound {TOL:.0e}), per slot " +
           " ".join(f"{k} {v:.1e}" for k, v in worst.items()))


TILED = {"uneven_chunks": lambda want: want // 6, "one_chunk": lambda want: want // 2 + 1}


@pytest.mark.gpu
@pytest.mark.parametrize("plan", list(TILED))
def test_form_factor_grad_chunk_plans(torch_mod, plan):
    """The base case's three lineouts tiled to B (lineout b is member b mod 3, Pbar and f_e with it), as
    tests/test_forward_mode_plans_gpu.py tiles: every lineout against its member's twin result at TOL of A, and grad_phys of all
    repeats of a member equal bit for bit (grad_fe is gathered by LDS atomic adds in no fixed order: every repeat is held to the twin).
    uneven_chunks: B = want // 6, six chunks over ten angles -- chunks 0 .. 3 walk two angles (a and a + 6), chunks 4 and 5 one: the
    strided angle loop, k_sum_chunks over unequal chunks; one_chunk: B = want // 2 + 1, one workgroup per lineout walks all ten angles
    and k_sum_chunks is not launched.  want = 4 x the device's compute units (angle_chunks)."""
    s, eng = _inputs("ni1"), _engine("ni1")
    want, NA, K = _want(torch_mod), len(s["sa"]["sa"]), s["B"]
    B = TILED[plan](want)
    nchunk = angle_chunks(B, NA, want // 4)
    if plan == "uneven_chunks":
        assert 1 < want // B < NA and NA % (want // B) != 0 and nchunk == want // B, (want, B, nchunk)
        assert NA // nchunk == 1 and NA % nchunk != 0, (NA, nchunk)   # chunks of two angles and chunks of one
    else:
        assert nchunk == 1, (want, B, nchunk)
    idx = np.arange(B) % K
    X, fe = np.ascontiguousarray(s["X"][idx]), np.ascontiguousarray(s["fe"][idx])
    worst = {}
    for feature, want_fe in CASES["ni1"][4]:
        t = _twin("ni1", feature)
        tt = {k: (None if v is None else np.ascontiguousarray(v[idx])) for k, v in t.items()}
        gp, gf = eng.form_factor_grad(feature, X, fe, tt["Pbar"], want_fe=True)
        torch_mod.cuda.synchronize()
        got = _launch_check(eng, s, True, nchunk)
        assert ("k_sum_chunks" in got) == (plan == "uneven_chunks"), got
        gp, gf = gp.cpu().numpy(), gf.cpu().numpy()
        w = _assert_entries(f"{plan} B={B} nchunk={nchunk} feature {feature} device", s, gp, gf, tt, TOL)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        assert np.array_equal(gp, gp[:K][idx]), (plan, feature, "repeats of a member differ")
        print(f"{plan} feature {feature}: repeats of a member, max |grad_fe - first repeat's| / A = {_ratio(np.abs(gf - gf[:K][idx]), tt['Af']).max():.2e}")
        gp2, _ = eng.form_factor_grad(feature, X, fe, tt["Pbar"], want_fe=True)
        assert np.array_equal(gp2.cpu().numpy(), gp)
    record(f"form_factor_grad[{plan}]", f"B {B} nchunk {nchunk} max |device - twin| / A {max(worst.values()):.3e} (bound {TOL:.0e}), per slot " +
           " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
