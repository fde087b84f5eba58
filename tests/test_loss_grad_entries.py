"""The 1-D loss gradient (tsff_loss_grad: k_spectrum_fused + k_fused_finish, k_spectrum_rows, k_spectrum and their shared tail in
k_chain.inc), entry by entry, against the oracle's torch twin -- each entry on its own scale.

For lineout b and trainable leaf k the gradient is a sum over the form-factor points and, for the direct paths (the amplitudes),
over the bins:

  g[b, k] = sum_(f,g,i,a) Pbar[f,g,i,a] dP[f,g,i,a]/dx_k + sum_(f,j) Tbar[f,j] (dT[f,j]/dx_k at fixed P)

A[b, k] is the same sum with every term replaced by its absolute value (oracle/tsadar_oracle_torch.py: loss_adjoint; for the DLM order
m a term is Pbar dP/d(node) d(node)/dm for every node of the f_e and W tables a point reads, the chain cut once more): the scale at
which two float64 evaluations of the sum may differ, the definition tests/test_ff2d_adjoint_twin.py uses for the 2-D path.  The bound
is |device - twin| <= TOL * A for every (lineout, trainable slot); inactive slots are exactly 0.  max |g| over the leaves or over a
column is not that scale: against it Te_gradient, ne_gradient, ud, a minority species' Ti and the fractions are pinned to percents
(test_cases_contain_quiet_entries prints how quiet they are).

The seed Tbar = d loss / d T is the twin's own functional derivative evaluated at the DEVICE's spectra, which are pinned separately
(1e-8 / 1e-7): a forward difference of 3e-9 must not blur the adjoint's bound, and a wrong seed formula on the device still fails.

CASES: name -> (deck tweaks, B, launch plan, kernels the call must launch).  Deck tweaks of decks.deck_fit: n_ion, ppp (points per
pixel), nvx, nang (scattering angles), G (gradient points, both gradients trainable), leaves (deck_fit's `active`), fract (every
species' fraction trainable), tie (species whose Ti is tied to ion-1's), loss, load ("ele" / "ion": one loaded feature), blue (False:
fit_EPWb off), offset (a background under the data, in units of its maximum).  B lineouts; the last one has no noise.  ele_lam_shift
0.3 and the notch filter are on throughout.  Every lineout draws its own T_e, n_e, T_i, Z, u_d, V_a, lam, amplitudes and -- where they
are leaves -- fractions, which do NOT sum to 1 (tie_renorm_adjoint's g = (g - dot) / fsum with fsum != 1, fr != the raw leaf).

Not checked: T_i on the EPW-only deck.  Beyond the Z' table T_i drops out of chi_i's asymptote, what is left of d P / d T_i in the
electron window is a rounding residue far above its own A (|g| ~ 5e-21 against A ~ 8e-23 in the twin), and the deck leaves T_i
inactive as the reference's EPW-only deck does.  One draw (SEED) serves every deck: a draw that puts a point on a kink, or on which
the two references or the twin's two summation orders disagree beyond their bounds, is replaced by another draw, never by another bound.

The CPU tests make the GPU cases worth what they claim: the twin's sum of terms equals its reverse mode (1e-12 A), the C++ oracle's
dual numbers agree with it a hundred times better than TOL, no point sits on a kink of the forward, and the quiet entries are there."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc
from oracle import tsadar_oracle_torch as ot
from tsadar_amd.params import SlotMap
from test_kernel_matrix import _library_kernels

TOL = 1e-7    # TOL of tests/test_ff2d_adjoint_twin.py, the 1e-7 the 1-D adjoint is held to on the global scale; a ceiling, not a fit
SEED = 7      # of every deck's draws (data, truth and lineouts)
KINK = 1e-6   # cells (xi_e on the vx nodes, xi_i on the Z' nodes, m on the DLM axis); of max T for |d - T| under l1

ALL1 = ("Te", "ne", "Ti", "Z", "Va", "ud", "lam", "amp1", "amp2", "amp3")
GRAD = ALL1 + ("Te_gradient", "ne_gradient")
EPW = tuple(k for k in ALL1 if k not in ("Ti", "amp3"))   # (in the EPW window T_i cancels from chi_i's asymptote: no derivative to check)
MULTI = ("Te", "ne", "Ti", "Z", "lam", "amp1", "amp3")

_FUSED = lambda n, gm, zh, ex: (f"k_fused_prep<{n}>", f"k_spectrum_fused<{n}, {gm}, {zh}, {ex}>", f"k_fused_finish<{n}>")
_ROWS = lambda n, gm, zh, ex: (f"k_spectrum_rows<{n}, {gm}, {zh}, {ex}, false>",)
_TWO = lambda n, gm, zh: (f"k_spectrum<{n}, 1, {gm}, 256, {zh}>",)
_M = ("k_fe_vectors<1>", "k_wgemm_w")

CASES = {
    # the one-sweep kernel, one ion: every scalar leaf, the four loss functionals, with and without the lane exchange
    "one_sweep_l2": (dict(), 3, 0, _FUSED(1, 0, "false", "true")),
    "one_sweep_l2_noex": (dict(), 3, 8, _FUSED(1, 0, "false", "false")),
    "one_sweep_l1": (dict(loss="l1", offset=0.05), 3, 0, _FUSED(1, 0, "false", "true")),
    "one_sweep_l1_noex": (dict(loss="l1", offset=0.05), 3, 8, _FUSED(1, 0, "false", "false")),
    "one_sweep_logcosh": (dict(loss="log-cosh"), 3, 0, _FUSED(1, 0, "false", "true")),
    "one_sweep_logcosh_noex": (dict(loss="log-cosh"), 3, 8, _FUSED(1, 0, "false", "false")),
    "one_sweep_poisson": (dict(loss="poisson"), 3, 0, _FUSED(1, 0, "false", "true")),
    "one_sweep_poisson_noex": (dict(loss="poisson"), 3, 8, _FUSED(1, 0, "false", "false")),
    # two ions, both fractions trainable: ion-2's Ti tied / free
    "one_sweep_2ion_fract_tied": (dict(n_ion=2, fract=True, tie=(2,)), 3, 0, _FUSED(2, 0, "false", "true")),
    "one_sweep_2ion_fract_free": (dict(n_ion=2, fract=True), 3, 0, _FUSED(2, 0, "false", "true")),
    "one_sweep_half_table": (dict(nvx=256), 3, 0, _FUSED(1, 0, "true", "true")),
    "one_sweep_17_angles": (dict(nang=17), 3, 0, _FUSED(1, 0, "false", "false")),
    # the rows kernel: split rounds (default) and one workgroup for all rounds (plan 1)
    "rows_ppp2": (dict(ppp=2), 3, 0, _ROWS(1, 0, "false", "true")),
    "rows_ppp2_one_wg": (dict(ppp=2), 3, 1, _ROWS(1, 0, "false", "true")),
    "rows_ppp2_2ion_fract": (dict(ppp=2, n_ion=2, fract=True), 3, 0, _ROWS(2, 0, "false", "true")),
    "rows_ppp2_2ion_fract_one_wg": (dict(ppp=2, n_ion=2, fract=True), 3, 1, _ROWS(2, 0, "false", "true")),
    "rows_ppp5": (dict(ppp=5, nvx=256), 2, 0, _ROWS(1, 0, "true", "true")),
    "rows_ppp5_one_wg": (dict(ppp=5, nvx=256), 2, 1, _ROWS(1, 0, "true", "true")),
    "rows_ppp5_2ion_fract": (dict(ppp=5, nvx=256, n_ion=2, fract=True), 2, 0, _ROWS(2, 0, "true", "true")),
    # the two-sweep kernel: three gradient points, three and four ions, and where the plan asks for it
    "two_sweep_G3": (dict(n_ion=2, G=3, leaves=GRAD), 3, 0, _TWO(2, 0, "false")),
    "two_sweep_G3_ppp2": (dict(n_ion=2, G=3, leaves=GRAD, ppp=2), 3, 0, _TWO(2, 0, "true")),
    "two_sweep_3ion": (dict(n_ion=3, leaves=MULTI, fract=True, tie=(3,)), 3, 0, _TWO(3, 0, "false")),
    "two_sweep_4ion": (dict(n_ion=4, leaves=MULTI, fract=True), 3, 0, _TWO(4, 0, "false")),
    "two_sweep_plan2": (dict(), 3, 2, _TWO(1, 0, "false")),
    "two_sweep_plan3": (dict(), 3, 3, _TWO(1, 0, "false")),
    # the DLM order a leaf
    "dlm_one_sweep": (dict(leaves=ALL1 + ("m",)), 3, 0, _M + _FUSED(1, 1, "false", "true")),
    "dlm_rows_ppp2": (dict(leaves=ALL1 + ("m",), ppp=2), 3, 0, _M + _ROWS(1, 1, "false", "true")),
    # one loaded feature (the gradient written directly), one fitted EPW range
    "epw_only": (dict(load="ele", leaves=EPW), 3, 0, _FUSED(1, 0, "false", "true")),
    "iaw_only": (dict(load="ion"), 3, 0, _FUSED(1, 0, "false", "true")),
    "red_only": (dict(blue=False), 3, 0, _FUSED(1, 0, "false", "true")),
    # workgroup f * B + b at an odd B: the per-feature partial gradients meet in the finish kernel
    "interleaved_B5": (dict(n_ion=2, fract=True), 5, 0, _FUSED(2, 0, "false", "true")),
}


def _deck_key(name):
    d, B, _, _ = CASES[name]
    return repr(sorted(d.items())), B


DECKS = {}   # one representative case name per (deck, B): the CPU references are per deck, the plans share them
for _n in CASES:
    DECKS.setdefault(_deck_key(_n), _n)
DECK_CASES = sorted(DECKS.values())


def _deck(d):
    n = d.get("n_ion", 1)
    leaves = d.get("leaves", GRAD if d.get("G", 1) > 1 else ALL1)
    cfg = decks.deck_fit(points_per_pixel=d.get("ppp", 1), nvx=d.get("nvx", 128), active=leaves, n_ion=n)
    P = cfg["parameters"]
    if d.get("G", 1) > 1:
        P["general"]["Te_gradient"].update(val=3.0, num_grad_points=d["G"])
        P["general"]["ne_gradient"].update(val=4.0, num_grad_points=d["G"])
    for s in range(1, n + 1):
        P[f"ion-{s}"]["fract"]["active"] = bool(d.get("fract"))
        P[f"ion-{s}"]["Ti"]["same"] = s in d.get("tie", ())
    cfg["optimizer"]["loss_method"] = d.get("loss", "l2")
    cfg["data"]["ele_lam_shift"] = 0.3
    assert cfg["other"]["iawfilter"][0]
    ext = cfg["other"]["extraoptions"]
    if d.get("load") == "ele":
        ext.update(load_ion_spec=False, fit_IAW=False)
    if d.get("load") == "ion":
        ext.update(load_ele_spec=False, fit_EPWb=False, fit_EPWr=False)
    if not d.get("blue", True):
        ext["fit_EPWb"] = False
    return cfg


def _names_and_mask(cfg):
    """(trainable leaves as test_kernel_matrix._trained names them -- a tied Ti is not one --, the gradient mask [NP]).  The
    fractions are leaves where the deck says so: SlotMap gives them their activation and leaves the mask to the caller."""
    sm = SlotMap(cfg["parameters"], True)
    gm = sm.active.astype(np.uint8)
    order = ["Te", "ne", "m", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]
    for s, sp in enumerate(sm.species):
        order += [f"Ti_{s + 1}", f"Z_{s + 1}", f"fract_{s + 1}"]
        if cfg["parameters"][sp]["fract"]["active"]:
            gm[util.slot_of(f"fract_{s + 1}")] = 1
        if sm.ti_same[s]:
            gm[util.slot_of(f"Ti_{s + 1}")] = 0
    return [k for k in order if gm[util.slot_of(k)]], gm


@functools.lru_cache(maxsize=None)
def _inputs(name):
    d, B, _, _ = CASES[name]
    cfg = _deck(d)
    n_ion = d.get("n_ion", 1)
    nang = d.get("nang", 10)
    sa = util.sa_fit(B) if nang == 10 else dict(sa=np.linspace(53.6, 66.1, nang), weights=np.ones((B, nang)) / nang)
    # (the data of a one-feature deck: drawn with both features loaded, the other feature's then unused)
    batch = util.synthetic_batch(_deck({k: v for k, v in d.items() if k != "load"}), sa, B, seed=40 + SEED)
    for k in ("e_data", "i_data"):   # (l1: a background under the data keeps |d - T| off zero in the wings, where both vanish)
        batch[k] = batch[k] + d.get("offset", 0.0) * batch[k].max()
    batch["noise_e"][B - 1] = 0.0
    batch["noise_i"][B - 1] = 0.0
    ranges = dict(ud=(-0.8, 0.8), Z_1=(4.0, 12.0))
    if "m" in d.get("leaves", ()):
        ranges["m"] = (2.1, 4.3)
    ranges.update({f"Ti_{s}": (0.05, 0.5) for s in range(2, n_ion + 1) if s not in d.get("tie", ())})
    if n_ion >= 3:   # (every Z a leaf there; the two-ion deck's Z_2 is not one)
        ranges.update(dict(Z_2=(0.8, 2.0), Z_3=(4.0, 8.0), Z_4=(1.5, 3.0)))
    if d.get("fract"):   # raw fractions of a lineout: their sum anywhere in (0.2, 3.6), never 1
        ranges.update({f"fract_{s}": (0.1, 0.9) for s in range(1, n_ion + 1)})
    normed = util.random_lineouts(cfg, B, seed=70 + SEED, ranges=ranges)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    names, gm = _names_and_mask(cfg)
    return dict(cfg=cfg, sa=sa, B=B, n_ion=n_ion, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, names=names, gm=gm,
                X=util.normed_to_matrix(normed, n_ion), slots=[util.slot_of(k) for k in names])


_TWIN = {}    # deck key -> the inputs and the twin's own-seed result (small arrays), every deck
_GRAPH = {}   # deck key -> the twin's stage graph and per-point Jacobians (ot.loss_adjoint's cache): the last deck's only


def _twin(name):
    key = _deck_key(name)
    if key not in _TWIN:
        _graph(name)
    return _TWIN[key]


def _graph(name):
    """the seed-independent part of the twin's adjoint for the case's deck, shared by its plans; building it gives _TWIN's entry"""
    key = _deck_key(name)
    if key not in _GRAPH:
        _GRAPH.clear()
        s = _inputs(DECKS[key])
        _GRAPH[key] = {}
        g, A, E, I = ot.loss_adjoint(s["cfg"], s["sa"], s["normed"], s["batch"], s["i_norm"], s["e_norm"], s["names"], cache=_GRAPH[key])
        _TWIN.setdefault(key, dict(s, g=g, A=A, E=E, I=I))
    return _GRAPH[key]


def _ratio(err, A):
    return err / np.where(A > 0, A, 1.0)


def _assert_entries(what, names, dev, ref, A, tol):
    """|dev - ref| <= tol * A for every (lineout, leaf); the worst one reported"""
    err = np.abs(dev - ref)
    r = _ratio(err, A)
    print(what, "max |. - twin| / A per leaf:", {k: float("%.2e" % r[:, c].max()) for c, k in enumerate(names)},
          "entries with A = 0:", int((A == 0).sum()))
    b, c = np.unravel_index(np.argmax(err - tol * A), err.shape)
    assert np.all(err <= tol * A), (what, "lineout", b, names[c], "got", dev[b, c], "twin", ref[b, c], "A", A[b, c], "ratio", r[b, c])


@pytest.mark.parametrize("name", DECK_CASES)
def test_twin_terms_sum_to_reverse_mode(name):
    """The sum of the twin's terms is its reverse-mode gradient, to 1e-12 of A (largest measured: 1e-13).  For the DLM order the terms
    are those of every (point, table node): d P / d m of one point is a cancelling sum over the f_e and W nodes the point reads, and
    summed per point its rounding reaches 1e-12 of the per-point accumulation."""
    t = _twin(name)
    val, ref, E, I = ot.value_and_grad(t["cfg"], t["sa"], t["normed"], t["batch"], t["i_norm"], t["e_norm"], t["names"])
    R = np.stack([ref[k] for k in t["names"]], axis=1)
    assert np.array_equal(E, t["E"]) and np.array_equal(I, t["I"])
    assert np.all(np.isfinite(t["g"])) and np.all(t["A"] >= np.abs(t["g"]) * (1 - 1e-12))
    _assert_entries(name + " reverse mode", t["names"], R, t["g"], t["A"], 1e-12)


def _twin_sums(t):
    """(masked sums [3], their entry counts, the loss) of the twin at its own spectra"""
    if "S" not in t:
        S, N, _, _ = ot.masked_sums(t["cfg"], t["sa"], {k: ot._t(v) for k, v in t["normed"].items()}, t["batch"])
        t["S"] = (S.numpy(), N, float(ot._loss_of_sums(t["cfg"], S, N, t["i_norm"], t["e_norm"])))
    return t["S"]


def _twin_weights(t):
    """the factor of each masked sum in the twin's loss (what Engine.loss_weights gives on the device)"""
    import torch

    N = _twin_sums(t)[1]
    return np.array([float(ot._loss_of_sums(t["cfg"], torch.eye(3, dtype=ot.DT)[k], N, t["i_norm"], t["e_norm"])) for k in range(3)])


@pytest.mark.parametrize("name", [n for n in DECK_CASES if "m" not in CASES[n][0].get("leaves", ())])
def test_reference_floor(name):
    """The two references -- the C++ oracle's forward-mode dual numbers and the twin as it stands, each at its own spectra -- agree
    within TOL / 100 of A, entry by entry (largest measured: 7e-10, the ion feature's leaves)."""
    from oracle import c_oracle as co

    t = _twin(name)
    w = _twin_weights(t)
    sums, gref, Eo, Io = co.loss_grad(t["cfg"], t["sa"], t["X"], t["batch"], w=w, gmask=t["gm"])
    off = np.ones(gref.shape[1], dtype=bool)
    off[t["slots"]] = False
    assert np.all(gref[:, off] == 0.0)
    _assert_entries(name + " C++ oracle", t["names"], gref[:, t["slots"]], t["g"], t["A"], TOL / 100)


@pytest.mark.parametrize("name", DECK_CASES)
def test_no_point_on_a_kink(name):
    """From the oracle's own intermediates: every point's xi_e keeps KINK of a cell from the vx nodes and xi_i from the Z' nodes, no
    row maximum is tied, m keeps off the DLM axis' nodes, and under l1 no fitted bin has |d - T| below KINK * max T."""
    t = _twin(name)
    cfg, sa, B, n_ion = t["cfg"], t["sa"], t["B"], t["n_ion"]
    ext = cfg["other"]["extraoptions"]
    G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
    vx = orc.velocity_grid(cfg["parameters"]["electron"]["fe"]["nvx"])
    _, xi2 = orc.xi_grids()
    phys = orc.physical_params(cfg["parameters"], t["normed"], True)
    worst = dict(xe=np.inf, xi=np.inf)
    for b in range(B):
        p = orc.lineout_params(phys, b, n_ion)
        if "m" in t["names"]:
            assert util.node_distance(p["m"], orc.DLM_M_AXIS) >= KINK
        fe = orc.lineout_fe(cfg, p)[1]
        for f, feature, on in ((0, "ele", ext["load_ele_spec"]), (1, "ion", ext["load_ion_spec"])):
            if not on:
                continue
            for g in range(G):
                for s in range(n_ion):
                    xe, xi = util.positions(cfg, sa, p, f, ion=s, grad_point=g)
                    worst["xe"] = min(worst["xe"], util.node_distance(xe, vx).min())
                    worst["xi"] = min(worst["xi"], util.node_distance(xi, xi2).min())
            lam, modl = orc.model_spectrum(cfg, sa, p, vx, fe, feature)
            wid = cfg["other"]["PhysParams"]["widIRF"]
            y = orc._gauss_same(lam, modl, wid["spect_stddev_ele" if f == 0 else "spect_stddev_ion"])
            for row in (modl, y, np.average(y.reshape(1024, -1), axis=1)):
                top = np.sort(row)[-2:]
                assert top[1] > top[0], (name, b, feature, "tied row maximum")
    print(name, "nearest node, cells: xi_e on vx %.2e, xi_i on Z' %.2e" % (worst["xe"], worst["xi"]))
    assert worst["xe"] >= KINK and worst["xi"] >= KINK, (name, worst)
    if cfg["optimizer"]["loss_method"] == "l1":
        lamE, lamI = orc.ts_diag(cfg, sa, t["normed"], t["batch"])[2:]
        iaw, blue, red = orc.fit_masks(cfg, lamE, lamI)
        for T, d, mask, on in ((t["E"], t["batch"]["e_data"], (blue & bool(ext["fit_EPWb"])) | (red & bool(ext["fit_EPWr"])), True),
                               (t["I"], t["batch"]["i_data"], iaw, ext["fit_IAW"])):
            if on:
                assert np.abs(d - T)[mask].min() >= KINK * T.max(), (name, np.abs(d - T)[mask].min())


QUIET = ("Te_gradient", "ne_gradient", "ud", "fract", "minority Ti")


def test_cases_contain_quiet_entries():
    """What the global and the column scale cannot see: in at least one case each of Te_gradient, ne_gradient, ud, a fraction and a
    minority species' Ti has an entry below 1e-3 of the case's largest |g| whose |g| / A is above 1e-3 (a real signal, not a residue)."""
    found = {k: [] for k in QUIET}
    for name in DECK_CASES:
        t = _twin(name)
        g, A = np.abs(t["g"]), t["A"]
        rel, sig = g / g.max(), g / np.where(A > 0, A, 1.0)
        print(name)
        for c, k in enumerate(t["names"]):
            print("   %-12s |g| / max |g| %s   |g| / A %s" % (k, " ".join("%.1e" % v for v in rel[:, c]), " ".join("%.1e" % v for v in sig[:, c])))
            kind = "fract" if k.startswith("fract_") else "minority Ti" if (k.startswith("Ti_") and k != "Ti_1") else k
            if kind in found and np.any((rel[:, c] < 1e-3) & (sig[:, c] > 1e-3)):
                found[kind].append(name)
    print({k: v for k, v in found.items()})
    assert all(found.values()), found


def test_named_kernels_are_in_the_library():
    from tsadar_amd import build

    build.build()
    shipped = _library_kernels(build.OUT)
    named = {k for c in CASES.values() for k in c[3]}
    assert not sorted(named - shipped), sorted(named - shipped)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


_ENGINES = {}


def _engine(name, t):
    from tsadar_amd.engine import Engine

    key = _deck_key(name)
    if key not in _ENGINES:
        _ENGINES.clear()
        _ENGINES[key] = Engine(t["cfg"], t["sa"])
    return _ENGINES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES, key=lambda n: (_deck_key(n), n)))
def test_loss_grad_entries_match_twin(torch_mod, name):
    """Engine.loss_grad under the case's plan: the kernels it names launched, the spectra and the loss at the suite's bounds, and
    every gradient entry within TOL of its own absolute accumulation A of the twin's adjoint seeded at the device's spectra."""
    _, B, plan, kernels = CASES[name]
    t = _twin(name)
    eng = _engine(name, t)
    cfg, names = t["cfg"], t["names"]
    eng.set_launch_plan(plan)
    w = eng.loss_weights(B, t["i_norm"], t["e_norm"], cfg["data"]["ion_loss_scale"])
    terms, grad, E, I = eng.loss_grad(t["X"], t["batch"], w, t["gm"], want_spectra=True)
    torch_mod.cuda.synchronize()
    got = eng.last_launch()
    print(name, "plan", plan, got)
    missing = [k for k in kernels if k not in got]
    assert not missing, f"expected {missing} among the launched kernels {got}"
    terms, grad, E, I = (a.cpu().numpy() for a in (terms, grad, E, I))
    ext = cfg["other"]["extraoptions"]
    if ext["load_ele_spec"]:
        assert util.rel_err(E, t["E"]) < 1e-8, util.rel_err(E, t["E"])
    if ext["load_ion_spec"]:
        assert util.rel_err(I, t["I"]) < 1e-7, util.rel_err(I, t["I"])
    val = _twin_sums(t)[2]
    assert abs(float(np.dot(terms, w)) - val) <= 1e-9 * abs(val), (float(np.dot(terms, w)), val)
    g, A, _, _ = ot.loss_adjoint(cfg, t["sa"], t["normed"], t["batch"], t["i_norm"], t["e_norm"], names,
                                 seed_from=(E if ext["load_ele_spec"] else t["E"], I if ext["load_ion_spec"] else t["I"]), cache=_graph(name))
    off = np.ones(grad.shape[1], dtype=bool)
    off[t["slots"]] = False
    assert np.all(grad[:, off] == 0.0), np.nonzero(grad[:, off])
    assert np.all(np.isfinite(grad))
    _assert_entries(f"{name} plan {plan} device", names, grad[:, t["slots"]], g, A, TOL)
