"""tsff_form_factor_2d_jvp (Engine.form_factor_2d_jvp): forward mode of the 2-D form factor for arbitrary directions of the physical
parameters and of the table, SphericalHarmonics.jvp, and the host side of the 2-D angular post-fit path.

The yardstick is the torch twin as it stands: one reverse pass of ``ot.form_factor_2d`` per seeded point (``ot.ff2d_adjoint`` on a
single point with a unit seed) gives dP/d(every name of ``ot.phys_names_2d``) and dP/d(table), contracted with each direction.  A
CPU test pins that yardstick to central differences of the NumPy oracle before the device is compared with it.  Every row -- one
direction's P_dot over the seeded points of one (lineout, gradient point) -- lies within ROW_TOL of its own largest entry in the
twin; a row that is identically zero in the twin is exactly zero on the device.  Every seeded point is compared, at most 40 per
parametrised case.

Directions: phys_dot random over the names of ``phys_names_2d`` (a tenth of each value's scale, lam a hundredth), a table direction
= the table times a smooth function of (vx, vy).  The kinds of a case's directions are listed in CASES: phys only ("p"), table only
("t"), both ("b"), identically zero ("0").  The cases of fewer than four directions cannot hold all four kinds; the zero table
tangent is also checked on nv = 132 against the call without table directions."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import angular_twin as at
import decks
import util
from oracle import tsadar_oracle as orc
from oracle import tsadar_oracle_torch as ot
from tsadar_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "ff2d_jvp_pytest.txt")
KINK = 1e-6   # cells: no seeded point closer than this to a vx node (|xi_e|) or to a node of the Z' table (xi_i)


def record(key, text):
    """One line per case in profiles/ff2d_jvp_pytest.txt: the case's previous line is replaced."""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    lines = {}
    if os.path.exists(RECORD):
        lines = {l.split(" ", 1)[0]: l.rstrip("\n") for l in open(RECORD) if l.strip()}
    lines[key] = f"{key} {text}"
    with open(RECORD, "w") as f:
        f.write("".join(v + "\n" for _, v in sorted(lines.items())))


# nv = 96: a case of this file's own, by the recipe of util.ff2d_twin_case -- the table in LDS, 2 parts, the largest nv of the
# pitch = 1 (mod 32) rule
_CASE96 = dict(n_ion=1, G=1, sa=[35.0, 60.0, 110.0], lam={0: [262, 333, 431, 610], 1: [100, 236, 511]}, drifts=[(None, 25.0, -40.0)])


@functools.lru_cache(maxsize=None)
def _case(nv):
    if nv != 96:
        return util.ff2d_twin_case(nv)
    c = _CASE96
    cfg = decks.deck_fit(n_ion=c["n_ion"])
    B = 2
    sa = dict(sa=np.array(c["sa"]), weights=np.ones((B, len(c["sa"]))) / len(c["sa"]))
    normed = util.random_lineouts(cfg, B, seed=67, ranges=dict(ud=(-1.5, 1.5)))
    phys = orc.physical_params(cfg["parameters"], normed, True)
    phys["ud"] = np.array([0.8, -1.1])
    vx, fe2 = util.fe2d(nv)
    return dict(cfg=cfg, sa=sa, B=B, G=c["G"], n_ion=c["n_ion"], phys=phys, vx=vx, fe2=fe2, lam=c["lam"], drifts=c["drifts"], nv=nv)


# id -> (nv, feature, drift setting, seeded wavelength samples, kinds of the directions)
CASES = {
    "nv48_ele": (48, 0, 0, [333, 431], "ptb0bpt"),     # LDS, 4 parts, two ions, G = 3; launch groups 3, 3, 1
    "nv48_ion": (48, 1, 0, [100, 511], "ptb0bpt"),
    "nv96_ele": (96, 0, 0, [262, 333, 431, 610], "ptb0"),
    "nv96_ion": (96, 1, 0, [100, 236, 511], "ptb0"),
    "nv132_d0": (132, 1, 0, [231, 234, 235], "ptb"),   # L1/L2 path, 1 part, the second padded buffer; the laser line between 234 and 235
    "nv132_d1": (132, 1, 1, [231, 234, 235], "ptb"),   # the other orientation of the table copy
    "nv133_ele": (133, 0, 0, [280, 430], "b"),         # odd sample count per line
    "nv133_ion": (133, 1, 0, [236], "b"),
}


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    nv, feature, drift, lam, kinds = CASES[cid]
    case = dict(_case(nv))
    case["lam"] = {feature: lam}
    ud, ud_ang, va_ang = case["drifts"][drift]
    _, X, lineouts = util.ff2d_with_drift(case, ud)
    B, NP = X.shape
    n_dir = len(kinds)
    rng = np.random.default_rng(1000 * nv + 10 * drift + feature)
    names = ot.phys_names_2d(case["n_ion"])
    pd = np.zeros((n_dir, B, NP))
    for nm in names:
        s = util.slot_of(nm)
        pd[:, :, s] = rng.normal(size=(n_dir, B)) * 0.1 * np.maximum(np.abs(X[None, :, s]), 0.05) * (1e-2 if s == L.P_LAM else 1.0)
    VX, VY = np.meshgrid(case["vx"], case["vx"], indexing="ij")
    fd = np.zeros((n_dir, nv, nv))
    for k in range(n_dir):
        a, wx, wy, ph = rng.normal(size=3), rng.uniform(0.3, 1.5, 3), rng.uniform(0.3, 1.5, 3), rng.uniform(0, 6.28, 3)
        fd[k] = case["fe2"] * sum(a[i] * np.cos(wx[i] * VX + wy[i] * VY + ph[i]) for i in range(3))
    for k, kind in enumerate(kinds):
        if kind in "t0":
            pd[k] = 0.0
        if kind in "p0":
            fd[k] = 0.0
    npoint = B * case["G"] * len(lam) * len(case["sa"]["sa"])
    assert npoint <= 40, npoint
    return dict(case=case, feature=feature, lam=np.array(lam), angles=(ud_ang, va_ang), X=X, lineouts=lineouts, pd=pd, fd=fd,
                with_table="t" in kinds or "b" in kinds, names=names, n_dir=n_dir, nv=nv)


def _lam_shift(s):
    return s["case"]["cfg"]["data"].get("ele_lam_shift", 0.0) if s["feature"] == 0 else 0.0


def _twin_point_grads(s, b, g, l, t):
    """dP/d(names) [len(names)] and dP/d(table) [nv, nv] of one seeded point: one reverse pass of the twin."""
    case = s["case"]
    seed = np.zeros((case["B"], case["G"], s["lam"].size, len(case["sa"]["sa"])))
    seed[b, g, l, t] = 1.0
    gp, gt, _, _ = ot.ff2d_adjoint(util.ff2d_lam_range(case, s["feature"]), 1024, _lam_shift(s), case["sa"]["sa"], case["G"], s["lineouts"],
                                   case["vx"], case["fe2"], s["angles"][0], s["angles"][1], s["lam"], seed, s["names"], points=[(b, g, l, t)])
    return gp[b], gt


@functools.lru_cache(maxsize=None)
def _twin(cid):
    """The twin's P_dot [n_dir, B, G, n_lam, n_angles] on the seeded points of the case: computed once, shared, never modified."""
    s = _inputs(cid)
    case = s["case"]
    shape = (case["B"], case["G"], s["lam"].size, len(case["sa"]["sa"]))
    slots = [util.slot_of(nm) for nm in s["names"]]
    out = np.zeros((s["n_dir"],) + shape)
    for (b, g, l, t) in np.ndindex(*shape):
        gp, gt = _twin_point_grads(s, b, g, l, t)
        for k in range(s["n_dir"]):
            out[k, b, g, l, t] = float(np.dot(gp, s["pd"][k, b, slots])) + float(np.sum(gt * s["fd"][k]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_twin_rows_match_oracle_differences():
    """The twin's rows along one direction of (Te, ne, lam, ud, Va) and along one table direction against central differences of the
    NumPy oracle on one lineout of the nv = 48 case, with the (h, h/2) ladder of
    tests/test_form_factor_jvp.py::test_twin_jvp_matches_oracle_differences: per row the pair of steps whose quotients agree best is
    taken and held to 1e-5 of the row's largest entry."""
    s = _inputs("nv48_ele")
    case, b = s["case"], 1
    shape = (case["G"], s["lam"].size, len(case["sa"]["sa"]))
    slots = [util.slot_of(nm) for nm in s["names"]]
    pdir = np.zeros(s["X"].shape[1])
    for nm in ("Te", "ne", "lam", "ud", "Va"):
        pdir[util.slot_of(nm)] = s["pd"][0, b, util.slot_of(nm)]
    tdir = s["fd"][1]
    assert np.any(pdir) and np.any(tdir)
    rows = np.zeros((2,) + shape)
    for (g, l, t) in np.ndindex(*shape):
        gp, gt = _twin_point_grads(s, b, g, l, t)
        rows[0, g, l, t] = float(np.dot(gp, pdir[slots]))
        rows[1, g, l, t] = float(np.sum(gt * tdir))

    def oracle(step, table):
        p = dict(s["lineouts"][b])
        if not table:
            for nm in ("Te", "ne", "lam", "ud", "Va"):
                p[nm] = p[nm] + step * pdir[util.slot_of(nm)]
        fe = case["fe2"] + (step * tdir if table else 0.0)
        return orc.form_factor_2d(util.ff2d_lam_range(case, 0), 1024, _lam_shift(s), case["sa"]["sa"], case["G"], p, case["vx"], fe,
                                  s["angles"][0], s["angles"][1], lam_index=s["lam"])[0]

    for which, table in ((0, False), (1, True)):
        quot = [(oracle(h, table) - oracle(-h, table)) / (2 * h) for h in (1e-3 / 2 ** i for i in range(8))]
        J = rows[which].reshape(case["G"], -1)
        best = None
        for q0, q1 in zip(quot[:-1], quot[1:]):
            q0, q1 = q0.reshape(case["G"], -1), q1.reshape(case["G"], -1)
            gap = np.max(np.abs(q0 - q1), axis=-1)
            pick = q1 if best is None else np.where((gap < best[0])[..., None], q1, best[1])
            best = (gap if best is None else np.minimum(gap, best[0]), pick)
        ratio = np.max(np.abs(best[1] - J), axis=-1) / np.max(np.abs(J), axis=-1)
        print(f"twin vs oracle differences, {'table' if table else 'parameters'}: {np.max(ratio):.3e}")
        assert np.max(ratio) < 1e-5, (which, ratio)


def _sph(flm_type, nvx=32, nvr=32):
    from tsadar_amd import distribution as Dist

    p = {"flm_type": flm_type, "init_m": 2.2, "Nl": 1, "nvr": nvr}
    if flm_type == "mora-yahi":
        p.update(LTx=225000.0, LTy=400000.0)
    sph = Dist.SphericalHarmonics({"active": True, "dim": 2, "type": "sphericalharmonic", "nvx": nvx, "params": p})
    if flm_type == "arbitrary":
        rng = np.random.default_rng(11)
        for key in sorted(sph.flm):
            sph.flm[key]["flm_sign"] = rng.normal(0.0, 1.0, nvr)
            sph.flm[key]["flm_mag"] = rng.normal(-1.0, 0.5, nvr)
    return sph


@pytest.mark.parametrize("flm_type", ["mora-yahi", "arbitrary"])
def test_sph_jvp_is_the_transpose_of_vjp(flm_type):
    """<fe_bar, jvp()[j]> = vjp(fe_bar)[j] for a random fe_bar: to rtol 1e-6 (central differences on one side; the entries are held
    on the scale of the largest of the vector), and to rounding where vjp is itself _vjp_fd (Mora-Yahi)."""
    sph = _sph(flm_type)
    theta = sph.get_params().copy()
    J = sph.jvp()
    assert J.shape == (theta.size, sph.nvx, sph.nvx) and np.array_equal(sph.get_params(), theta)
    fe_bar = np.random.default_rng(3).standard_normal((sph.nvx, sph.nvx))
    lhs = np.tensordot(J, fe_bar, axes=([1, 2], [0, 1]))
    rhs = sph.vjp(fe_bar)
    print(f"{flm_type}: max |<fe_bar, jvp> - vjp| / max |vjp| = {np.max(np.abs(lhs - rhs)) / np.max(np.abs(rhs)):.3e}")
    assert np.max(np.abs(lhs - rhs)) <= 1e-6 * np.max(np.abs(rhs))
    if flm_type == "mora-yahi":
        assert np.max(np.abs(lhs - sph._vjp_fd(fe_bar))) <= 1e-12 * np.max(np.abs(rhs))


def test_header_binding_and_export():
    import re

    hdr = open(os.path.join(ROOT, "include", "tsff.h")).read()
    ver = int(re.search(r"#define TSFF_ABI_VERSION (\d+)", hdr).group(1))
    assert ver == L.ABI_VERSION >= 18
    assert "tsff_form_factor_2d_jvp" in hdr and "tsff_form_factor_2d_jvp" in L.EXPORTS
    lib = C.CDLL(L.LIB_PATH)
    assert lib.tsff_abi_version() == ver
    assert hasattr(lib, "tsff_form_factor_2d_jvp")


CCD, START, END = (128, 256), 10, 110


def _sph_deck(flm_type="mora-yahi", nvx=32, active=True):
    cfg = decks.deck_angular(2, nvx, CCD, START, END)
    p = {"flm_type": flm_type, "init_m": 2.2, "Nl": 1, "nvr": nvx}
    if flm_type == "mora-yahi":
        p.update(LTx=225000.0, LTy=400000.0)
    cfg["parameters"]["electron"]["fe"] = {"active": active, "dim": 2, "type": "sphericalharmonic", "nvx": nvx, "params": p}
    return cfg


def _dummy_batch():
    rows = END - START
    return dict(e_data=np.ones((rows, 256)), i_data=np.zeros((rows, 256)), e_amps=np.ones((rows, 1)), i_amps=np.zeros(rows),
                noise_e=np.zeros((rows, 256)), noise_i=np.array([0.0]))


def test_2d_refusals_fire_before_an_engine_exists():
    import copy

    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    batch = _dummy_batch()
    big = _sph_deck()
    big["parameters"]["electron"]["fe"]["nvx"] = 258
    for cfg in (decks.deck_angular(2, 32, CCD, START, END), _sph_deck("nn"), big):   # an active Arbitrary2V.fval, flm_type nn, nv > 256
        sa = util._angular_sa(cfg)
        lf = LossFunction(cfg, sa, batch)
        tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
        before = copy.deepcopy(lf.cfg)
        for name in ("angular_jacobian", "angular_gn_loss_wrt_params"):
            with pytest.raises(NotImplementedError):
                getattr(lf, name)(tp, batch)
        assert lf.ts_diag._engines == {} and lf.cfg == before


def test_angular_directions_of_a_mora_yahi_deck():
    """The leaves in ravel order (Te, ne, the generator's values, lam), table directions for exactly the generator's values."""
    from tsadar_amd import ThomsonParams, tree
    from tsadar_amd.loss_function import LossFunction

    cfg = _sph_deck()
    sa = util._angular_sa(cfg)
    lf = LossFunction(cfg, sa, _dummy_batch())
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    names, pd, fd, ad = lf._angular_directions(tp)
    n_gen = tp.sph.get_params().size
    assert n_gen == 3
    want = []
    for name, s in tree.get_filter_spec(None, tp):
        want += [(name[0], name[1], j) for j in range(n_gen)] if s == tree.GEN2D_SLOT else [name]
    assert names == want and ("electron", "fe", 0) in names
    assert pd.shape == (len(names), tp.slots.NP) and fd.shape == (len(names), 32, 32) and ad.shape == (len(names), 2)
    J = tp.sph.jvp()
    for k, nm in enumerate(names):
        if len(nm) == 3:
            assert np.array_equal(fd[k], J[nm[2]]) and not np.any(pd[k]) and np.any(fd[k])
        else:
            assert not np.any(fd[k]) and np.count_nonzero(pd[k]) == 1
    assert lf.ts_diag._engines == {}


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _engine(nv):
    from tsadar_amd.engine import Engine

    case = _case(nv)
    return Engine(case["cfg"], case["sa"])


def _call(eng, s, **kw):
    return eng.form_factor_2d_jvp(s["feature"], s["X"], s["case"]["fe2"], s["pd"], s["fd"] if s["with_table"] else None,
                                  s["angles"][0], s["angles"][1], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_form_factor_2d_jvp_matches_twin(torch_mod, cid):
    s = _inputs(cid)
    case, eng = s["case"], _engine(s["nv"])
    beta, d_e, d_i = util.ff2d_kink_distances(case, s["feature"], s["lineouts"], *s["angles"])
    assert d_e.min() >= KINK, (cid, "|xi_e| on a vx node or outside the grid", d_e.min())
    assert d_i.min() >= KINK, (cid, "xi_i on a node of the Z' table", d_i.min())
    Pdt = _twin(cid)
    P, Pd = _call(eng, s, want_P=True)
    launched = eng.last_launch()
    n_ion = case["n_ion"]
    assert launched.count(f"k_ff2d_jvp<{n_ion}, 3>") == (s["n_dir"] + 2) // 3, launched
    assert sum("k_ff2d_project" in k for k in launched) == s["n_dir"], launched
    assert sum("k_form_factor_2d<" in k for k in launched) == 1 and any(k.startswith("k_form_factor_2d<") and k.endswith("true>") for k in launched), launched
    # the value: the saving forward's bit for bit
    assert torch_mod.equal(P, eng.form_factor_2d(s["feature"], s["X"], case["fe2"], *s["angles"], save=True))
    dev = Pd[:, :, :, torch_mod.as_tensor(s["lam"], device=Pd.device), :].cpu().numpy()
    assert dev.shape == Pdt.shape and np.all(np.isfinite(dev))
    rows = lambda a: a.reshape(a.shape[0], a.shape[1], a.shape[2], -1)   # one direction x (lineout, gradient point)
    ratio = at.row_ratios(rows(dev), rows(Pdt))
    for k, kind in enumerate(CASES[cid][4]):
        if kind == "0":
            assert not np.any(Pdt[k]) and not bool(Pd[k].any())
    record(f"form_factor_2d_jvp[{cid}]", f"max row ratio {np.max(ratio):.3e} (bound {at.ROW_TOL:.0e}, {Pdt[0].size} points)")
    print(f"form_factor_2d_jvp[{cid}] max row ratio {np.max(ratio):.3e}")
    assert np.max(ratio) <= at.ROW_TOL, ratio
    # two calls give the same bits; without the value too
    none, Pd2 = _call(eng, s)
    assert none is None and torch_mod.equal(Pd, Pd2)


@pytest.mark.gpu
def test_form_factor_2d_jvp_point_ranges_and_table_switch(torch_mod):
    """nv = 132: three point ranges cut inside a lineout, one of them three points long, equal the whole call bit for bit; points
    outside a range keep the fill value they had; k_ff2d_project runs only when a table direction is present; a zero table tangent
    gives the values of the call without table directions."""
    torch = torch_mod
    s = _inputs("nv132_d0")
    case, eng = s["case"], _engine(132)
    P, Pd = _call(eng, s, want_P=True)
    na = Pd.shape[4]
    total = P.numel()
    per_bg = P.shape[2] * na
    cuts = [234 * na + 2, 234 * na + 5, per_bg + 235 * na + 1]
    assert all(c % per_bg for c in cuts) and cuts[1] - cuts[0] == 3
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        Pr, Pdr = _call(eng, s, want_P=True, point_range=(lo, hi))
        assert torch.equal(Pr.reshape(-1)[lo:hi], P.reshape(-1)[lo:hi]) and not bool(Pr.reshape(-1)[:lo].any()) and not bool(Pr.reshape(-1)[hi:].any())
        flat, ref = Pdr.reshape(s["n_dir"], -1), Pd.reshape(s["n_dir"], -1)
        assert torch.equal(flat[:, lo:hi], ref[:, lo:hi]) and not bool(flat[:, :lo].any()) and not bool(flat[:, hi:].any())
    # the fill value outside the range survives: through the raw ABI on a prefilled buffer
    lo, hi = cuts[0], cuts[1]
    p = eng._ptr
    X, fe, pdot, fdot = eng.dev(s["X"]), eng.dev(case["fe2"]), eng.dev(s["pd"]), eng.dev(s["fd"])
    out = torch.full((s["n_dir"], total), 7.0, dtype=torch.float64, device=eng.device)
    val = torch.full((total,), -3.0, dtype=torch.float64, device=eng.device)
    eng._sync_stream()
    rc = eng.lib.tsff_form_factor_2d_jvp(eng.h, 1, p(X), p(fe), 132, s["angles"][0], s["angles"][1], 2, s["n_dir"], p(pdot), p(fdot), lo, hi, p(val), p(out))
    assert rc == 0
    assert torch.equal(out[:, lo:hi], Pd.reshape(s["n_dir"], -1)[:, lo:hi]) and bool((out[:, :lo] == 7.0).all()) and bool((out[:, hi:] == 7.0).all())
    assert torch.equal(val[lo:hi], P.reshape(-1)[lo:hi]) and bool((val[:lo] == -3.0).all()) and bool((val[hi:] == -3.0).all())
    # no table direction: no projection kernel; a zero table tangent: the same values
    _, Pd_p = eng.form_factor_2d_jvp(1, s["X"], case["fe2"], s["pd"], None, *s["angles"])
    assert not any("k_ff2d_project" in k for k in eng.last_launch()), eng.last_launch()
    _, Pd_z = eng.form_factor_2d_jvp(1, s["X"], case["fe2"], s["pd"], np.zeros_like(s["fd"]), *s["angles"])
    assert sum("k_ff2d_project" in k for k in eng.last_launch()) == s["n_dir"]
    assert torch.equal(Pd_p, Pd_z)
    assert torch.equal(Pd_p[0], Pd[0])   # (direction 0 of the case carries no table tangent)


@pytest.mark.gpu
def test_form_factor_2d_jvp_return_codes(torch_mod):
    torch = torch_mod
    s = _inputs("nv48_ion")
    case, eng = s["case"], _engine(48)
    p = eng._ptr
    X, fe, pdot = eng.dev(s["X"]), eng.dev(case["fe2"]), eng.dev(s["pd"])
    n = s["n_dir"]
    out = torch.empty((n, 2, case["G"], 1024, 3), dtype=torch.float64, device=eng.device)
    call = lambda phys, tab, nv, pd, nd, o: eng.lib.tsff_form_factor_2d_jvp(eng.h, 1, p(phys), p(tab), nv, 25.0, -40.0, 2, nd, p(pd), p(None), 0, -1,
                                                                          p(None), p(o))
    eng._sync_stream()
    assert call(X, fe, 48, pdot, n, out) == 0
    assert call(X, fe, 48, None, n, out) == -1 and eng.last_launch() == []
    assert call(None, fe, 48, pdot, n, out) == -1
    assert call(X, fe, 48, pdot, n, None) == -1
    assert call(X, fe, 48, pdot, 0, out) == -1
    big = torch.zeros((257, 257), dtype=torch.float64, device=eng.device)
    assert call(X, big, 257, pdot, n, out) == -2 and eng.last_launch() == []
    # the call leaves no token behind, and an earlier save's is gone
    eng.form_factor_2d(1, s["X"], case["fe2"], 25.0, -40.0, save=True)
    tok = eng._saved_2d["token"]
    assert tok != 0 and call(X, fe, 48, pdot, n, out) == 0
    gp = torch.empty((2, eng.NP), dtype=torch.float64, device=eng.device)
    rc = eng.lib.tsff_form_factor_2d_grad(eng.h, 1, p(X), p(fe), 48, 25.0, -40.0, 2, 0, -1, C.c_uint64(tok), p(out[0]), p(gp), p(None))
    assert rc == -22
