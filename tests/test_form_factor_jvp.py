"""tsff_form_factor_jvp / tsff_ats_jvp (Engine.form_factor_jvp, Engine.ats_jvp): forward mode of the raw 1-D form factor for arbitrary
directions of the physical parameters and of f_e, and of the ARTS instrument chain, against the torch twin.

The yardstick is the twin as it stands (tests/angular_twin.py): ``ot.form_factor`` with ``ot.chi_table``, and ``ot.ats_spectrum``, one
``torch.autograd.functional.jvp`` per direction.  A CPU test pins that yardstick to central differences of the NumPy oracle before the
device is compared with it.  Every row -- one direction's P_dot of one lineout, one direction's image row -- lies within ROW_TOL of
its own largest entry in the twin; a row that is identically zero in the twin is exactly zero on the device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import angular_twin as at
import decks
import util
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "angular_jacobian_pytest.txt")
B = 3   # odd and > 1: lineout strides show
DOT_SLOTS = ("Te", "ne", "lam", "ud", "Va", "Ti", "Z")


def record(key, text):
    """One line per case in profiles/angular_jacobian_pytest.txt: the case's previous line is replaced."""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    lines = {}
    if os.path.exists(RECORD):
        lines = {l.split(" ", 1)[0]: l.rstrip("\n") for l in open(RECORD) if l.strip()}
    lines[key] = f"{key} {text}"
    with open(RECORD, "w") as f:
        f.write("".join(v + "\n" for _, v in sorted(lines.items())))


def _tie2(cfg):
    cfg["parameters"]["ion-2"]["Ti"]["same"] = True


def _grad3(cfg):
    g = cfg["parameters"]["general"]
    g["Te_gradient"].update(val=6.0, num_grad_points=3)
    g["ne_gradient"].update(val=9.0, num_grad_points=3)


# id -> (n_ion, nvx, deck modifiers, n_dir, fe directions: "all", "none" or the directions that carry one)
CASES = {
    "ni1_all": (1, 64, (), 7, "all"),                  # two full groups and a partial one of one direction
    "ni2_tied_G3": (2, 64, (_tie2, _grad3), 4, (0, 2)),   # a full group with fe_dot on two of its directions only, then one direction
    "ni3_tied_nvx320": (3, 320, (), 3, "all"),         # one full group; three table lanes at the production grid (118 KB of LDS)
    "ni4_none": (4, 64, (), 1, "none"),                # a single direction, no direction of f_e
    "ni1_none": (1, 64, (), 3, "none"),
}


def _free_form_fe(nb, nvx, seed):
    rng = np.random.default_rng(seed)
    vx = orc.velocity_grid(nvx)
    out = []
    for _ in range(nb):
        f = orc.dlm_fe(rng.uniform(2.0, 3.5), nvx) * np.exp(0.15 * np.sin(1.3 * vx + rng.uniform(0, 6.28)) + 0.05 * np.tanh(vx))
        out.append(f / np.sum(f) / (vx[1] - vx[0]))
    return np.stack(out)


def _directions(rng, X, fe, n_ion, n_dir, fe_dirs):
    """Random phys_dot over Te, ne, lam, ud, Va, Ti, Z (a tenth of each value's scale) and fe_dot = fe x smooth noise (a direction of
    ln f_e: the tails span 20 decades)."""
    nb, NP = X.shape
    nvx = fe.shape[1]
    pd = np.zeros((n_dir, nb, NP))
    slots = [util.slot_of(k) for k in ("Te", "ne", "lam", "ud", "Va")] + [util.slot_of(f"{k}_{s + 1}") for k in ("Ti", "Z") for s in range(n_ion)]
    for s in slots:
        pd[:, :, s] = rng.normal(size=(n_dir, nb)) * 0.1 * np.maximum(np.abs(X[None, :, s]), 0.05) * (1e-2 if s == L.P_LAM else 1.0)
    if fe_dirs == "none":
        return pd, None
    vx = orc.velocity_grid(nvx)
    fd = np.zeros((n_dir, nb, nvx))
    for k in (range(n_dir) if fe_dirs == "all" else fe_dirs):
        for b in range(nb):
            a, w, ph = rng.normal(size=3), rng.uniform(0.4, 2.0, 3), rng.uniform(0, 6.28, 3)
            fd[k, b] = fe[b] * sum(a[i] * np.cos(w[i] * vx + ph[i]) for i in range(3))
    return pd, fd


def _build(n_ion, nvx, mods, n_dir, fe_dirs, nb=B):
    """The inputs of a case (tests/test_forward_mode_plans_gpu.py builds its own with the same recipe)."""
    cfg = decks.deck_fit(nvx=nvx, n_ion=n_ion, active=("Te", "ne", "Ti", "Z", "Ti_same_3"))
    for m in mods:
        m(cfg)
    sa = util.sa_fit(nb)
    normed = util.random_lineouts(cfg, nb, seed=211, ranges=dict(ud=(-1.5, 1.5)))
    phys = orc.physical_params(cfg["parameters"], normed, True)
    X = util.normed_to_matrix(phys, n_ion)
    fe = _free_form_fe(nb, nvx, 9)
    pd, fd = _directions(np.random.default_rng(17), X, fe, n_ion, n_dir, fe_dirs)
    from tsadar_amd.params import SlotMap

    return dict(cfg=cfg, sa=sa, X=X, fe=fe, pd=pd, fd=fd, n_ion=n_ion, n_dir=n_dir, ti_same=SlotMap(cfg["parameters"], True).ti_same)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    return _build(*CASES[cid])


def _twin_of(s):
    """The twin's P and P_dot of the lineouts of ``s`` (_build)."""
    P, Pd = [], []
    for b in range(s["X"].shape[0]):
        p, d = at.form_factor_jvp(s["cfg"], s["sa"]["sa"], s["n_ion"], s["ti_same"], s["X"][b], s["fe"][b], s["pd"][:, b],
                                  None if s["fd"] is None else s["fd"][:, b])
        P.append(p)
        Pd.append(d)
    return np.array(P), np.array(Pd).transpose(1, 0, 2, 3, 4)   # [B, G, npts, NA], [n_dir, B, G, npts, NA]


@functools.lru_cache(maxsize=None)
def _twin(cid):
    """The twin's P and P_dot of the case's lineouts: computed once, shared by the tests, never modified."""
    return _twin_of(_inputs(cid))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the yardstick against central differences of the NumPy oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_twin_jvp_matches_oracle_differences():
    """The twin's jvp of the raw form factor along a direction of (Te, ne, lam) and of ln f_e against central differences of the
    NumPy oracle, with the (h, h/2) ladder of tests/test_jacobian.py: per row the pair of steps whose quotients agree best with each
    other is taken and held to 1e-5 of the row's largest entry."""
    s = _inputs("ni1_all")
    b, k = 1, 0
    _, Pd = at.form_factor_jvp(s["cfg"], s["sa"]["sa"], 1, s["ti_same"], s["X"][b], s["fe"][b], s["pd"][k:k + 1, b], s["fd"][k:k + 1, b])
    vx = orc.velocity_grid(64)
    names = ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]

    def oracle(t):
        x = s["X"][b] + t * s["pd"][k, b]
        fe = s["fe"][b] + t * s["fd"][k, b]
        p = {n: x[util.slot_of(n)] for n in names}
        p.update(Ti=[x[L.P_ION0 + L.ION_TI]], Z=[x[L.P_ION0 + L.ION_Z]], A=[x[L.P_ION0 + L.ION_A]], fract=[x[L.P_ION0 + L.ION_FRACT]])
        return orc.form_factor(s["cfg"]["other"]["lamrangE"], s["cfg"]["other"]["npts"], s["cfg"]["data"]["ele_lam_shift"], s["sa"]["sa"], 1, p, vx, fe)[0]

    quot = [(oracle(h) - oracle(-h)) / (2 * h) for h in (1e-3 / 2 ** i for i in range(8))]
    J = Pd[0].transpose(0, 2, 1)   # rows: one angle's spectrum
    best = None
    for q0, q1 in zip(quot[:-1], quot[1:]):
        q0, q1 = q0.transpose(0, 2, 1), q1.transpose(0, 2, 1)
        gap = np.max(np.abs(q0 - q1), axis=-1)
        pick = q1 if best is None else np.where((gap < best[0])[..., None], q1, best[1])
        best = (gap if best is None else np.minimum(gap, best[0]), pick)
    ratio = np.max(np.abs(best[1] - J), axis=-1) / np.max(np.abs(J), axis=-1)
    assert np.max(ratio) < 1e-5, np.max(ratio)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _engine(cid):
    from tsadar_amd.engine import Engine

    s = _inputs(cid)
    return Engine(s["cfg"], s["sa"], fe_mode=L.FE_PER_LINEOUT)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_form_factor_jvp_matches_twin(torch_mod, cid):
    s, eng = _inputs(cid), _engine(cid)
    Pt, Pdt = _twin(cid)
    P, Pd = eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"], want_P=True)
    launched = eng.last_launch()
    assert f"k_ffjvp<{s['n_ion']}, 3>" in launched, launched
    assert launched.count(f"k_ffjvp<{s['n_ion']}, 3>") == (s["n_dir"] + 2) // 3, launched
    assert ("k_fe_direction" in launched) == (s["fd"] is not None), launched
    # the value: tsff_form_factor's bit for bit
    assert torch_mod.equal(P, eng.form_factor(0, s["X"], s["fe"]))
    assert np.max(np.abs(P.cpu().numpy() - Pt) / np.abs(Pt)) < 1e-7
    # every (direction, lineout) row on its own scale
    ratio = at.row_ratios(Pd.cpu().numpy().reshape(s["n_dir"], B, -1), Pdt.reshape(s["n_dir"], B, -1))
    record(f"form_factor_jvp[{cid}]", f"max row ratio {np.max(ratio):.3e} (bound {at.ROW_TOL:.0e})")
    print(f"form_factor_jvp[{cid}] max row ratio {np.max(ratio):.3e}")
    assert np.max(ratio) <= at.ROW_TOL, ratio
    # two calls give the same bits; without the value too
    none, Pd2 = eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"])
    assert none is None and torch_mod.equal(Pd, Pd2)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["ni1_all", "ni2_tied_G3", "ni4_none"])
def test_form_factor_jvp_dot_product_identity(torch_mod, cid):
    """<Pbar, P_dot> = <grad_phys, phys_dot> + <grad_fe, fe_dot> against the shipped adjoint (tsff_form_factor_grad) for a random
    Pbar, within 1e-7 of sum |Pbar . P_dot|.  The adjoint returns a tied species' share in its own slot: its direction is ion 1's."""
    s, eng = _inputs(cid), _engine(cid)
    _, Pd = eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"])
    rng = np.random.default_rng(5)
    Pbar = torch_mod.as_tensor(rng.standard_normal(tuple(Pd.shape[1:])), device=Pd.device) / Pd.abs().mean()
    gp, gf = eng.form_factor_grad(0, s["X"], s["fe"], Pbar, want_fe=True)
    gp, gf = gp.cpu().numpy(), gf.cpu().numpy()
    pd = s["pd"].copy()
    for i in range(1, s["n_ion"]):
        if s["ti_same"][i]:
            pd[:, :, L.P_ION0 + 4 * i + L.ION_TI] = pd[:, :, L.P_ION0 + L.ION_TI]
    for k in range(s["n_dir"]):
        lhs = float((Pbar * Pd[k]).sum())
        rhs = float(np.sum(gp * pd[k])) + (float(np.sum(gf * s["fd"][k])) if s["fd"] is not None else 0.0)
        assert abs(lhs - rhs) <= 1e-7 * float((Pbar * Pd[k]).abs().sum()), (k, lhs, rhs)


@pytest.mark.gpu
def test_form_factor_jvp_angular_engine(torch_mod):
    """One plasma condition at the 241 angles of the ARTS calibration: the angles are spread over gridDim.y > 1."""
    cfg = decks.deck_angular(1, 64, (128, 256), 10, 110)
    sa = util._angular_sa(cfg)
    from tsadar_amd.engine import Engine

    eng = Engine(cfg, sa, fe_mode=L.FE_PER_LINEOUT)
    normed = util.random_lineouts(cfg, 1, seed=5)
    X = util.normed_to_matrix(orc.physical_params(cfg["parameters"], normed, True), 1)
    fe = _free_form_fe(1, 64, 3)
    pd, fd = _directions(np.random.default_rng(23), X, fe, 1, 2, (1,))
    Pt, Pdt = at.form_factor_jvp(cfg, sa["sa"], 1, np.zeros(4), X[0], fe[0], pd[:, 0], fd[:, 0])
    P, Pd = eng.form_factor_jvp(0, X, fe, pd, fd, want_P=True)
    assert tuple(Pd.shape) == (2, 1, 1, 1024, 241)
    assert torch_mod.equal(P, eng.form_factor(0, X, fe))
    ratio = at.row_ratios(Pd.cpu().numpy().reshape(2, -1), Pdt.reshape(2, -1))
    record("form_factor_jvp[angular]", f"max row ratio {np.max(ratio):.3e} (bound {at.ROW_TOL:.0e})")
    assert np.max(ratio) <= at.ROW_TOL, ratio
    # per angle too: every angle's spectrum of every direction on its own scale
    ratio = at.row_ratios(Pd.cpu().numpy().reshape(2, 1024, 241).transpose(0, 2, 1), Pdt.reshape(2, 1024, 241).transpose(0, 2, 1))
    assert np.max(ratio) <= at.ROW_TOL, np.max(ratio)


@pytest.mark.gpu
def test_form_factor_jvp_return_codes(torch_mod):
    torch = torch_mod
    s, eng = _inputs("ni1_none"), _engine("ni1_none")
    lib, h = eng.lib, eng.h
    X, fe, pd = eng.dev(s["X"]), eng.dev(s["fe"]), eng.dev(s["pd"])
    fdot = torch.zeros((3, B, 64), dtype=torch.float64, device=eng.device)
    out = torch.empty((3, B, 1, 1024, 10), dtype=torch.float64, device=eng.device)
    p = eng._ptr
    call = lambda phys, pdot, n, fd, o: lib.tsff_form_factor_jvp(h, 0, p(phys), p(fe), B, n, p(pdot), p(fd), p(None), p(o))
    assert call(X, pd, 3, None, out) == 0
    assert call(None, pd, 3, None, out) == -1 and eng.last_launch() == []
    assert call(X, None, 3, None, out) == -1
    assert call(X, pd, 3, None, None) == -1
    assert call(X, pd, 0, None, out) == -1
    assert call(X, pd, 3, fdot, out) == 0
    from tsadar_amd.engine import Engine

    shared = Engine(s["cfg"], s["sa"], fe_shared=s["fe"][0])   # fe_mode SHARED: no direction of f_e
    assert shared.fe_mode == L.FE_SHARED
    rc = shared.lib.tsff_form_factor_jvp(shared.h, 0, p(X), p(None), B, 3, p(pd), p(fdot), p(None), p(out))
    assert rc == -2 and shared.last_launch() == [] and b"PER_LINEOUT" in shared.lib.tsff_last_error(shared.h)
    Psh, Pdsh = shared.form_factor_jvp(0, s["X"], None, s["pd"], None, want_P=True)   # (the parameter directions run on a shared table)
    assert torch.equal(Psh, shared.form_factor(0, s["X"])) and bool(torch.isfinite(Pdsh).all())


# ---------------------------------------------------------------------------------------------------------------------
# tsff_ats_jvp
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ccd,n_lam,start,end", [((128, 256), 256, 10, 110), ((1024, 1024), 1024, 90, 950)])
def test_ats_jvp_matches_twin(torch_mod, ccd, n_lam, start, end):
    import torch
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd.engine import Engine

    cfg = decks.deck_angular(1, 64, ccd, start, end)
    sa = util._angular_sa(cfg)
    eng = Engine(cfg, sa, fe_mode=L.FE_PER_LINEOUT)
    wid = cfg["other"]["PhysParams"]["widIRF"]
    eng.ats_setup(sa["weights"], sa["angAxis"], wid["spect_FWHM_ele"] / 2.3548, wid["ang_FWHM_ele"] / 2.3548,
                  1024 // n_lam, 1024 // ccd[0], start, end)
    rows = end - start
    rng = np.random.default_rng(11)
    e_amps = rng.uniform(0.5, 2.0, (rows, 1))
    lam, a1, a2 = 526.5, 0.8, 1.3
    P = util.smooth_positive_image((1, 1024, 241), 1)
    Pdot = np.stack([util.smooth_positive_image((1, 1024, 241), 2) - 1.5, util.smooth_positive_image((1, 1024, 241), 3) - 1.4])
    amp_dot = np.array([[0.3, -0.7], [0.0, 0.0]])
    g = at.ats_fn(cfg, sa, n_lam, e_amps, lam)
    Et, Edt = None, []
    for k in range(2):
        Et, d = torch.autograd.functional.jvp(g, (ot._t(P), ot._t(np.array([a1, a2]))), (ot._t(Pdot[k]), ot._t(amp_dot[k])))
        Edt.append(d.numpy())
    # the twin's row maxima are unique: the arg-max the tangent goes through is defined
    modl = ot.ats_model(cfg, sa["weights"], ot._t(P), np.linspace(*cfg["other"]["lamrangE"], 1024))
    y = ot.add_ats_irf(cfg, sa["angAxis"], np.linspace(*cfg["other"]["lamrangE"], 1024), modl)
    unit = g(ot._t(P), ot._t(np.ones(2))).numpy() / e_amps   # the block means over their row maximum
    for img in (modl.numpy(), y.numpy(), unit):
        top = np.sort(img, axis=1)[:, -2:]
        assert np.all(top[:, 1] > top[:, 0])
    E, Ed = eng.ats_jvp(P, Pdot, e_amps, lam, a1, a2, amp_dot, want_E=True)
    assert eng.last_launch().count("k_ats_resunit_jvp") == 2 and "k_ats_rownorm_jvp" in eng.last_launch()
    assert torch_mod.equal(E, eng.ats_spectrum(P, e_amps, lam, a1, a2))
    ratio = at.row_ratios(Ed.cpu().numpy(), np.array(Edt))
    record(f"ats_jvp[{ccd[0]}x{ccd[1]}]", f"max row ratio {np.max(ratio):.3e} (bound {at.ROW_TOL:.0e})")
    assert np.max(ratio) <= at.ROW_TOL, np.max(ratio)
    # <Ebar, ThryE_dot> = <Pbar, P_dot> + <amp_bar, amp_dot> against the shipped adjoint
    Ebar = rng.normal(size=(rows, n_lam))
    Pbar, ab = eng.ats_adjoint(P, e_amps, lam, a1, a2, Ebar)
    Eb = eng.dev(Ebar)
    for k in range(2):
        lhs = float((Eb * Ed[k]).sum())
        rhs = float((Pbar * eng.dev(Pdot[k])).sum()) + ab[0] * amp_dot[k, 0] + ab[1] * amp_dot[k, 1]
        assert abs(lhs - rhs) <= 1e-7 * float((Eb * Ed[k]).abs().sum()), (k, lhs, rhs)
    none, Ed2 = eng.ats_jvp(P, Pdot, e_amps, lam, a1, a2, amp_dot)
    assert none is None and torch_mod.equal(Ed, Ed2)
