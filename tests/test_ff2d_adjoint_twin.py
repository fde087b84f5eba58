"""The adjoint of the 2-D form factor (tsff_form_factor_2d_grad) and of the ARTS instrument chain (tsff_ats_adjoint), entry by entry,
against reverse-mode autodiff of the oracle's torch twin (oracle/tsadar_oracle_torch.py: ff2d_adjoint, ats_adjoint).

Every table entry and every (lineout, parameter) is held to TOL times its own ABSOLUTE ACCUMULATION A: the sum over the seeded
points of the absolute value of each point's contribution, which is the scale at which two float64 summations of these terms
may differ.  max |g| is not that scale: the corners of the rotated grid lie outside the table, where the cubic boundary patch gives a
few rim entries weights orders of magnitude above everything else.  Where A is exactly 0 the bound is 0: inactive slots, and entries that
no seeded line touches.  The twin knows its own answer a hundred times better than TOL (test_twin_2d_adjoint_noise_floor).

The finite-difference tests of tests/test_gpu_parity.py pin the adjoint to the device's own forward; these pin it to the oracle."""
import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc
from oracle import tsadar_oracle_torch as ot
from tsadar_amd import _lib as L

pytestmark = pytest.mark.gpu

TOL = 1e-7   # the bound of the 1-D adjoint against its twin (test_gpu_parity._grad_case); a ceiling, not a fit
KINK = 1e-6  # cells: no seeded point closer than this to a node of the f1 lookup (|xi_e| on vx) or of the Z' table (xi_i)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _engine(cfg, sa, **kw):
    from tsadar_amd.engine import Engine

    return Engine(cfg, sa, **kw)


_REF = {}   # (nv, drift, feature) -> (engine, X, Pbar, twin result): the twin runs once per case


def _reference(torch, nv, drift, feature):
    """Device forward -> seed on the case's wavelength samples (zero elsewhere) -> the twin's gradients and absolute accumulations on
    the same points.  Asserts first, from the oracle's own intermediates, that no seeded point sits on a kink of the forward."""
    key = (nv, drift, feature)
    if key in _REF:
        return _REF[key]
    case = util.ff2d_twin_case(nv)
    ud, ud_ang, va_ang = case["drifts"][drift]
    _, X, lineouts = util.ff2d_with_drift(case, ud)
    beta, d_e, d_i = util.ff2d_kink_distances(case, feature, lineouts, ud_ang, va_ang)
    assert d_e.min() >= KINK, (nv, drift, feature, "|xi_e| on a vx node or outside the grid", d_e.min())
    assert d_i.min() >= KINK, (nv, drift, feature, "xi_i on a node of the Z' table", d_i.min())
    eng = _engine(case["cfg"], case["sa"])
    idx = np.array(case["lam"][feature])
    P0 = eng.form_factor_2d(feature, X, case["fe2"], ud_ang, va_ang)
    rng = np.random.default_rng(1000 * nv + 10 * drift + feature)
    seed = rng.standard_normal((case["B"], case["G"], idx.size, len(case["sa"]["sa"]))) / float(P0.abs().mean())
    Pbar = torch.zeros_like(P0)
    Pbar[:, :, torch.as_tensor(idx, device=P0.device), :] = torch.as_tensor(seed, device=P0.device)
    names = ot.phys_names_2d(case["n_ion"])
    g_phys, g_tab, A_phys, A_tab = ot.ff2d_adjoint(util.ff2d_lam_range(case, feature), 1024, 0.0, case["sa"]["sa"], case["G"], lineouts,
                                                   case["vx"], case["fe2"], ud_ang, va_ang, idx, seed, names)
    # the twin's columns -> the engine's slots; every other slot (amplitudes, A, m) carries nothing: A = 0 there
    gp, Ap = np.zeros((case["B"], eng.NP)), np.zeros((case["B"], eng.NP))
    for c, nm in enumerate(names):
        gp[:, util.slot_of(nm)], Ap[:, util.slot_of(nm)] = g_phys[:, c], A_phys[:, c]
    _REF[key] = dict(case=case, eng=eng, X=X, Pbar=Pbar, angles=(ud_ang, va_ang), beta=beta, gp=gp, Ap=Ap, gf=g_tab, Af=A_tab)
    return _REF[key]


def _check(ref, gp, gf, what):
    """|device - twin| <= TOL * A for every (lineout, slot) and every table entry; none left out.  (A = 0 makes the bound 0.)"""
    for name, dev, g, A in (("phys", gp, ref["gp"], ref["Ap"]), ("table", gf, ref["gf"], ref["Af"])):
        assert dev.shape == g.shape and np.all(np.isfinite(dev)), (what, name)
        err = np.abs(dev - g)
        ratio = err / np.where(A > 0, A, 1.0)
        print(f"{what} {name}: max |device - twin| / A = {ratio[A > 0].max():.3e}; entries with A = 0: {int((A == 0).sum())}, "
              f"max |device| there = {np.abs(dev[A == 0]).max() if (A == 0).any() else 0.0:.3e}")
        worst = np.unravel_index(np.argmax(err - TOL * A), err.shape)
        assert np.all(err <= TOL * A), (what, name, worst, dev[worst], g[worst], A[worst])


@pytest.mark.parametrize("nv", sorted(util.FF2D_TWIN_CASES))
def test_ff2d_adjoint_matches_twin(torch_mod, nv):
    """nv = 48: tables in LDS, two ions (fract / Z tying through Zbar), three gradient points, both features; 129: the table through
    L1/L2 with a single 128-cell tile; 132: all eight sampler forms (six angles, ion window around the laser line, four drift settings),
    2 x 2 tiles whose second tile is three cells wide; 133: an odd number of samples per line; 257: several columns per thread, the
    adjoint's second sampling sweep, no records, the seam at cell 128 of 256; 258: 3 x 3 tiles, the last one cell wide.
    nv <= 256: also from the projection records of a saving forward, against the twin and not against the resampling result."""
    case = util.FF2D_TWIN_CASES[nv]
    seen = set()
    for drift in range(len(case["drifts"])):
        for feature in sorted(case["lam"]):
            ref = _reference(torch_mod, nv, drift, feature)
            eng, X, fe2, Pbar, (ud_ang, va_ang) = ref["eng"], ref["X"], ref["case"]["fe2"], ref["Pbar"], ref["angles"]
            gp, gf = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang)
            _check(ref, gp.cpu().numpy(), gf.cpu().numpy(), f"nv={nv} drift={drift} feature={feature} resampled")
            if nv <= 256:
                eng.form_factor_2d(feature, X, fe2, ud_ang, va_ang, save=True)
                assert eng._saved_2d is not None and eng._saved_2d["token"] != 0
                gp, gf = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang, use_saved=True)
                _check(ref, gp.cpu().numpy(), gf.cpu().numpy(), f"nv={nv} drift={drift} feature={feature} saved")
            cb, sb = np.cos(ref["beta"]).ravel(), np.sin(ref["beta"]).ravel()
            seen |= set(zip((cb >= 0).tolist(), (sb >= 0).tolist(), (np.abs(sb) > np.abs(cb)).tolist()))
    if nv == 132:   # direction of the cell walk on each axis x orientation of the table copy, as test_rolling_sampler_every_walk_direction
        assert len(seen) == 8, sorted(seen)


def test_ff2d_adjoint_point_ranges_sum_to_twin(torch_mod):
    """Both adjoints are sums over points: the slices of the flat (lineout, gradient point, wavelength, angle) list, cut inside a
    lineout -- one of them three points long, inside a seeded wavelength sample -- add up to the twin's gradient within the same bound
    (worker count, points per tile and the partial-slot reduce at small point counts)."""
    nv, feature = 132, 1
    ref = _reference(torch_mod, nv, 0, feature)
    eng, X, fe2, Pbar, (ud_ang, va_ang) = ref["eng"], ref["X"], ref["case"]["fe2"], ref["Pbar"], ref["angles"]
    na, per_bg = Pbar.shape[3], Pbar.shape[2] * Pbar.shape[3]
    total = Pbar.shape[0] * Pbar.shape[1] * per_bg
    cuts = [234 * na + 2, 234 * na + 5, per_bg + 235 * na + 1]
    assert all(c % per_bg for c in cuts) and 234 in ref["case"]["lam"][feature] and 235 in ref["case"]["lam"][feature]
    gp, gf = 0.0, 0.0
    for lo, hi in zip([0] + cuts, cuts + [total]):
        a, b = eng.form_factor_2d_grad(feature, X, fe2, Pbar, ud_ang, va_ang, point_range=(lo, hi))
        gp, gf = gp + a.cpu().numpy(), gf + b.cpu().numpy()
    _check(ref, gp, gf, f"nv={nv} four point ranges")


@pytest.mark.parametrize("ccd,n_lam,start,end", [((1024, 1024), 1024, 90, 950), ((128, 256), 256, 10, 110)])
def test_ats_adjoint_matches_twin(torch_mod, ccd, n_lam, start, end):
    """Reverse of the ARTS instrument chain, the whole Pbar [G, npts, n_angles] and both amplitude adjoints against one backward of the
    twin, for the two geometries of test_ats_adjoint_directional_derivatives.  P is random, positive and smooth (no ties among the row
    maxima).  Each entry within 1e-7 of the largest |reference| at its own wavelength sample: the notch filter's band is smaller by
    10^-OD and may not hide behind the rest.  The amplitudes, plain sums, to 1e-9 relative."""
    cfg = decks.deck_angular(1, 64, ccd, start, end)
    sa = util._angular_sa(cfg)
    eng = _engine(cfg, sa, fe_mode=L.FE_PER_LINEOUT)
    wid = cfg["other"]["PhysParams"]["widIRF"]
    eng.ats_setup(sa["weights"], sa["angAxis"], wid["spect_FWHM_ele"] / 2.3548, wid["ang_FWHM_ele"] / 2.3548,
                  1024 // n_lam, 1024 // ccd[0], start, end)
    rows = end - start
    P = util.smooth_positive_image((1, 1024, sa["weights"].shape[1]), seed=3)
    rng = np.random.default_rng(11)
    e_amps = rng.uniform(0.5, 2.0, rows)
    Ebar = rng.normal(size=(rows, n_lam))
    p = dict(lam=526.5, amp1=0.8, amp2=1.3)
    Pbar, (a1b, a2b) = eng.ats_adjoint(P, e_amps, p["lam"], p["amp1"], p["amp2"], Ebar)
    Pbar = Pbar.cpu().numpy()
    lam_nm = np.linspace(*cfg["other"]["lamrangE"], 1024)
    Pref, a1r, a2r = ot.ats_adjoint(cfg, sa["weights"], sa["angAxis"], P, lam_nm, n_lam, e_amps[:, None], p, Ebar)
    assert Pbar.shape == Pref.shape and np.all(np.isfinite(Pbar))
    scale = np.max(np.abs(Pref), axis=(0, 2), keepdims=True)   # per wavelength sample
    assert scale.min() > 0
    print(f"ccd={ccd}: max |Pbar - twin| / max |twin| per wavelength = {np.max(np.abs(Pbar - Pref) / scale):.3e} "
          f"(scales {scale.min():.2e} .. {scale.max():.2e}); amp1 {abs(a1b - a1r) / abs(a1r):.2e}, amp2 {abs(a2b - a2r) / abs(a2r):.2e}")
    assert np.all(np.abs(Pbar - Pref) <= 1e-7 * scale)
    assert abs(a1b - a1r) <= 1e-9 * abs(a1r), (a1b, a1r)
    assert abs(a2b - a2r) <= 1e-9 * abs(a2r), (a2b, a2r)
