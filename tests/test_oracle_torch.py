"""The torch autograd twin of the oracle: same forward values as the NumPy oracle, gradients
consistent with finite differences.  CPU only."""
import copy

import numpy as np
import pytest
import torch

import decks
import util
from oracle import tsadar_oracle as orc
from oracle import tsadar_oracle_torch as ot


def _case(active, n_ion=1, B=2, seed=4, tweak=None):
    cfg = decks.deck_fit(active=active, n_ion=n_ion)
    if tweak:
        tweak(cfg)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed)
    normed = util.random_lineouts(cfg, B, seed=seed + 50)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    return cfg, sa, batch, normed, i_norm, e_norm


def test_twin_forward_equals_numpy_oracle():
    cfg, sa, batch, normed, i_norm, e_norm = _case(("Te", "ne", "Ti", "Va", "lam", "amp1"))
    lo, Eo, Io = orc.loss(cfg, sa, normed, batch, i_norm, e_norm)
    val, g, E, I = ot.value_and_grad(cfg, sa, normed, batch, i_norm, e_norm, ["Te"])
    assert abs(val - lo) < 1e-11 * abs(lo)
    assert util.rel_err(E, Eo) < 1e-9 and util.rel_err(I, Io) < 1e-9


def test_twin_gradient_vs_finite_differences():
    """Smooth leaves agree with central differences to ~1e-6; Te/lam move points across kinks of the
    piecewise-linear Z' table, where FD is only first-order accurate -> looser bound."""
    names = ["Te", "ne", "Ti_1", "lam", "amp1", "amp2", "amp3", "Va"]
    cfg, sa, batch, normed, i_norm, e_norm = _case(("Te", "ne", "Ti", "lam", "amp1", "amp2", "amp3", "Va"))
    val, g, _, _ = ot.value_and_grad(cfg, sa, normed, batch, i_norm, e_norm, names)
    fd = orc.fd_gradient(cfg, sa, normed, batch, i_norm, e_norm, names, h=1e-6)
    scale = max(np.max(np.abs(v)) for v in fd.values())
    for k in names:
        tol = 1e-4 if k in ("Te", "lam", "ne") else 2e-6
        assert np.max(np.abs(g[k] - fd[k])) / scale < tol, (k, g[k], fd[k])


def test_twin_dlm_order_gradient():
    """d loss / d m through f_e -> {ln f_e Hermite table, W table}: autodiff vs finite differences."""
    cfg, sa, batch, normed, i_norm, e_norm = _case(("Te", "ne", "m", "amp1", "amp2", "lam"), B=1, seed=6)
    normed["m"] = np.array([-0.3])  # m ~ 3.28, inside a table cell
    val, g, _, _ = ot.value_and_grad(cfg, sa, normed, batch, i_norm, e_norm, ["m", "Te"])
    fd = orc.fd_gradient(cfg, sa, normed, batch, i_norm, e_norm, ["m"], h=1e-5)
    assert abs(g["m"][0] - fd["m"][0]) < 1e-4 * max(abs(fd["m"][0]), abs(g["Te"][0]))


# ---- the 2-D form factor and the ARTS chain: the twin of tsadar_oracle's calc_in_2D / ats_spectrum restatements ----
def _ff2d_inputs(nv, feature, drift=0, seed=8):
    """One case of util.FF2D_TWIN_CASES on the CPU: the seed is random on the case's wavelength samples."""
    case = util.ff2d_twin_case(nv)
    ud, ud_ang, va_ang = case["drifts"][drift]
    _, _, lineouts = util.ff2d_with_drift(case, ud)
    idx = np.array(case["lam"][feature])
    sa = case["sa"]["sa"]
    Pbar = np.random.default_rng(seed).standard_normal((case["B"], case["G"], idx.size, sa.size))
    args = (util.ff2d_lam_range(case, feature), 1024, 0.0, sa, case["G"])
    return case, args, lineouts, (ud_ang, va_ang), idx, Pbar


@pytest.mark.parametrize("nv", [48, 133])
def test_twin_rotate_df_equals_numpy_oracle(nv):
    vx, fe2 = util.fe2d(nv)
    for angle in (0.0, 33.3, 90.0, 151.0, 262.5, -17.0):
        ro = orc.rotate_df(vx, fe2, angle)
        rt = ot.rotate_df(vx, ot._t(fe2), angle).numpy()
        assert np.max(np.abs(rt - ro)) <= 1e-12 * np.max(np.abs(ro)), (nv, angle)


@pytest.mark.parametrize("nv", [48, 133])
def test_twin_form_factor_2d_forward_equals_numpy_oracle(nv):
    """Every point of a lam_index subset, both features (nv = 48: two ions, three gradient points), 1e-12 relative per point."""
    for feature in (0, 1):
        case, args, lineouts, (ud_ang, va_ang), idx, _ = _ff2d_inputs(nv, feature)
        for p_np in lineouts:
            Po, lam_o = orc.form_factor_2d(*args, p_np, case["vx"], case["fe2"], ud_ang, va_ang, lam_index=idx)
            p, _ = ot._leaf_params(p_np, [])
            with torch.no_grad():
                Pt, lam_t = ot.form_factor_2d(*args, p, case["vx"], ot._t(case["fe2"]), ud_ang, va_ang, lam_index=idx)
            assert Pt.shape == Po.shape
            assert np.max(np.abs(Pt.numpy() - Po) / np.abs(Po)) < 1e-12, (nv, feature)
            assert np.max(np.abs(lam_t.numpy() - lam_o) / lam_o) < 1e-15


def _ats_inputs():
    """The small CCD geometry of test_ats_instrument_chain_matches_oracle with a smooth positive image."""
    ccd, n_lam, start, end = (128, 256), 256, 10, 110
    cfg = decks.deck_angular(1, 64, ccd, start, end)
    sa = util._angular_sa(cfg)
    P = util.smooth_positive_image((1, 1024, 241), seed=3)
    rng = np.random.default_rng(11)
    e_amps = rng.uniform(0.5, 2.0, (end - start, 1))
    Ebar = rng.normal(size=(end - start, n_lam))
    lam_nm = np.linspace(*cfg["other"]["lamrangE"], 1024)
    return (cfg, sa["weights"], sa["angAxis"]), P, (lam_nm, n_lam, e_amps), dict(lam=526.5, amp1=0.8, amp2=1.3), Ebar


def test_twin_ats_spectrum_forward_and_gradient():
    """ats_spectrum: the NumPy oracle's values to 1e-12 relative; its reverse mode against central differences of the NumPy
    oracle along a smooth direction of P (a rough one moves the arg-max of the flat row maxima inside the step) and in the
    two amplitudes."""
    head, P, tail, p, Ebar = _ats_inputs()
    Eo, lam_o = orc.ats_spectrum(*head, P, *tail, p)
    with torch.no_grad():
        Et, lam_t = ot.ats_spectrum(*head, ot._t(P), *tail, dict(lam=p["lam"], amp1=ot._t(p["amp1"]), amp2=ot._t(p["amp2"])))
    assert np.max(np.abs(Et.numpy() - Eo) / np.abs(Eo)) < 1e-12
    assert np.array_equal(lam_t.numpy(), lam_o)
    Pbar, a1b, a2b = ot.ats_adjoint(*head, P, *tail, p, Ebar)

    def J(Pm, q=p):
        return float(np.sum(Ebar * orc.ats_spectrum(*head, Pm, *tail, q)[0]))

    d, h = util.smooth_positive_image(P.shape, seed=9) - 1.5, 1e-5
    fd = (J(P + h * d) - J(P - h * d)) / (2 * h)
    assert abs(fd - float(np.sum(Pbar * d))) < 2e-6 * abs(fd)
    for nm, an in (("amp1", a1b), ("amp2", a2b)):
        fd = (J(P, dict(p, **{nm: p[nm] + h})) - J(P, dict(p, **{nm: p[nm] - h}))) / (2 * h)
        assert abs(fd - an) < 2e-6 * abs(fd), (nm, fd, an)


def test_twin_2d_gradient_vs_finite_differences():
    """ff2d_adjoint against central differences of the NumPy oracle's form_factor_2d: every physical parameter of both lineouts and a
    handful of table entries, nv = 48, two ions, three gradient points.  A sanity check of the twin at the bounds of
    test_twin_gradient_vs_finite_differences, taken against each entry's own absolute accumulation."""
    names = ot.phys_names_2d(2)
    for feature in (0, 1):
        case, args, lineouts, (ud_ang, va_ang), idx, Pbar = _ff2d_inputs(48, feature)
        vx, fe2 = case["vx"], case["fe2"]

        def J(los, fe):
            return sum(float(np.sum(Pbar[b] * orc.form_factor_2d(*args, los[b], vx, fe, ud_ang, va_ang, lam_index=idx)[0])) for b in range(len(los)))

        g_phys, g_tab, A_phys, A_tab = ot.ff2d_adjoint(*args, lineouts, vx, fe2, ud_ang, va_ang, idx, Pbar, names)
        for b in range(case["B"]):
            for c, nm in enumerate(names):
                key, s = (nm.rsplit("_", 1)[0], int(nm.rsplit("_", 1)[1]) - 1) if nm[-1].isdigit() else (nm, None)
                val = lineouts[b][key] if s is None else lineouts[b][key][s]
                h = (1e-9 if nm == "lam" else 1e-6) * max(abs(val), 1e-2)   # lam moves omega - omega_L a million times faster
                los = [copy.deepcopy(lineouts), copy.deepcopy(lineouts)]
                for lo, sgn in zip(los, (1.0, -1.0)):
                    if s is None:
                        lo[b][key] += sgn * h
                    else:
                        lo[b][key][s] += sgn * h
                fd = (J(los[0], fe2) - J(los[1], fe2)) / (2 * h)
                tol = 1e-4 if nm in ("Te", "lam", "ne") else 2e-6
                assert abs(g_phys[b, c] - fd) < tol * A_phys[b, c], (feature, b, nm, g_phys[b, c], fd)
        for (i, j) in [(0, 0), (24, 24), (27, 19), (10, 30), (40, 12)]:
            h = 1e-6 * fe2.max()
            fp, fm = fe2.copy(), fe2.copy()
            fp[i, j] += h
            fm[i, j] -= h
            fd = (J(lineouts, fp) - J(lineouts, fm)) / (2 * h)
            assert abs(g_tab[i, j] - fd) <= 2e-6 * A_tab[i, j], (feature, i, j, g_tab[i, j], fd)
        assert A_tab[0, 0] == 0.0 and g_tab[0, 0] == 0.0   # no seeded line reaches the corner


@pytest.mark.parametrize("nv,feature", [(48, 0), (48, 1), (129, 0), (132, 1)])
def test_twin_2d_adjoint_noise_floor(nv, feature):
    """How well does the twin know its own answer?  ff2d_adjoint on the problem and on its mirror image (transposed table rotated
    by the reflected angle, gradient transposed back): the same mathematics summed in another order.  The two must agree, for every
    table entry and every (lineout, parameter), within 1e-9 of that entry's absolute accumulation A -- a hundred times below the
    1e-7 the device adjoint is held to (tests/test_ff2d_adjoint_twin.py) -- and exactly where A is 0.

    Measured max |g1 - g2| / A, table / parameters: nv = 48 electron window 1.1e-12 / 5.2e-14, ion window 6.6e-13 / 7.4e-15;
    nv = 129 electron window 3.1e-10 / 1.1e-14; nv = 132 ion window 5.1e-12 / 6.0e-14.

    The electron window's samples include one beside the laser line on purpose: away from it every ion's xi_i is beyond the Z'
    table, chi_i = -(omega_pi / omega)^2 does not depend on T_i, and d P / d T_i is an exact cancellation whose rounding residue
    (1e-20) has no honest scale of its own."""
    case, args, lineouts, (ud_ang, va_ang), idx, Pbar = _ff2d_inputs(nv, feature)
    names = ot.phys_names_2d(case["n_ion"])
    a = ot.ff2d_adjoint(*args, lineouts, case["vx"], case["fe2"], ud_ang, va_ang, idx, Pbar, names)
    b = ot.ff2d_adjoint(*args, lineouts, case["vx"], case["fe2"], ud_ang, va_ang, idx, Pbar, names, mirrored=True)
    for g1, g2, A1, A2 in ((a[0], b[0], a[2], b[2]), (a[1], b[1], a[3], b[3])):
        assert np.all(np.isfinite(g1)) and np.all(np.isfinite(g2))
        assert np.array_equal(A1 == 0, A2 == 0)
        floor = np.abs(g1 - g2) / np.where(A1 > 0, A1, 1.0)
        print(nv, feature, g1.shape, "max |g1 - g2| / A =", floor.max())
        assert np.all(np.abs(g1 - g2) <= 1e-9 * A1), floor.max()
