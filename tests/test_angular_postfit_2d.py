"""The post-fit half of angular (ARTS) decks with a 2-D f_e: Engine.form_factor_2d_jvp + Engine.ats_jvp against the shipped adjoint
(which tests/test_ff2d_adjoint_twin.py pins to the torch twin), LossFunction.angular_jacobian against central differences of the
device image, angular_gn_loss_wrt_params against the NumPy formulas on the returned J, and array_loss.

Two decks on the small geometry of tests/test_angular_postfit.py (CCD (128, 256), rows 10:110), nv = 32: the reference's arts2v kind
(``SphericalHarmonics``, Mora-Yahi, the generator fitted: leaves Te, ne, three generator values, lam, amp1, amp2) and a static
``Arbitrary2V`` table with the plasma scalars fitted (Te, ne, lam, amp1, amp2, ud, Va -- the drifts act through their angles)."""
import copy
import functools

import numpy as np
import pytest

import decks
import util
from tsadar_amd import _lib as L

pytestmark = pytest.mark.gpu

CCD, N_LAM, START, END = (128, 256), 256, 10, 110
ROWS = END - START
NV = 32
FD_TOL = 1e-4   # a difference quotient of the device's ARTS image against a derivative, of the image's largest entry: the bound and
                # the reason at the top of tests/test_angular_postfit.py
DOT_TOL = 1e-7  # of sum |Ebar . ThryE_dot|: the absolute-accumulation scale and the TOL of tests/test_ff2d_adjoint_twin.py


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _deck(kind):
    cfg = decks.deck_angular(2, NV, CCD, START, END)
    if kind == "mora-yahi":
        cfg["parameters"]["electron"]["fe"] = {"active": True, "dim": 2, "type": "sphericalharmonic", "nvx": NV,
                                               "params": {"flm_type": "mora-yahi", "init_m": 2.2, "Nl": 1, "nvr": NV, "LTx": 225000.0, "LTy": 400000.0}}
    else:   # a fixed Arbitrary2V table; the drifts fitted too
        cfg["parameters"]["electron"]["fe"]["active"] = False
        cfg["parameters"]["general"]["ud"].update(val=0.6, active=True)
        cfg["parameters"]["general"]["Va"].update(val=-0.9, active=True)
    return cfg


@functools.lru_cache(maxsize=None)
def _setup(kind):
    """-> (loss function, parameters, batch): the data are the device's own image at Te - 0.2, ne + 0.12 (normalised) plus the batch's
    noise.  One engine per deck, shared by the tests."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg = _deck(kind)
    sa = util._angular_sa(cfg)
    e_amps = np.random.default_rng(3).uniform(0.5, 2.0, (ROWS, 1))
    noise = 0.01 * np.abs(np.random.default_rng(4).standard_normal((ROWS, N_LAM)))
    batch = dict(e_data=np.ones((ROWS, N_LAM)), i_data=np.zeros((ROWS, N_LAM)), e_amps=e_amps, i_amps=np.zeros(ROWS), noise_e=noise,
                 noise_i=np.array([0.0]))
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    truth = tp.copy()
    truth.X[0, L.P_TE] -= 0.2
    truth.X[0, L.P_NE] += 0.12
    batch = dict(batch, e_data=lf.ts_diag(truth, batch)[0].copy())
    return lf, tp, batch


def _leaves(kind):
    if kind == "mora-yahi":
        return [("electron", "Te"), ("electron", "ne"), ("electron", "fe", 0), ("electron", "fe", 1), ("electron", "fe", 2), ("general", "lam"),
                ("general", "amp1"), ("general", "amp2")]
    return [("electron", "Te"), ("electron", "ne"), ("general", "lam"), ("general", "amp1"), ("general", "amp2"), ("general", "ud"), ("general", "Va")]


@pytest.mark.parametrize("kind", ["mora-yahi", "static"])
def test_dot_product_identity_against_the_adjoint(torch_mod, kind):
    """sum Ebar . ThryE_dot[k] (form_factor_2d_jvp + ats_jvp) = grad_phys . phys_dot[k] + <grad_fe2d, fe2d_dot[k]> + amp_bar . amp_dot[k]
    (ats_adjoint + form_factor_2d_grad) for a random image-space seed and the directions of the deck's fitted leaves."""
    lf, tp, batch = _setup(kind)
    eng = lf.ts_diag.engine(True)
    names, pd, fd, ad = lf._angular_directions(tp)
    assert names == _leaves(kind) and (fd is not None) == (kind == "mora-yahi")
    lf.ts_diag._ats_prepare(eng, batch)
    gen = lf.cfg["parameters"]["general"]
    ang = (gen["ud"]["angle"], gen["Va"]["angle"])
    assert ang == (20.0, -35.0)
    phys = tp.physical_matrix()
    p = phys[0]
    fe2 = np.ascontiguousarray(tp()["electron"]["fe"], dtype=np.float64)
    P, Pd = eng.form_factor_2d_jvp(0, phys, fe2, pd[:, None, :], fd, *ang, want_P=True)
    E, Ed = eng.ats_jvp(P[0], Pd[:, 0], batch["e_amps"], p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2], ad, want_E=True)
    rng = np.random.default_rng(21)
    Ebar = eng.dev(rng.standard_normal((ROWS, N_LAM)))
    Pbar, (a1b, a2b) = eng.ats_adjoint(P[0], batch["e_amps"], p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2], Ebar)
    gp, gf = eng.form_factor_2d_grad(0, phys, fe2, Pbar.reshape(P.shape), *ang, want_table=True)
    gp, gf = gp.cpu().numpy()[0], gf.cpu().numpy()
    for k, nm in enumerate(names):
        lhs = float((Ebar * Ed[k]).sum())
        rhs = float(np.dot(gp, pd[k])) + (float(np.sum(gf * fd[k])) if fd is not None else 0.0) + a1b * ad[k, 0] + a2b * ad[k, 1]
        scale = float((Ebar * Ed[k]).abs().sum())
        print(f"{kind} {nm}: |lhs - rhs| / sum |Ebar . E_dot| = {abs(lhs - rhs) / scale:.3e}")
        assert scale > 0 and abs(lhs - rhs) <= DOT_TOL * scale, (nm, lhs, rhs, scale)


def _perturbed(tp, leaf, step):
    from tsadar_amd import tree

    out = tp.copy()
    if len(leaf) == 3:
        theta = out.sph.get_params()
        theta[leaf[2]] += step
        out.sph.set_params(theta)
    else:
        slot = dict((n, s) for n, s in tree.get_filter_spec(None, tp))[leaf]
        out.X[0, slot] += step
    return out


@pytest.mark.parametrize("kind", ["mora-yahi", "static"])
def test_angular_jacobian_matches_image_differences(torch_mod, kind):
    """Each leaf's J against central differences of the device image (ts_diag, h = 1e-6 in normalised units) within FD_TOL of the
    image's largest entry; leaves in ravel order; ThryE is the image of the saving forward (the fit loop's) bit for bit, and the
    plain forward's to rounding (the saving and the plain sampler differ by 1e-13, tests/test_gpu_parity.py)."""
    lf, tp, batch = _setup(kind)
    out = lf.angular_jacobian(tp, batch, chunk=3)   # (three chunks)
    assert out["leaves"] == _leaves(kind) and out["ele"].shape == (len(out["leaves"]), ROWS, N_LAM)
    eng = lf.ts_diag.engine(True)
    launched = eng.last_launch()
    lf.ts_diag._angular(eng, tp, batch, to_host=False)
    assert np.array_equal(out["ThryE"], lf.ts_diag._angular_ctx["E_dev"].cpu().numpy())
    E0 = lf.ts_diag(tp, batch)[0] - batch["noise_e"]
    top = np.max(np.abs(E0))
    assert np.max(np.abs(out["ThryE"] - E0)) <= 1e-11 * top
    h = 1e-6
    for k, leaf in enumerate(out["leaves"]):
        quot = (lf.ts_diag(_perturbed(tp, leaf, h), batch)[0] - lf.ts_diag(_perturbed(tp, leaf, -h), batch)[0]) / (2 * h)
        err = np.max(np.abs(out["ele"][k] - quot)) / top
        print(f"{kind} {leaf}: max |J - quotient| / max |image| = {err:.3e}, max |J| / max |image| = {np.max(np.abs(out['ele'][k])) / top:.3e}")
        assert np.any(out["ele"][k]) and err <= FD_TOL, (leaf, err)
    one = lf.angular_jacobian(tp, batch, chunk=32)
    assert np.array_equal(one["ele"], out["ele"])   # (the chunking does not change a bit)


def _get_sigmas(hess, batch_size):
    """postprocess.get_sigmas' arithmetic (postprocess.py:205-242) for 1 x 1 blocks."""
    keys = [(sp, k) for sp in hess for k in hess[sp]]
    sig = np.zeros((batch_size, len(keys)))
    for i in range(batch_size):
        temp = np.array([[np.asarray(hess[s1][k1][s2][k2]).reshape(batch_size, batch_size)[i, i] for s2, k2 in keys] for s1, k1 in keys])
        inv = np.linalg.inv(temp)
        sig[i] = np.sign(np.diag(inv)) * np.sqrt(np.abs(np.diag(inv)))
    return sig


@pytest.mark.parametrize("kind", ["mora-yahi", "static"])
def test_angular_gauss_newton_on_2d_decks(torch_mod, kind):
    """H, grad and loss are the NumPy formulas applied to the returned J, to 1e-12 of each entry's absolute accumulation; H is
    symmetric; sigmas = sign sqrt|diag H^-1|; the nested ``hess`` exists exactly when every leaf is a scalar."""
    lf, tp, batch = _setup(kind)
    out = lf.angular_gn_loss_wrt_params(tp, batch)
    jac = lf.angular_jacobian(tp, batch)
    assert out["leaves"] == jac["leaves"] == _leaves(kind)
    J, Et = jac["ele"], jac["ThryE"]
    lam = lf.ts_diag._ats_lam_axis(lf.ts_diag.engine(True), 1024 // N_LAM)
    r = lf.cfg["data"]["fit_rng"]
    w = 0.5 * (((lam > r["blue_min"]) & (lam < r["blue_max"])).astype(float) + ((lam > r["red_min"]) & (lam < r["red_max"])))
    assert w.sum() > 0
    d = batch["e_data"]
    t = Et + batch["noise_e"]
    iu = 1.0 / (np.abs(d) + 1e-10)
    H = np.einsum("arc,rc,brc->ab", J, w[None, :] * 2.0 * iu, J)
    grad = np.einsum("arc,rc->a", J, w[None, :] * (-2.0 * (d - t) * iu))
    gacc = np.einsum("arc,rc->a", np.abs(J), w[None, :] * np.abs(2.0 * (d - t) * iu))
    loss = float(np.sum(w[None, :] * np.square(d - t) * iu))
    sc = np.sqrt(np.outer(np.diag(H), np.diag(H)))
    assert np.all(np.abs(out["H"] - H) <= 1e-12 * sc), np.max(np.abs(out["H"] - H) / sc)
    assert np.all(np.abs(out["grad"] - grad) <= 1e-12 * gacc), np.max(np.abs(out["grad"] - grad) / gacc)
    assert abs(out["loss"] - loss) <= 1e-12 * loss
    assert np.array_equal(out["H"], out["H"].T)
    inv = np.linalg.inv(out["H"])
    assert np.array_equal(out["sigmas"], np.sign(np.diag(inv)) * np.sqrt(np.abs(np.diag(inv))))
    assert np.all(np.isfinite(out["sigmas"])) and out["sigmas"].shape == (len(out["leaves"]),)
    if kind == "static":   # only scalar leaves: the nested layout get_sigmas(hess, 1) reads
        np.testing.assert_allclose(_get_sigmas(out["hess"], 1)[0], out["sigmas"], rtol=1e-12)
        assert out["hess"]["electron"]["Te"]["general"]["Va"].shape == (1, 1)
    else:
        assert "hess" not in out


def test_array_loss_on_a_2d_deck(torch_mod):
    """array_loss on the Mora-Yahi deck: post_loss (denominators = the theory image, nanmean over the blue and the red columns of a
    row, halved) written out on the device's image -- the call and the numbers of the 1-D angular decks."""
    lf, tp, batch = _setup("mora-yahi")
    total, sqdev, ThryE, ThryI, params = lf.array_loss(tp, batch)
    E, _, lam, _ = lf.ts_diag(tp, batch)
    assert np.array_equal(ThryE, E) and ThryE.shape == (ROWS, N_LAM)
    r = lf.cfg["data"]["fit_rng"]
    err = np.square(batch["e_data"] - E) / E
    blue = np.where((lam > r["blue_min"]) & (lam < r["blue_max"]), err, np.nan)
    red = np.where((lam > r["red_min"]) & (lam < r["red_max"]), err, np.nan)
    np.testing.assert_allclose(total, 0.5 * (np.nanmean(blue, axis=1) + np.nanmean(red, axis=1)), rtol=1e-14)
    np.testing.assert_allclose(sqdev["ele"], np.nan_to_num(blue) + np.nan_to_num(red), rtol=1e-14)
    assert total.shape == (ROWS,) and not np.any(sqdev["ion"]) and np.all(ThryI == 0.0) and "electron" in params
