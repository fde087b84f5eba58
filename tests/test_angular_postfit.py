"""The post-fit half of angular (ARTS) decks: LossFunction.angular_jacobian, angular_gn_loss_wrt_params and array_loss on an angular
deck, and distribution.arbitrary_1v_jvp.

The yardstick of the Jacobian is the torch twin as it stands (tests/angular_twin.py): the normalised leaves through
``ot.physical_params``, ``ot.dlm_fe`` (or the free-form generator written out in torch), ``ot.chi_table``, ``ot.form_factor`` and
``ot.ats_spectrum``, one ``torch.autograd.functional.jvp`` per leaf.  A CPU test pins the twin's jvp of the ARTS image to central
differences of the NumPy oracle.  Every (leaf, image row) of J lies within ROW_TOL of its own largest entry in the twin."""
import copy
import functools

import numpy as np
import pytest

import angular_twin as at
import decks
import util
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L
from test_form_factor_jvp import record

CCD, N_LAM, START, END = (128, 256), 256, 10, 110   # resolution units of 8 x 4, 100 image rows
ROWS = END - START
NVX = 64
SIGMA_RTOL = 1e-6   # the bound tests/test_jacobian.py holds the sigmas to
# A difference quotient of the oracle's ARTS image against a derivative, of the image's largest entry: the bound
# tests/test_gpu_parity.py::test_angular_vg_loss_finite_difference holds quotients of this very chain to (h = 1e-6).  It cannot be the
# 1e-5 of the 1-D spectra: P jumps where an ion's xi leaves the Z' table (the table's last value against the asymptote xi^-2), a
# quotient divides the jump of every sample that crosses inside the step by 2 h while the number of such samples shrinks with h, so
# that part of its error does not fall with the step; a derivative (the twin's, the device's) does not see the jumps.
FD_TOL = 1e-4


def _deck(free_form=False):
    cfg = decks.deck_angular(1, NVX, CCD, START, END)
    if free_form:
        cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": NVX, "params": {"init_m": 2.5}}
    return cfg


@functools.lru_cache(maxsize=None)
def _setup(free_form=False):
    """The small angular deck, its calibration, and a batch whose data are the oracle's image at Te - 0.2, ne + 0.12 (normalised)."""
    cfg = _deck(free_form)
    sa = util._angular_sa(cfg)
    dcfg = _deck(False)
    truth = orc.init_normed_params(dcfg["parameters"], 1, True)
    truth["Te"] = truth["Te"] - 0.2
    truth["ne"] = truth["ne"] + 0.12
    p = orc.lineout_params(orc.physical_params(dcfg["parameters"], truth, True), 0, 1)
    Po, lam_cm = orc.form_factor(dcfg["other"]["lamrangE"], 1024, 0.0, sa["sa"], 1, p, orc.velocity_grid(NVX), orc.dlm_fe(float(p["m"]), NVX))
    e_amps = np.random.default_rng(3).uniform(0.5, 2.0, (ROWS, 1))
    data, lam = orc.ats_spectrum(dcfg, sa["weights"], sa["angAxis"], Po, np.squeeze(lam_cm) * 1e7, N_LAM, e_amps, p)
    batch = dict(e_data=data, i_data=np.zeros((ROWS, N_LAM)), e_amps=e_amps, i_amps=np.zeros(ROWS),
                 noise_e=0.01 * np.abs(np.random.default_rng(4).standard_normal((ROWS, N_LAM))), noise_i=np.array([0.0]))
    return cfg, sa, batch, lam


def _loss_fn(free_form=False):
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg, sa, batch, _ = _setup(free_form)
    cfg = copy.deepcopy(cfg)
    return LossFunction(cfg, sa, batch), ThomsonParams(cfg["parameters"], 1, batch=False, activate=True), batch


def _torch_arbitrary_1v(fval):
    """Arbitrary1V.__call__ (base.py:201-204) in torch: the smoothing matrix is a constant of the generator."""
    import torch
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd import distribution as D

    u = ot._t(D.butterworth_matrix(NVX)) @ fval
    f = torch.pow(ot._t(10.0), -((7.0 * u) ** 2.0))
    return f / torch.sum(f) / (12.0 / NVX)


def _image_fn(free_form, tp):
    """-> (names, x0, F): F(x) = the twin's ARTS image [ROWS, N_LAM] (no noise) of the fitted normalised leaves x in ravel order."""
    import torch
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd import tree

    cfg, sa, batch, _ = _setup(free_form)
    spec = tree.get_filter_spec(None, tp)
    base = {k: ot._t(v) for k, v in orc.init_normed_params(cfg["parameters"], 1, True).items()}
    names, sizes, x0 = [], [], []
    for (sp, k), s in spec:
        names.append(k)
        if s == tree.FVAL_SLOT:
            sizes.append(NVX); x0.append(ot._t(tp.fval[0]))
        else:
            sizes.append(1); x0.append(ot._t(tp.X[:, s]))
    f = at.form_factor_fn(cfg, sa["sa"], 1, np.zeros(4), [cfg["parameters"]["ion-1"]["A"]["val"]], 0)
    vx = ot._t(orc.velocity_grid(NVX))
    other = cfg["other"]
    G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
    lam_nm = np.linspace(*other["lamrangE"], 1024)

    def F(x):
        nm, fval, o = dict(base), None, 0
        for k, n in zip(names, sizes):
            if k == "fval":
                fval = x[o:o + n]
            else:
                nm[k] = x[o:o + 1]
            o += n
        phys = ot.physical_params(cfg["parameters"], nm, True)
        p = {k: phys[k][0] for k in ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]}
        for k in ["Ti", "Z", "A", "fract"]:
            p[k] = [phys[f"{k}_1"][0]]
        fe = _torch_arbitrary_1v(fval) if free_form else ot.dlm_fe(phys["m"][0], NVX)
        P, _ = ot.form_factor(other["lamrangE"], other["npts"], cfg["data"]["ele_lam_shift"], sa["sa"], G, p, vx, fe, ot.chi_table(vx, fe))
        y, _ = ot.ats_spectrum(cfg, sa["weights"], sa["angAxis"], P, lam_nm, N_LAM, batch["e_amps"],
                               dict(lam=float(p["lam"].detach()), amp1=p["amp1"], amp2=p["amp2"]))
        return y

    return names, torch.cat(x0), F


@functools.lru_cache(maxsize=None)
def _twin_dlm():
    """The twin's image and its Jacobian w.r.t. {Te, ne, m, lam, amp1, amp2} (ravel order): computed once, shared, never modified."""
    import torch

    _, tp, _ = _loss_fn(False)
    names, x0, F = _image_fn(False, tp)
    E, rows = None, []
    for i in range(x0.numel()):
        v = torch.zeros_like(x0)
        v[i] = 1.0
        E, jv = torch.autograd.functional.jvp(F, x0, v)
        rows.append(jv.numpy())
    return names, E.numpy(), np.array(rows)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_twin_image_jvp_matches_oracle_differences():
    """The twin's jvp of the ARTS image along Te, ne, amp1 (physical units) and one smooth direction of f_e against central
    differences of the NumPy oracle; per image row the pair of steps (h, h/2) whose quotients agree best with each other is taken."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    cfg, sa, batch, _ = _setup(False)
    normed = orc.init_normed_params(cfg["parameters"], 1, True)
    x = util.normed_to_matrix(orc.physical_params(cfg["parameters"], normed, True), 1)[0]
    vx = orc.velocity_grid(NVX)
    fe = orc.dlm_fe(2.5, NVX)
    f = at.form_factor_fn(cfg, sa["sa"], 1, np.zeros(4), [x[L.P_ION0 + L.ION_A]], 0)
    g = at.ats_fn(cfg, sa, N_LAM, batch["e_amps"], x[L.P_LAM])
    image = lambda px, fet: g(f(px, fet), torch.stack([px[L.P_AMP1], px[L.P_AMP2]]))
    names = ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]

    def oracle(px, fev):
        p = {n: px[util.slot_of(n)] for n in names}
        p.update(Ti=[px[L.P_ION0 + L.ION_TI]], Z=[px[L.P_ION0 + L.ION_Z]], A=[px[L.P_ION0 + L.ION_A]], fract=[px[L.P_ION0 + L.ION_FRACT]])
        Po, lam_cm = orc.form_factor(cfg["other"]["lamrangE"], 1024, 0.0, sa["sa"], 1, p, vx, fev)
        return orc.ats_spectrum(cfg, sa["weights"], sa["angAxis"], Po, np.squeeze(lam_cm) * 1e7, N_LAM, batch["e_amps"], p)[0]

    dirs = []
    for nm in ("Te", "ne", "amp1"):
        d = np.zeros_like(x)
        d[util.slot_of(nm)] = 1.0
        dirs.append((nm, d, np.zeros(NVX)))
    dirs.append(("fe", np.zeros_like(x), fe * (0.4 * np.cos(0.9 * vx + 0.3) + 0.2 * np.sin(1.7 * vx))))
    for nm, dx, dfe in dirs:
        _, jv = torch.autograd.functional.jvp(image, (ot._t(x), ot._t(fe)), (ot._t(dx), ot._t(dfe)))
        jv = jv.numpy()
        quot = [(oracle(x + h * dx, fe + h * dfe) - oracle(x - h * dx, fe - h * dfe)) / (2 * h) for h in (2e-6, 1e-6, 5e-7)]
        gap = [np.max(np.abs(a - b), axis=1) for a, b in zip(quot[:-1], quot[1:])]
        pick = np.where((gap[1] < gap[0])[:, None], quot[2], quot[1])
        # On the scale of the image's largest entry, not of each row's: what a quotient of this image is off by is absolute -- the
        # samples of P that cross a cell boundary of the piecewise-linear tables inside the step, and the rounding of the image over
        # 2 h -- and the two convolutions spread it over the rows whatever a row's own derivative is (the rows' largest entries span
        # two decades here).
        ratio = np.max(np.abs(pick - jv), axis=1) / np.max(np.abs(jv))
        print(f"twin image jvp vs oracle quotient, {nm}: {np.max(ratio):.2e} of the maximum")
        assert np.max(ratio) < FD_TOL, (nm, np.max(ratio))


def test_arbitrary_1v_jvp():
    from tsadar_amd import distribution as D

    rng = np.random.default_rng(2)
    fval = D.arbitrary_1v_init(2.7, NVX) * (1.0 + 0.02 * rng.standard_normal(NVX))
    J = D.arbitrary_1v_jvp(fval)
    assert J.shape == (NVX, NVX)
    h = 1e-6
    for j in (0, 5, NVX // 2, NVX - 1):
        e = np.zeros(NVX)
        e[j] = h
        fd = (D.arbitrary_1v(fval + e) - D.arbitrary_1v(fval - e)) / (2 * h)
        assert np.max(np.abs(fd - J[j])) <= 1e-8 * np.max(np.abs(J[j])) + 1e-9 * np.max(np.abs(J)), j
    d = rng.standard_normal((3, NVX))
    np.testing.assert_allclose(D.arbitrary_1v_jvp(fval, d), d @ J, rtol=1e-12, atol=1e-14 * np.max(np.abs(J)))
    # the rows of the adjoint: arbitrary_1v_vjp(fval, g) = J g
    for i in (0, 17, NVX - 1):
        gfe = np.zeros(NVX)
        gfe[i] = 1.0
        np.testing.assert_allclose(D.arbitrary_1v_vjp(fval, gfe), J[:, i], rtol=1e-11, atol=1e-13 * np.max(np.abs(J)))


def test_refusals_fire_before_an_engine_exists():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    def check(lf, tp, batch, calls=("angular_jacobian", "angular_gn_loss_wrt_params")):
        before = copy.deepcopy(lf.cfg)
        for name in calls:
            with pytest.raises(NotImplementedError):
                getattr(lf, name)(tp, batch)
        assert lf.ts_diag._engines == {} and lf.cfg == before

    lf, tp, batch = _loss_fn(False)
    # the 1-D calls keep refusing angular decks by name
    for call in (lambda: lf.jacobian(tp, batch), lambda: lf.gn_loss_wrt_params(tp, batch),
                 lambda: lf.h_loss_wrt_params(tp, batch, method="exact")):
        with pytest.raises(NotImplementedError, match="angular"):
            call()
    assert lf.ts_diag._engines == {}
    lf.distributed = True
    check(lf, tp, batch)
    lf.distributed = False
    lf.multiplex_ang = True
    check(lf, tp, batch)
    lf.multiplex_ang = False
    lf.cfg["optimizer"]["loss_method"] = "l1"
    check(lf, tp, batch, ("angular_gn_loss_wrt_params",))
    # a 2-D f_e deck
    cfg2 = decks.deck_angular(2, 32, CCD, START, END)
    sa = _setup(False)[1]
    lf2 = LossFunction(cfg2, sa, batch)
    check(lf2, ThomsonParams(cfg2["parameters"], 1, batch=False, activate=True), batch)
    # a 1-D deck
    cfg1 = decks.deck_fit()
    b1 = util.synthetic_batch(cfg1, util.sa_fit(2), 2, seed=1)
    check(LossFunction(cfg1, util.sa_fit(2), b1), ThomsonParams(cfg1["parameters"], 2, batch=True, activate=True), b1)


def _post_loss_formula(cfg, E, lamE, d):
    """calc_ei_error with denom = [ThryI, ThryE] and reduce nanmean(axis=1), the electron feature, written out (l2)."""
    r = cfg["data"]["fit_rng"]
    err = np.square(d - E) / E
    blue = np.where((lamE > r["blue_min"]) & (lamE < r["blue_max"]), err, np.nan)
    red = np.where((lamE > r["red_min"]) & (lamE < r["red_max"]), err, np.nan)
    return 0.5 * (np.nanmean(blue, axis=1) + np.nanmean(red, axis=1)), np.nan_to_num(blue) + np.nan_to_num(red)


def test_array_loss_host_formula():
    """array_loss on an angular deck with a NumPy image in place of the device's."""
    lf, tp, batch = _loss_fn(False)
    _, _, _, lam = _setup(False)
    rng = np.random.default_rng(8)
    E = batch["e_data"] * (1.0 + 0.05 * rng.standard_normal(batch["e_data"].shape))

    class Mock:
        _engines = {}

        def __call__(self, weights, b):
            return E, 0 + np.asarray(b["noise_i"]), lam, []

    lf.ts_diag = Mock()
    total, sqdev, ThryE, ThryI, params = lf.array_loss(tp, batch)
    want, sq = _post_loss_formula(lf.cfg, E, lam, batch["e_data"])
    assert total.shape == (ROWS,)
    np.testing.assert_allclose(total, want, rtol=1e-14)
    np.testing.assert_allclose(sqdev["ele"], sq, rtol=1e-14)
    assert sqdev["ion"].shape == batch["i_data"].shape and not np.any(sqdev["ion"])
    assert ThryE is E and np.all(ThryI == 0.0) and "electron" in params
    assert Mock._engines == {}


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.mark.gpu
def test_angular_jacobian_matches_twin(torch_mod):
    lf, tp, batch = _loss_fn(False)
    names, Et, Jt = _twin_dlm()
    out = lf.angular_jacobian(tp, batch, chunk=4)   # (two chunks: 4 + 2 directions)
    assert [k for _, k in out["leaves"]] == names == ["Te", "ne", "m", "lam", "amp1", "amp2"]
    assert out["ele"].shape == (6, ROWS, N_LAM)
    assert np.max(np.abs(out["ThryE"] - Et)) <= 1e-7 * np.max(np.abs(Et))
    ratio = at.row_ratios(out["ele"], Jt)
    record("angular_jacobian[dlm]", f"max row ratio {np.max(ratio):.3e} (bound {at.ROW_TOL:.0e}), per leaf " +
           " ".join(f"{n} {r:.1e}" for n, r in zip(names, np.max(ratio, axis=1))))
    assert np.max(ratio) <= at.ROW_TOL, np.max(ratio, axis=1)
    one = lf.angular_jacobian(tp, batch, chunk=32)
    assert np.array_equal(one["ele"], out["ele"])   # (the chunking does not change a bit)


@pytest.mark.gpu
def test_angular_jacobian_free_form(torch_mod):
    """``fe: {type: arbitrary, dim: 1, active: true}`` at nvx 64: six fval columns (first, last, the two next to the peak of f_e, two
    drawn), one random combination of all 64, and J^T Ebar against the gradient vg_loss returns for the same seed."""
    import torch
    from tsadar_amd import tree

    lf, tp, batch = _loss_fn(True)
    names, x0, F = _image_fn(True, tp)
    out = lf.angular_jacobian(tp, batch, chunk=32)
    J = out["ele"]
    k0 = names.index("fval")
    assert J.shape[0] == x0.numel() == len(names) - 1 + NVX and out["leaves"][k0] == ("electron", "fval", 0)
    peak = int(np.argmax(tp.fe_table()[0]))
    rng = np.random.default_rng(12)
    cols = [0, NVX - 1, peak - 1, peak + 1] + [int(c) for c in rng.choice(np.arange(2, NVX - 2), 2, replace=False)]
    worst = 0.0
    for c in cols:
        v = torch.zeros_like(x0)
        v[k0 + c] = 1.0
        _, jv = torch.autograd.functional.jvp(F, x0, v)
        worst = max(worst, float(np.max(at.row_ratios(J[k0 + c], jv.numpy()))))
    comb = rng.standard_normal(NVX)
    v = torch.zeros_like(x0)
    v[k0:k0 + NVX] = torch.as_tensor(comb)
    _, jv = torch.autograd.functional.jvp(F, x0, v)
    worst = max(worst, float(np.max(at.row_ratios(np.tensordot(comb, J[k0:k0 + NVX], axes=1), jv.numpy()))))
    record("angular_jacobian[free_form]", f"max row ratio {worst:.3e} (bound {at.ROW_TOL:.0e})")
    assert worst <= at.ROW_TOL, worst
    # the gradient of the fit loss: both sides chain the same seed Ebar = d loss / d ThryE, so they differ by the rounding of a sum of
    # |Ebar . J| worth of terms, held to 1e-7 of it (the bound of the dot-product identities of the device calls)
    diff, static = tree.partition(tp, tree.get_filter_spec(None, tp))
    x, lf.unravel_weights = tree.ravel_pytree(diff)   # (the deck's optimiser is l-bfgs-b: flat leaves in, flat gradient out)
    value, grad = lf.vg_loss(x, static, batch)
    eng = lf.ts_diag.engine(True)
    Ebar = lf._angular_value_device(eng, tp, batch, False)[2].cpu().numpy()
    g = np.tensordot(J, Ebar, axes=([1, 2], [0, 1]))
    bound = 1e-7 * np.tensordot(np.abs(J), np.abs(Ebar), axes=([1, 2], [0, 1]))
    assert grad.shape == g.shape and np.all(np.abs(g - grad) <= bound), np.max(np.abs(g - grad) / bound)


L1_OFFSET = 1.0   # the background tests/test_angular_loop_device.py puts under the data for l1: every |d - E| stays off zero


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["l2", "l1", "log-cosh", "poisson"])
def test_angular_vg_loss_dlm_matches_twin(torch_mod, method):
    """vg_loss on the DLM deck (leaves Te, ne, m, lam, amp1, amp2) for every loss functional, in three steps.  Value: the reference's
    functional (orc.loss_functional, the blue / red masks on the resolution-unit axis, the mean of each over the image, halved:
    _angular_wcol) evaluated on the host at the device's image, rtol 1e-12.  Seed: _angular_value_device's Ebar against torch
    autograd of that functional at the device's image, 1e-12 of the seed's largest entry.  Gradient: per leaf within 1e-7 of its own
    absolute accumulation sum |Jt| |Ebar| of the twin's image Jacobian (_twin_dlm) -- the bound of the free-form check above.
    The test of tests/test_gpu_parity.py holds this gradient to difference quotients at 1e-4."""
    import torch
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd import ThomsonParams, tree
    from tsadar_amd.loss_function import LossFunction

    cfg, sa, batch, lam = _setup(False)
    cfg = copy.deepcopy(cfg)
    cfg["optimizer"]["loss_method"] = method
    batch = dict(batch)
    if method == "l1":
        batch["e_data"] = batch["e_data"] + L1_OFFSET
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    names, _, Jt = _twin_dlm()
    diff, static = tree.partition(tp, tree.get_filter_spec(None, tp))
    assert [k for (_, k), _ in diff.slots] == names == ["Te", "ne", "m", "lam", "amp1", "amp2"]   # (Jt's ravel order)
    x, lf.unravel_weights = tree.ravel_pytree(diff)
    value, grad = lf.vg_loss(x, static, batch)
    eng = lf.ts_diag.engine(True)
    val_dev, E, Ebar = lf._angular_value_device(eng, tp, batch, True)
    Ebar = Ebar.cpu().numpy()
    assert val_dev == value
    d, un, r = batch["e_data"], lf.e_norm**2, cfg["data"]["fit_rng"]
    blue, red = (lam > r["blue_min"]) & (lam < r["blue_max"]), (lam > r["red_min"]) & (lam < r["red_max"])
    assert blue.any() and red.any() and E.shape == (ROWS, N_LAM)
    if method == "l1":
        assert np.min(np.abs(d - E)[:, blue | red]) > 1e-6 * np.max(E)
    err = orc.loss_functional(d, E, un, method)
    ref = 0.5 * (np.mean(err[:, blue]) + np.mean(err[:, red]))
    assert abs(value - ref) <= 1e-12 * abs(ref), (method, value, ref)
    # the seed: autograd of the same functional (the twin's, oracle/tsadar_oracle_torch.py: _sums_of_spectra.fun) at the device's image
    Et, dt = ot._t(E).clone().requires_grad_(True), ot._t(d)
    ft = {"l1": lambda: torch.abs(dt - Et) / un, "l2": lambda: torch.square(dt - Et) / un,
          "log-cosh": lambda: torch.log(torch.cosh(dt - Et)), "poisson": lambda: Et - dt * torch.log(Et)}[method]()
    tb, tr = torch.as_tensor(blue), torch.as_tensor(red)
    val_t = 0.5 * (ft[:, tb].mean() + ft[:, tr].mean())
    seed, = torch.autograd.grad(val_t, Et)
    seed = seed.numpy()
    assert abs(float(val_t) - ref) <= 1e-12 * abs(ref)
    assert np.max(np.abs(Ebar - seed)) <= 1e-12 * np.max(np.abs(seed)), (method, np.max(np.abs(Ebar - seed)) / np.max(np.abs(seed)))
    # the gradient, each leaf on its own scale
    g = np.tensordot(Jt, Ebar, axes=([1, 2], [0, 1]))
    A = np.tensordot(np.abs(Jt), np.abs(Ebar), axes=([1, 2], [0, 1]))
    ratio = np.abs(grad - g) / A
    record(f"angular_vg_loss[dlm-{method}]", f"max |grad - Jt.Ebar| / sum |Jt||Ebar| {np.max(ratio):.3e} (bound 1e-07), per leaf " +
           " ".join(f"{n} {v:.1e}" for n, v in zip(names, ratio)))
    print(method, "per leaf |grad - Jt.Ebar| / sum |Jt||Ebar|:", dict(zip(names, ratio)), "|g| / A:", dict(zip(names, np.abs(g) / A)))
    assert grad.shape == g.shape and np.all(np.abs(grad - g) <= 1e-7 * A), (method, dict(zip(names, ratio)))


def _get_sigmas(hess, batch_size):
    """postprocess.get_sigmas' arithmetic (postprocess.py:205-242) for 1 x 1 blocks."""
    keys = [(sp, k) for sp in hess for k in hess[sp]]
    sig = np.zeros((batch_size, len(keys)))
    for i in range(batch_size):
        temp = np.array([[np.asarray(hess[s1][k1][s2][k2]).reshape(batch_size, batch_size)[i, i] for s2, k2 in keys] for s1, k1 in keys])
        inv = np.linalg.inv(temp)
        sig[i] = np.sign(np.diag(inv)) * np.sqrt(np.abs(np.diag(inv)))
    return sig


@pytest.mark.gpu
def test_angular_gauss_newton_matches_twin(torch_mod):
    lf, tp, batch = _loss_fn(False)
    names, Et, Jt = _twin_dlm()
    cfg, _, _, lam = _setup(False)
    r = cfg["data"]["fit_rng"]
    w = 0.5 * (((lam > r["blue_min"]) & (lam < r["blue_max"])).astype(float) + ((lam > r["red_min"]) & (lam < r["red_max"])))
    d = batch["e_data"]
    t = Et + batch["noise_e"]
    iu = 1.0 / (np.abs(d) + 1e-10)
    H = np.einsum("arc,rc,brc->ab", Jt, w[None, :] * 2.0 * iu, Jt)
    grad = np.einsum("arc,rc->a", Jt, w[None, :] * (-2.0 * (d - t) * iu))
    loss = float(np.sum(w[None, :] * np.square(d - t) * iu))
    out = lf.angular_gn_loss_wrt_params(tp, batch)
    assert [k for _, k in out["leaves"]] == names
    sc = np.sqrt(np.outer(np.diag(H), np.diag(H)))
    assert np.all(np.abs(out["H"] - H) <= 1e-7 * sc), np.max(np.abs(out["H"] - H) / sc)
    assert np.all(np.abs(out["grad"] - grad) <= 1e-7 * np.sqrt(np.diag(H)) * np.sqrt(2.0 * loss) + 1e-7 * np.abs(grad))
    assert abs(out["loss"] - loss) <= 1e-7 * loss
    inv = np.linalg.inv(H)
    sig = np.sign(np.diag(inv)) * np.sqrt(np.abs(np.diag(inv)))
    np.testing.assert_allclose(out["sigmas"], sig, rtol=SIGMA_RTOL)
    np.testing.assert_allclose(_get_sigmas(out["hess"], 1)[0], out["sigmas"], rtol=1e-12)
    assert out["hess"]["electron"]["Te"]["general"]["lam"].shape == (1, 1)


@pytest.mark.gpu
def test_array_loss_angular_and_1d_unchanged(torch_mod):
    lf, tp, batch = _loss_fn(False)
    cfg, sa, _, lam = _setup(False)
    total, sqdev, ThryE, ThryI, params = lf.array_loss(tp, batch)
    p = orc.lineout_params(orc.physical_params(cfg["parameters"], orc.init_normed_params(cfg["parameters"], 1, True), True), 0, 1)
    Po, lam_cm = orc.form_factor(cfg["other"]["lamrangE"], 1024, 0.0, sa["sa"], 1, p, orc.velocity_grid(NVX), orc.dlm_fe(float(p["m"]), NVX))
    Eo = orc.ats_spectrum(cfg, sa["weights"], sa["angAxis"], Po, np.squeeze(lam_cm) * 1e7, N_LAM, batch["e_amps"], p)[0] + batch["noise_e"]
    want, sq = _post_loss_formula(cfg, Eo, lam, batch["e_data"])
    np.testing.assert_allclose(total, want, rtol=1e-7)
    np.testing.assert_allclose(sqdev["ele"], sq, rtol=1e-6, atol=1e-12 * np.max(sq))
    np.testing.assert_allclose(ThryE, Eo, rtol=1e-7)
    assert not np.any(sqdev["ion"]) and np.all(ThryI == 0.0)
    # a 1-D deck takes the path it took: the batch kernel's sums through the same host arithmetic, bit for bit
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg1 = decks.deck_fit()
    sa1 = util.sa_fit(2)
    b1 = util.synthetic_batch(cfg1, sa1, 2, seed=1)
    lf1 = LossFunction(cfg1, sa1, b1)
    tp1 = ThomsonParams(cfg1["parameters"], 2, batch=True, activate=True)
    t1, sq1, E1, I1, _ = lf1.array_loss(tp1, b1)
    eng = lf1.ts_diag.engine(True)
    sums, sqe, sqi, E, I = eng.array_loss(tp1.to_matrix(), lf1._device_batch(eng, b1, 2))
    s = sums.cpu().numpy()
    ref = cfg1["data"]["ion_loss_scale"] * (s[:, 0] / eng.n_iaw) + (s[:, 1] / eng.n_blue + s[:, 2] / eng.n_red) * 0.5
    assert np.array_equal(t1, ref) and np.array_equal(sq1["ele"], sqe.cpu().numpy()) and np.array_equal(E1, E.cpu().numpy())
