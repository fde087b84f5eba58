"""tsff_loss_hess / Engine.loss_hess / LossFunction.h_loss_wrt_params(method="exact"): the exact per-lineout Hessian of the
reference's Hessian loss (_loss_for_hess_fn_, loss_function.py:170-188) against the double-backward Hessian of the torch twin.

The twin's own ``hessian_loss`` is l2 only; ``_twin_loss`` composes ``ot.ts_diag`` with torch forms of all four loss
functionals (the denominators of ``orc.loss_functional``: |data| + 1e-10 for l1 / l2, none for log-cosh / poisson), and a CPU
test pins that composition to central differences of the NumPy oracle first."""
import copy
import re
import subprocess

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L

HESS_TOL = 1e-7      # max |H_gpu - H_twin| <= HESS_TOL * max |H_twin|  (the bar of the gradient tests)
SIGMA_RTOL = 1e-6

# kernels of the exact-Hessian path and the GPU cases that launch each of them
HESS_KERNELS = {
    "k_hess_pairs<1>": "test_exact_hessian_matches_twin[sigmas]",
    "k_hess_pairs<2>": "test_exact_hessian_matches_twin[ions2]",
    "k_hess_pairs<3>": "test_exact_hessian_matches_twin[ions3_tied]",
    "k_hess_pairs<4>": "test_exact_hessian_matches_twin[ions4]",
    "k_hess_finish": "test_exact_hessian_matches_twin[sigmas]",
    "k_hess_mtab<1>": "test_exact_hessian_matches_twin[prod_nvx128]",
    "k_hess_mtab<2>": "test_exact_hessian_matches_twin[ions2_m]",
    "k_hess_mtab<3>": "test_exact_hessian_matches_twin[ions3_m]",
    "k_hess_mtab<4>": "test_exact_hessian_matches_twin[ions4_m]",
}


def _library_kernels(path):
    data = open(path, "rb").read()
    mangled = sorted({m.decode()[:-3] if m.endswith(b".kd") else m.decode() for m in re.findall(rb"_ZN4tsff\d+k_hess\w+", data)})
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^(void )?tsff::", "", s).split("(")[0] for s in out if s.strip()}


def test_every_hessian_kernel_has_a_case():
    from tsadar_amd import build

    path = build.build()
    have = _library_kernels(path)
    assert have, "no k_hess* kernel in libtsff.so"
    assert have == set(HESS_KERNELS), (sorted(have), sorted(HESS_KERNELS))
    ids = {c[0] for c in CASES}
    for k, case in HESS_KERNELS.items():
        assert case.split("[")[1].rstrip("]") in ids, (k, case)


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _twin_loss(cfg, sa, normed, batch, activate=True, fe_batch=None):
    """_loss_for_hess_fn_ for every loss_method: sum over the fitted samples, i_error + e_error (halved with both EPW ranges)."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    ThryE, ThryI, lamE, lamI = ot.ts_diag(cfg, sa, normed, batch, activate, fe_batch)
    ext = cfg["other"]["extraoptions"]
    method = cfg["optimizer"]["loss_method"]
    iaw, blue, red = orc.fit_masks(cfg, lamE.detach().numpy(), lamI.detach().numpy())

    def fun(d, t):
        d = ot._t(d)
        if method == "l1":
            return torch.abs(d - t) / (torch.abs(d) + 1e-10)
        if method == "l2":
            return torch.square(d - t) / (torch.abs(d) + 1e-10)
        if method == "log-cosh":
            return torch.log(torch.cosh(d - t))
        return t - d * torch.log(t)

    z = torch.zeros((), dtype=torch.float64)
    i_err = fun(batch["i_data"], ThryI)[torch.as_tensor(iaw)].sum() if ext["fit_IAW"] else z
    e_err = z
    if ext["fit_EPWb"]:
        e_err = e_err + fun(batch["e_data"], ThryE)[torch.as_tensor(blue)].sum()
    if ext["fit_EPWr"]:
        e_err = e_err + fun(batch["e_data"], ThryE)[torch.as_tensor(red)].sum()
        if ext["fit_EPWb"]:
            e_err = e_err * 0.5
    return i_err + e_err


def _twin_hessian(cfg, sa, normed_b, batch_b, names, activate=True, fe_batch=None):
    import torch
    from oracle import tsadar_oracle_torch as ot

    base = {k: ot._t(v).clone() for k, v in normed_b.items()}

    def f(vec):
        nm = dict(base)
        for i, k in enumerate(names):
            nm[k] = vec[i:i + 1]
        return _twin_loss(cfg, sa, nm, batch_b, activate, fe_batch)

    x0 = torch.cat([base[k].reshape(1) for k in names])
    return torch.autograd.functional.hessian(f, x0).numpy()


def _numpy_loss(cfg, normed_b, batch_b, activate=True):
    """The NumPy oracle's calc_ei_error with sum reduce and the denominators |data| + 1e-10 (loss_function.py:173-188)."""
    sa = util.sa_fit(1)
    ThryE, ThryI, lamE, lamI = orc.ts_diag(cfg, sa, normed_b, batch_b, activate)
    unc = (np.abs(np.asarray(batch_b["i_data"])) + 1e-10, np.abs(np.asarray(batch_b["e_data"])) + 1e-10)
    i_err, e_err, _ = orc.calc_ei_error(cfg, batch_b, ThryI, lamI, ThryE, lamE, unc, np.nansum)
    return i_err + e_err


@pytest.mark.parametrize("method", ["l1", "log-cosh", "poisson", "l2"])
def test_twin_loss_with_iaw_matches_numpy_oracle(method):
    """The IAW half of the yardstick: the value with every range fitted, against calc_ei_error."""
    import torch

    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "lam", "amp1"))
    cfg["optimizer"]["loss_method"] = method
    assert cfg["other"]["extraoptions"]["fit_IAW"]
    sa = util.sa_fit(1)
    batch = util.synthetic_batch(cfg, sa, 1, seed=13)
    normed = util.random_lineouts(cfg, 1, seed=14)
    nt = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)) for k, v in normed.items()}
    v0 = _numpy_loss(cfg, normed, batch)
    assert abs(float(_twin_loss(cfg, sa, nt, batch)) - v0) <= 1e-10 * abs(v0)
    off = copy.deepcopy(cfg)
    off["other"]["extraoptions"]["fit_IAW"] = False
    assert abs(v0 - _numpy_loss(off, normed, batch)) > 1e-3 * abs(v0)   # (the IAW term carries weight)


@pytest.mark.parametrize("method", ["l1", "log-cosh", "poisson", "l2"])
def test_twin_loss_matches_numpy_oracle(method):
    """The composed yardstick (value and gradient) against the NumPy oracle and its central differences, to 1e-5."""
    import torch

    cfg = decks.deck_fit(active=("Te", "ne", "lam", "amp1"))
    cfg["optimizer"]["loss_method"] = method
    cfg["other"]["extraoptions"]["fit_IAW"] = False   # (ion samples near 1e-7 make 1/|d| too stiff for a difference quotient)
    sa = util.sa_fit(1)
    batch = util.synthetic_batch(cfg, sa, 1, seed=11)
    normed = util.random_lineouts(cfg, 1, seed=12)
    names = ["Te", "ne", "lam", "amp1"]
    nt = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)).clone() for k, v in normed.items()}
    for k in names:
        nt[k].requires_grad_(True)
    val = _twin_loss(cfg, sa, nt, batch)
    g = torch.autograd.grad(val, [nt[k] for k in names])
    v0 = _numpy_loss(cfg, normed, batch)
    assert abs(float(val.detach()) - v0) <= 1e-10 * abs(v0)
    for k, gk in zip(names, g):
        def cd(h):
            p, m = copy.deepcopy(normed), copy.deepcopy(normed)
            p[k] = np.asarray(p[k], dtype=np.float64) + h
            m[k] = np.asarray(m[k], dtype=np.float64) - h
            return (_numpy_loss(cfg, p, batch) - _numpy_loss(cfg, m, batch)) / (2 * h)

        fd = cd(1e-7)   # (a small step keeps nearly every sample inside its Z' / W table cell: the slope convention)
        assert abs(float(gk) - fd) <= 1e-5 * max(abs(fd), 1e-3 * abs(v0)), (k, float(gk), fd)


# ---------------------------------------------------------------------------------------------------------------------
# GPU cases: (id, deck builder, leaves in ravel order)
# ---------------------------------------------------------------------------------------------------------------------
def _fit(**kw):
    return lambda: decks.deck_fit(**kw)


def _with(builder, fn):
    def b():
        cfg = builder()
        fn(cfg)
        return cfg
    return b


def _fract_active(cfg):
    for k, v in cfg["parameters"].items():
        if k.startswith("ion-"):
            v["fract"]["active"] = True
            v["Z"]["active"] = True


def _method(m):
    return lambda cfg: cfg["optimizer"].__setitem__("loss_method", m)


def _features(ele_b, ele_r, iaw):
    def f(cfg):
        ext = cfg["other"]["extraoptions"]
        ext["fit_EPWb"], ext["fit_EPWr"], ext["fit_IAW"] = ele_b, ele_r, iaw
    return f


def _grad3(cfg):
    g = cfg["parameters"]["general"]
    g["Te_gradient"]["num_grad_points"] = 3
    g["ne_gradient"]["num_grad_points"] = 3
    g["Te_gradient"]["active"] = True
    g["ne_gradient"]["active"] = True


def _no_ion_irf(cfg):
    cfg["other"]["PhysParams"]["widIRF"]["spect_stddev_ion"] = 0.0


def _iawfilter(cfg):
    cfg["other"]["iawfilter"] = [True, 1, 3, 526.5]


SIG = ("Te", "ne", "Ti", "lam", "amp1")
PROD = ("Te", "ne", "m", "amp1", "amp2", "lam")   # the reference's production leaves
CASES = [
    ("sigmas", _fit(active=SIG)),
    ("prod_nvx128", _fit(points_per_pixel=5, nvx=128, active=PROD)),
    ("prod_nvx320", _fit(points_per_pixel=5, nvx=320, active=PROD)),
    ("ions2", _with(_fit(n_ion=2, active=("Te", "ne", "Ti", "lam")), _fract_active)),
    ("ions3_tied", _with(_fit(n_ion=3, active=("Te", "ne", "Ti", "Z", "Ti_same_3")), _fract_active)),
    ("ions4", _with(_fit(n_ion=4, active=("Te", "ne", "Ti", "Z")), _fract_active)),
    ("grad3", _with(_fit(active=("Te", "ne", "lam")), _grad3)),
    ("ud_va", _fit(active=("Te", "ne", "ud", "Va", "amp1"))),
    ("l1", _with(_fit(active=SIG), _method("l1"))),
    ("logcosh", _with(_fit(active=SIG), _method("log-cosh"))),
    ("poisson", _with(_fit(active=SIG), _method("poisson"))),
    ("epw_only", _with(_fit(active=("Te", "ne", "lam", "amp1", "amp2")), _features(True, True, False))),
    ("iaw_only", _with(_fit(active=("Te", "ne", "Ti", "amp3")), _features(False, False, True))),
    ("blue_iaw", _with(_fit(active=SIG), _features(True, False, True))),
    ("no_ion_irf", _with(_fit(active=("Te", "ne", "Ti", "lam")), _no_ion_irf)),
    ("iawfilter", _with(_fit(active=SIG), _iawfilter)),
    ("ions2_m", _fit(n_ion=2, active=("Te", "ne", "m", "Ti", "lam"))),
    ("ions3_m", _with(_fit(n_ion=3, active=("Te", "ne", "m", "Ti", "Z")), _fract_active)),
    ("ions4_m", _fit(n_ion=4, active=("Te", "ne", "m", "Ti", "amp1"))),
]


def _leaves(cfg):
    """Trainable leaves in ravel order as (species, key), their oracle names and slots."""
    from tsadar_amd.params import SlotMap

    sm = SlotMap(cfg["parameters"], True)
    leaves = sm.active_leaves
    names = []
    for (sp, k), s in leaves:
        names.append(f"{k}_{int(sp.split('-')[1])}" if sp.startswith("ion-") else k)
    return leaves, names, [s for _, s in leaves]


def _weights(cfg):
    ext = cfg["other"]["extraoptions"]
    c = 0.5 if (ext["fit_EPWb"] and ext["fit_EPWr"]) else 1.0
    return np.array([1.0 if ext["fit_IAW"] else 0.0, c if ext["fit_EPWb"] else 0.0, c if ext["fit_EPWr"] else 0.0])


def _setup(cfg, B, seed):
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed)
    normed = util.random_lineouts(cfg, B, seed=seed + 50)
    return sa, batch, normed


def _sigmas(H):
    keep = np.any(H != 0.0, axis=1)   # (a tied leaf -- ion-3's Ti with Ti same -- has an all-zero row and no sigma)
    d = np.diag(np.linalg.inv(H[np.ix_(keep, keep)]))
    return np.sign(d) * np.sqrt(np.abs(d))


def _engine(cfg, sa):
    from tsadar_amd.engine import Engine

    return Engine(cfg, sa)


def _sync():
    import torch

    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,builder", CASES, ids=[c[0] for c in CASES])
def test_exact_hessian_matches_twin(cid, builder):
    cfg = builder()
    B = 2
    sa, batch, normed = _setup(cfg, B, seed=53)
    leaves, names, act = _leaves(cfg)
    n_ion = sum(1 for k in cfg["parameters"] if k.startswith("ion-"))
    eng = _engine(cfg, sa)
    X = util.normed_to_matrix(normed, n_ion)
    terms, grad, hess = eng.loss_hess(X, batch, _weights(cfg), act)
    _sync()
    launched = eng.last_launch()
    assert f"k_hess_pairs<{n_ion}>" in launched and "k_hess_finish" in launched, launched
    # only new kernels and shipped table / reduction kernels
    assert all(k.startswith(("k_hess_", "k_fe_", "k_wgemm", "k_loss_reduce")) for k in launched), launched
    assert (f"k_hess_mtab<{n_ion}>" in launched) == (L.P_M in act), launched
    H = hess.cpu().numpy()
    assert np.array_equal(H, np.transpose(H, (0, 2, 1)))
    for b in range(B):
        nb = {k: np.asarray(v)[b:b + 1] for k, v in normed.items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in batch.items()}
        Ho = _twin_hessian(cfg, util.sa_fit(1), nb, bb, names)
        err = np.max(np.abs(H[b] - Ho))
        assert err <= HESS_TOL * np.max(np.abs(Ho)), (cid, b, err / np.max(np.abs(Ho)), H[b], Ho)
        np.testing.assert_allclose(_sigmas(H[b]), _sigmas(Ho), rtol=SIGMA_RTOL)


def _sigma_deck():
    return decks.deck_fit(active=SIG)


@pytest.mark.gpu
def test_grad_and_terms_match_loss_grad_denominator_mode_2():
    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "Z", "lam", "amp1", "amp2", "amp3", "Va"))
    cfg["other"]["extraoptions"]["fit_IAW"] = False   # (the IAW case: test_grad_with_iaw_as_close_to_twin_as_loss_grad)
    B = 5
    sa, batch, normed = _setup(cfg, B, seed=71)
    _, _, act = _leaves(cfg)
    eng = _engine(cfg, sa)
    X = util.normed_to_matrix(normed, 1)
    w = _weights(cfg)
    terms, grad, _ = eng.loss_hess(X, batch, w, act)
    _sync()
    assert len(act) == 9
    n9 = eng.last_launch()
    gm = np.zeros(L.n_params(1), dtype=np.uint8)
    gm[act] = 1
    eng.set_denominator_mode(2)
    try:
        t2, g2 = eng.loss_grad(X, batch, w, gm)[:2]
        _sync()
    finally:
        eng.set_denominator_mode(0)
    t2, g2 = t2.cpu().numpy(), g2.cpu().numpy()[:, act]
    np.testing.assert_allclose(terms.cpu().numpy(), t2, rtol=1e-12, atol=0)
    assert np.max(np.abs(grad.cpu().numpy() - g2)) <= 1e-10 * np.max(np.abs(g2))
    # launch count: the same kernels for 3 and for 9 active leaves, only new kernels and shipped table / reduce kernels
    eng.loss_hess(X, batch, w, act[:3])
    _sync()
    n3 = eng.last_launch()
    assert n3 == n9, (n3, n9)
    for k in n9:
        assert k.startswith(("k_hess_", "k_fe_", "k_wgemm", "k_loss_reduce")), n9


@pytest.mark.gpu
def test_deterministic_and_independent_of_batch():
    cfg = _sigma_deck()
    B = 37
    sa, batch, normed = _setup(cfg, B, seed=81)
    _, _, act = _leaves(cfg)
    eng = _engine(cfg, sa)
    X = util.normed_to_matrix(normed, 1)
    w = _weights(cfg)
    a = [t.cpu().numpy() for t in eng.loss_hess(X, batch, w, act)]
    b = [t.cpu().numpy() for t in eng.loss_hess(X, batch, w, act)]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    k = 23
    one = {n: np.asarray(v)[k:k + 1] for n, v in batch.items()}
    eng1 = _engine(cfg, util.sa_fit(1))
    g1, h1 = [t.cpu().numpy() for t in eng1.loss_hess(X[k:k + 1], one, w, act)[1:]]
    assert np.array_equal(g1[0], a[1][k]) and np.array_equal(h1[0], a[2][k])


@pytest.mark.gpu
def test_exact_vs_central_across_batch_and_layout():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg = _sigma_deck()
    B = 37
    sa, batch, normed = _setup(cfg, B, seed=91)
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    tp.X[:] = util.normed_to_matrix(normed, 1)
    he = lf.h_loss_wrt_params(tp, batch, method="exact")
    hc = lf.h_loss_wrt_params(tp, batch)
    assert set(he) == set(hc)
    leaves, names, _ = _leaves(cfg)
    keys = [k for k, _ in leaves]
    for s1, k1 in keys:
        assert set(he[s1]) == set(hc[s1])
        for s2, k2 in keys:
            assert he[s1][k1][s2][k2].shape == (B, B)
    He = np.array([[[he[s1][k1][s2][k2][b, b] for (s2, k2) in keys] for (s1, k1) in keys] for b in range(B)])
    Hc = np.array([[[hc[s1][k1][s2][k2][b, b] for (s2, k2) in keys] for (s1, k1) in keys] for b in range(B)])
    # every lineout: an indexing error anywhere in the batch shows here.  Where central differences disagree at 2e-4 (their
    # step of 1e-7 can still cross a Z' / W table cell and pick up curvature the convention sets to zero), the twin decides.
    for b in range(B):
        if np.max(np.abs(He[b] - Hc[b])) <= 2e-4 * np.max(np.abs(Hc[b])):
            continue
        nb = {k: np.asarray(v)[b:b + 1] for k, v in normed.items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in batch.items()}
        Ho = _twin_hessian(cfg, util.sa_fit(1), nb, bb, names)
        assert np.max(np.abs(He[b] - Ho)) <= HESS_TOL * np.max(np.abs(Ho)), ("exact and central disagree and exact is off", b)
    for b in (0, 17, 36):
        nb = {k: np.asarray(v)[b:b + 1] for k, v in normed.items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in batch.items()}
        Ho = _twin_hessian(cfg, util.sa_fit(1), nb, bb, names)
        assert np.max(np.abs(He[b] - Ho)) <= HESS_TOL * np.max(np.abs(Ho)), b
    with pytest.raises(ValueError):
        lf.h_loss_wrt_params(tp, batch, method="forward")


@pytest.mark.gpu
def test_refusals():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg = _sigma_deck()
    B = 2
    sa, batch, normed = _setup(cfg, B, seed=5)
    eng = _engine(cfg, sa)
    X = util.normed_to_matrix(normed, 1)
    w = _weights(cfg)
    for slots, code in (([L.P_TE, L.P_TE], -1), ([L.P_TE, L.P_ION0 + L.ION_A], -3), ([L.P_TE, 99], -1), ([L.P_M], -2)):
        with pytest.raises(L.TsffError) as e:
            eng.loss_hess(X, batch, w, slots)
        assert f"error {code}:" in str(e.value), (slots, str(e.value))   # (-2: this deck's f_e is not a DLM)


def _case_vs_twin(cfg, B, seed, rows, engine_kw=None, activate=True, fe=None, tol=HESS_TOL, ranges=None):
    """Engine.loss_hess on B lineouts, the twin on the lineouts ``rows``.  ``ranges``: further leaves to draw per lineout
    (util.random_lineouts)."""
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed, activate=activate)
    normed = util.random_lineouts(cfg, B, seed=seed + 50, activate=activate, ranges=ranges)
    _, names, act = _leaves(cfg)
    n_ion = sum(1 for k in cfg["parameters"] if k.startswith("ion-"))
    eng = _engine_kw(cfg, sa, activate=activate, **(engine_kw or {}))
    X = util.normed_to_matrix(normed, n_ion)
    H = eng.loss_hess(X, batch, _weights(cfg), act, fe=fe)[2].cpu().numpy()
    for b in rows:
        nb = {k: np.asarray(v)[b:b + 1] for k, v in normed.items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in batch.items()}
        Ho = _twin_hessian(cfg, util.sa_fit(1), nb, bb, names, activate, None if fe is None else fe[b])
        err = np.max(np.abs(H[b] - Ho))
        assert err <= tol * np.max(np.abs(Ho)), (b, err / np.max(np.abs(Ho)))
        np.testing.assert_allclose(_sigmas(H[b]), _sigmas(Ho), rtol=SIGMA_RTOL)
    return eng


def _engine_kw(cfg, sa, **kw):
    from tsadar_amd.engine import Engine

    return Engine(cfg, sa, **kw)


@pytest.mark.gpu
def test_exact_hessian_without_activation():
    _case_vs_twin(decks.deck_fit(active=SIG), 2, 61, (0, 1), activate=False)


@pytest.mark.gpu
def test_exact_hessian_per_lineout_and_dlm_tables_scalar_leaves():
    """fe_mode PER_LINEOUT (explicit f_e per lineout, not trained) and DLM (per-lineout tables, m fixed) with scalar leaves."""
    import sys

    sys.path.insert(0, __file__.rsplit("/", 1)[0])
    from test_kernel_matrix import _free_form_fe

    cfg = decks.deck_fit(active=SIG)
    fe = _free_form_fe(2, cfg["parameters"]["electron"]["fe"]["nvx"], 7)
    _case_vs_twin(cfg, 2, 63, (0, 1), engine_kw=dict(fe_mode=L.FE_PER_LINEOUT), fe=fe)
    eng = _case_vs_twin(cfg, 2, 65, (0, 1), engine_kw=dict(fe_mode=L.FE_DLM))
    assert "k_hess_mtab" not in ";".join(eng.last_launch())


@pytest.mark.gpu
def test_exact_hessian_at_scale_configs2():
    """B = 4096 on the configs[2] deck: 8 seeded lineouts against the twin."""
    cfg = decks.deck_fit()
    rows = np.random.default_rng(4096).choice(4096, 8, replace=False)
    _case_vs_twin(cfg, 4096, 101, rows)


@pytest.mark.gpu
def test_refusals_angular_and_free_form():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg = decks.deck_fit(active=SIG)
    nvx = cfg["parameters"]["electron"]["fe"]["nvx"]
    cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": nvx, "params": {"init_m": 2.4}}
    B = 2
    sa, batch, normed = _setup(decks.deck_fit(active=SIG), B, seed=5)
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    assert tp.fval is not None and tp.slots.fval_active
    with pytest.raises(NotImplementedError, match="free-form"):
        lf.h_loss_wrt_params(tp, batch, method="exact")
    lfa = LossFunction(decks.deck_fit(active=SIG), sa, batch)
    lfa.angular = True   # (what LossFunction.__init__ sets for an angular_full deck)
    tpa = ThomsonParams(decks.deck_fit(active=SIG)["parameters"], B, batch=True, activate=True)
    with pytest.raises(NotImplementedError, match="angular"):
        lfa.h_loss_wrt_params(tpa, batch, method="exact")


@pytest.mark.gpu
def test_grad_with_iaw_as_close_to_twin_as_loss_grad():
    """With the IAW range fitted, samples of i_data near 1e-7 weight their terms by 1/|d| and the finite difference along
    lambda amplifies last-bit differences of the spectrum: the two device paths then differ from EACH OTHER at ~1e-10 (loss) /
    ~1e-9 (gradient) -- and each differs from the twin by the same order.  The exact path must be no farther from the twin than
    tsff_loss_grad itself."""
    import torch

    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "Z", "lam", "amp1", "amp2", "amp3", "Va"))
    sa, batch, normed = _setup(cfg, 1, seed=71)
    _, names, act = _leaves(cfg)
    eng = _engine(cfg, sa)
    X = util.normed_to_matrix(normed, 1)
    w = _weights(cfg)
    th, gh, _ = [t.cpu().numpy() for t in eng.loss_hess(X, batch, w, act)]
    gm = np.zeros(L.n_params(1), dtype=np.uint8)
    gm[act] = 1
    eng.set_denominator_mode(2)
    try:
        tg, gg = [t.cpu().numpy() for t in eng.loss_grad(X, batch, w, gm)[:2]]
    finally:
        eng.set_denominator_mode(0)
    nt = {k: torch.as_tensor(np.asarray(v, dtype=np.float64)).clone() for k, v in normed.items()}
    for k in names:
        nt[k].requires_grad_(True)
    val = _twin_loss(cfg, util.sa_fit(1), nt, batch)
    gt = np.array([float(g) for g in torch.autograd.grad(val, [nt[k] for k in names])])
    v = float(val.detach())
    assert abs(w @ th - v) <= max(2.0 * abs(w @ tg - v), 1e-12 * abs(v))
    assert np.max(np.abs(gh[0] - gt)) <= max(2.0 * np.max(np.abs(gg[0, act] - gt)), 1e-12 * np.max(np.abs(gt)))
    assert np.max(np.abs(gh[0] - gt)) <= 1e-8 * np.max(np.abs(gt))
