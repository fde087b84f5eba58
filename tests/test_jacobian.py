"""tsff_spectrum_jacobian / tsff_loss_gauss_newton (Engine.spectrum_jacobian, Engine.loss_gauss_newton, LossFunction.jacobian,
LossFunction.gn_loss_wrt_params): the Jacobian of the model spectra w.r.t. the fitted leaves and the Gauss-Newton curvature of
the Hessian loss, against the torch twin.

The yardstick is J from ``ot.ts_diag``: per lineout one ``torch.autograd.functional.jvp`` per active leaf.  CPU tests pin that
yardstick to central differences of the NumPy oracle and the definition of ``gn`` to the twin's double-backward Hessian at zero
residual, before the device is compared with either."""
import copy
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L

ROW_TOL = 1e-7       # max_j |J_gpu - J_twin| <= ROW_TOL * max_j |J_twin[b, a, :]|: the gradient bar of the suite, each row on its own scale
FD_TOL = 1e-5        # a difference quotient against a derivative: the north-star tolerance, per row
GN_TOL = 1e-7        # gn, grad, loss_terms: of the largest entry per lineout
SIGMA_RTOL = 1e-6
JAC_WIDTH = 3        # tangents per group of k_jac_sweep<NI, 3, .> (the GPU cases read the width off the launched kernel's name)
B = 3                # odd and > 1: lineout strides show

# Steps of the difference quotients, each half the one before.  No single step serves every row: the ion rows need a large one (the
# spectrum near the ion-acoustic resonance carries rounding noise of ~1e-11, which a quotient divides by 2 h), the rows of the
# electron feature and of lam a small one (a step that crosses a kink -- a cell boundary of the piecewise-linear tables under the
# peak sample, a change of the arg-max bin -- picks up the jump in slope).  Per row the pair (h, h/2) whose two quotients agree
# best WITH EACH OTHER is taken -- a choice made without looking at the Jacobian under test -- and then held to FD_TOL.
FD_LADDER = tuple(1.28e-4 / 2 ** k for k in range(11))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "jacobian_pytest.txt")

# every shipped k_jac_* instantiation and the GPU case that launches it
JAC_KERNELS = {
    # the row form (1-2 ion species, one gradient point, no DLM order among the leaves, no raw feature): k_jac_sweep<NI, 3, true>
    "k_jac_sweep<1, 3, true>": "test_jacobian_matches_twin[ions1]",
    "k_jac_sweep<2, 3, true>": "test_jacobian_matches_twin[ions2]",
    # the tangent form: everything else
    "k_jac_sweep<1, 3, false>": "test_jacobian_matches_twin[G3]",
    "k_jac_sweep<2, 3, false>": "test_jacobian_matches_twin[ions2_sdi0]",
    "k_jac_sweep<3, 3, false>": "test_jacobian_matches_twin[ions3_tied]",
    "k_jac_sweep<4, 3, false>": "test_jacobian_matches_twin[ions4]",
    "k_jac_sweep<1, 1, false>": "test_jacobian_matches_twin[ppp5]",
    "k_jac_sweep<2, 1, false>": "test_jacobian_matches_twin[ions2_one]",
    "k_jac_sweep<3, 1, false>": "test_jacobian_matches_twin[ions3_one]",
    "k_jac_sweep<4, 1, false>": "test_jacobian_matches_twin[ions4_one]",
}


# ---------------------------------------------------------------------------------------------------------------------
# decks
# ---------------------------------------------------------------------------------------------------------------------
def _fract_active(cfg):
    for k, v in cfg["parameters"].items():
        if k.startswith("ion-"):
            v["fract"]["active"] = True
            v["Z"]["active"] = True


def _grad3(cfg):
    g = cfg["parameters"]["general"]
    for k in ("Te_gradient", "ne_gradient"):
        g[k]["num_grad_points"] = 3
        g[k]["active"] = True


def _no_ion_irf(cfg):
    cfg["other"]["PhysParams"]["widIRF"]["spect_stddev_ion"] = 0.0


def _deck(mod=None, **kw):
    def build():
        cfg = decks.deck_fit(**kw)
        if mod:
            mod(cfg)
        return cfg
    return build


WIDE = ("Te", "ne", "Ti", "Z", "Va", "lam", "amp1", "amp2")   # 8 leaves: groups of 3, 3 and a partial one of 2
PROD = ("Te", "ne", "m", "amp1", "amp2", "lam")
# id -> (deck builder, options): activate, fe ("per_lineout": a constant table per lineout), ranges of further draws
CASES = {
    "ions1": (_deck(), {}),
    "ions2": (_deck(_fract_active, n_ion=2, active=("Te", "ne", "Ti", "lam")), {}),
    "ions3_tied": (_deck(_fract_active, n_ion=3, active=("Te", "ne", "Ti", "Z", "Ti_same_3")), {}),
    "ions4": (_deck(_fract_active, n_ion=4, active=("Te", "ne", "Ti", "Z")), {}),
    "ppp2": (_deck(points_per_pixel=2), {}),
    "ppp5": (_deck(points_per_pixel=5, active=("ne", "lam", "amp1")), {}),   # (three leaves: the twin's 5120 samples per jvp set the test's time)
    "G3": (_deck(_grad3, active=("Te", "ne", "lam")), {}),
    "m": (_deck(nvx=128, active=PROD), dict(ranges=dict(m=(2.1, 4.3)))),
    "fe_const": (_deck(active=("Te", "ne", "Ti", "lam", "amp1")), dict(fe="per_lineout")),
    "raw": (_deck(), dict(activate=False)),
    "sdi0": (_deck(_no_ion_irf, active=("Te", "ne", "Ti", "lam")), {}),
    "wide": (_deck(active=WIDE), {}),
    "ions2_sdi0": (_deck(_no_ion_irf, n_ion=2, active=("Te", "ne", "Ti")), {}),   # two species on the tangent form (a raw ion feature)
    # a single leaf takes the one-tangent kernel: its instantiations for 2-4 ion species
    "ions2_one": (_deck(n_ion=2, active=("ne",)), {}),
    "ions3_one": (_deck(n_ion=3, active=("ne",)), {}),
    "ions4_one": (_deck(n_ion=4, active=("ne",)), {}),
}
assert len(WIDE) > JAC_WIDTH and len(WIDE) % JAC_WIDTH != 0


def _leaves(cfg, activate=True):
    """Trainable leaves in ravel order as (species, key), their oracle names and slots."""
    from tsadar_amd.params import SlotMap

    leaves = SlotMap(cfg["parameters"], activate).active_leaves
    names = [f"{k}_{int(sp.split('-')[1])}" if sp.startswith("ion-") else k for (sp, k), _ in leaves]
    return leaves, names, [s for _, s in leaves]


def _n_ion(cfg):
    return sum(1 for k in cfg["parameters"] if k.startswith("ion-"))


def _weights(cfg):
    ext = cfg["other"]["extraoptions"]
    c = 0.5 if (ext["fit_EPWb"] and ext["fit_EPWr"]) else 1.0
    return np.array([1.0 if ext["fit_IAW"] else 0.0, c if ext["fit_EPWb"] else 0.0, c if ext["fit_EPWr"] else 0.0])


def _constant_tables(nb, nvx, seed):
    """One f_e per lineout that no DLM order reproduces: a super-Gaussian times a smooth ripple, normalised on the velocity grid."""
    rng = np.random.default_rng(seed)
    vx = orc.velocity_grid(nvx)
    out = []
    for _ in range(nb):
        f = orc.dlm_fe(rng.uniform(2.0, 3.5), nvx) * np.exp(0.15 * np.sin(1.3 * vx + rng.uniform(0, 6.28)) + 0.05 * np.tanh(vx))
        out.append(f / np.sum(f) / (vx[1] - vx[0]))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    build, opt = CASES[cid]
    cfg = build()
    activate = opt.get("activate", True)
    n_ion = _n_ion(cfg)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=53, activate=activate)
    ranges = dict(opt.get("ranges", {}))
    if any(v["fract"]["active"] for k, v in cfg["parameters"].items() if k.startswith("ion-")):
        ranges.update({f"fract_{s}": (0.1, 0.9) for s in range(1, n_ion + 1)})   # drawn per lineout; their sum is never 1
    normed = util.random_lineouts(cfg, B, seed=103, activate=activate, ranges=ranges)
    fe = None
    if opt.get("fe") == "per_lineout":
        fe = _constant_tables(B, cfg["parameters"]["electron"]["fe"]["nvx"], 7)
    leaves, names, act = _leaves(cfg, activate)
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, fe=fe, activate=activate, n_ion=n_ion, leaves=leaves, names=names, act=act,
                X=util.normed_to_matrix(normed, n_ion))


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick: J of the twin, one jvp per (lineout, leaf)
# ---------------------------------------------------------------------------------------------------------------------
def _twin_jacobian_1(cfg, normed_b, batch_b, names, activate=True, fe_b=None):
    """-> (JE [n, 1024], JI [n, 1024], ThryE [1024], ThryI [1024], lamE, lamI) of one lineout."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    sa = util.sa_fit(1)
    base = {k: ot._t(v).clone() for k, v in normed_b.items()}
    axes = {}

    def f(vec):
        nm = dict(base)
        for i, k in enumerate(names):
            nm[k] = vec[i:i + 1]
        E, I, lamE, lamI = ot.ts_diag(cfg, sa, nm, batch_b, activate, fe_b)
        axes["lam"] = (lamE.detach().numpy(), lamI.detach().numpy())
        return torch.cat([E.reshape(-1), I.reshape(-1)])

    x0 = torch.cat([base[k].reshape(1) for k in names])
    rows, val = [], None
    for i in range(len(names)):
        v = torch.zeros_like(x0)
        v[i] = 1.0
        val, jv = torch.autograd.functional.jvp(f, x0, v)
        rows.append(jv.detach().numpy())
    J = np.array(rows)
    val = val.detach().numpy()
    return J[:, :1024], J[:, 1024:], val[:1024], val[1024:], axes["lam"][0].reshape(-1), axes["lam"][1].reshape(-1)


@functools.lru_cache(maxsize=None)
def _twin(cid):
    """The twin's Jacobians and spectra of the case's B lineouts: computed once, shared by the tests, never modified."""
    s = _inputs(cid)
    out = []
    for b in range(B):
        nb = {k: np.asarray(v)[b:b + 1] for k, v in s["normed"].items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in s["batch"].items()}
        out.append(_twin_jacobian_1(s["cfg"], nb, bb, s["names"], s["activate"], None if s["fe"] is None else s["fe"][b]))
    res = tuple(np.array([o[i] for o in out]) for i in range(6))
    for a in res:
        a.setflags(write=False)
    return res


def _loss_derivatives(method, d, t):
    """(l, dl/dt, d2l/dt2) of the Hessian loss per sample (denominators |d| + 1e-10 for l2)."""
    if method == "l2":
        u = np.abs(d) + 1e-10
        return (d - t) ** 2 / u, -2.0 * (d - t) / u, 2.0 / u
    if method == "log-cosh":
        th = np.tanh(d - t)
        return np.log(np.cosh(d - t)), -th, 1.0 - th * th
    assert method == "poisson"
    return t - d * np.log(t), 1.0 - d / t, d / t ** 2


def _gn_reference(cfg, batch, w, JE, JI, E, I, lamE, lamI):
    """(S [3], grad [B, n], gn [B, n, n]) in NumPy from the twin's J and spectra (E, I include the batch's noise)."""
    method = cfg["optimizer"]["loss_method"]
    iaw, blue, red = orc.fit_masks(cfg, lamE, lamI)
    nb, n = JE.shape[0], JE.shape[1]
    S, grad, gn = np.zeros(3), np.zeros((nb, n)), np.zeros((nb, n, n))
    for k, (mask, J, d, t) in enumerate(((iaw, JI, batch["i_data"], I), (blue, JE, batch["e_data"], E), (red, JE, batch["e_data"], E))):
        for b in range(nb):
            m = mask[b]
            l0, l1, l2 = _loss_derivatives(method, np.asarray(d)[b][m], t[b][m])
            S[k] += l0.sum()
            grad[b] += w[k] * (J[b][:, m] @ l1)
            gn[b] += w[k] * (J[b][:, m] * l2) @ J[b][:, m].T
    return S, grad, gn


def _sigmas_of(hess, batch_size):
    """The sigmas the reference's get_sigmas computes from the nested Hessian layout: per lineout the matrix of the [i, i]
    entries of every block, inverted; sign(diag) sqrt(|diag|)."""
    keys = [(sp, k) for sp in hess for k in hess[sp]]
    out = np.zeros((batch_size, len(keys)))
    for i in range(batch_size):
        Hm = np.array([[np.squeeze(hess[s1][k1][s2][k2])[i, i] for (s2, k2) in keys] for (s1, k1) in keys])
        d = np.diag(np.linalg.inv(Hm))
        out[i] = np.sign(d) * np.sqrt(np.abs(d))
    return out


def _assert_row_is_the_quotient(J, quotients, what):
    """J [R, 1024] rows; quotients: per step of FD_LADDER the central differences [R, 1024].  Per row: the pair of consecutive steps
    that agree best with each other must agree within FD_TOL of the row's maximum, and J must be within FD_TOL of both."""
    Q = np.array(quotients)                                     # [steps, R, 1024]
    scale = np.max(np.abs(J), axis=-1)                          # [R]
    for r in range(J.shape[0]):
        if scale[r] == 0.0:
            assert not Q[:, r].any(), what
            continue
        gap = np.max(np.abs(Q[1:, r] - Q[:-1, r]), axis=-1) / scale[r]
        k = int(np.argmin(gap))
        a, c = Q[k, r], Q[k + 1, r]
        err = max(np.max(np.abs(J[r] - a)), np.max(np.abs(J[r] - c))) / scale[r]
        print(f"{what} row {r}: steps {FD_LADDER[k]:.2e}, {FD_LADDER[k + 1]:.2e} agree to {gap[k]:.2e}; J within {err:.2e}")
        assert gap[k] <= FD_TOL, (what, r, FD_LADDER[k], gap)
        assert err <= FD_TOL, (what, r, FD_LADDER[k], err)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_interface_has_the_jacobian():
    from tsadar_amd.engine import Engine
    from tsadar_amd.loss_function import LossFunction

    header = open(os.path.join(ROOT, "include", "tsff.h")).read()
    for name in ("tsff_spectrum_jacobian", "tsff_loss_gauss_newton"):
        assert re.search(rf"\bint {name}\(tsff_handle \*h,", header), name
        assert name in L.EXPORTS
    for cls, attr in ((Engine, "spectrum_jacobian"), (Engine, "loss_gauss_newton"), (LossFunction, "jacobian"),
                      (LossFunction, "gn_loss_wrt_params")):
        assert callable(getattr(cls, attr, None)), (cls.__name__, attr)


def _library_kernels(path):
    data = open(path, "rb").read()
    mangled = sorted({m.decode()[:-3] if m.endswith(b".kd") else m.decode() for m in re.findall(rb"_ZN4tsff\d+k_jac_\w+", data)})
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^(void )?tsff::", "", s).split("(")[0] for s in out if s.strip()}


def test_every_jacobian_kernel_has_a_case():
    from tsadar_amd import build

    have = _library_kernels(build.build())
    assert have, "no k_jac_* kernel in libtsff.so"
    assert have == set(JAC_KERNELS), (sorted(have), sorted(JAC_KERNELS))
    for k, case in JAC_KERNELS.items():
        test, cid = case.rstrip("]").split("[")
        assert test in globals() and cid in CASES, (k, case)


def test_twin_jacobian_matches_differences_of_the_numpy_oracle():
    """The yardstick differentiates the right function: every twin row against central differences of orc.ts_diag, at two step
    sizes that agree with each other."""
    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "lam", "amp1"))
    sa = util.sa_fit(1)
    batch = util.synthetic_batch(cfg, sa, 1, seed=13)
    normed = util.random_lineouts(cfg, 1, seed=14)
    _, names, _ = _leaves(cfg)
    JE, JI = _twin_jacobian_1(cfg, normed, batch, names)[:2]

    def cd(k, h):
        p, m = copy.deepcopy(normed), copy.deepcopy(normed)
        p[k] = np.asarray(p[k], dtype=np.float64) + h
        m[k] = np.asarray(m[k], dtype=np.float64) - h
        Ep, Ip = orc.ts_diag(cfg, sa, p, batch)[:2]
        Em, Im = orc.ts_diag(cfg, sa, m, batch)[:2]
        return (Ep[0] - Em[0]) / (2 * h), (Ip[0] - Im[0]) / (2 * h)

    for i, k in enumerate(names):
        quotients = [cd(k, h) for h in FD_LADDER]
        for f, J in enumerate((JE[i], JI[i])):
            _assert_row_is_the_quotient(J[None], [q[f][None] for q in quotients], k)


def _twin_hess_loss(cfg, sa, normed, batch):
    """_loss_for_hess_fn_ with l2 on the twin (the construction of tests/test_hessian_exact.py's _twin_loss)."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    E, I, lamE, lamI = ot.ts_diag(cfg, sa, normed, batch, True, None)
    ext = cfg["other"]["extraoptions"]
    iaw, blue, red = orc.fit_masks(cfg, lamE.detach().numpy(), lamI.detach().numpy())

    def fun(d, t):
        d = ot._t(d)
        return torch.square(d - t) / (torch.abs(d) + 1e-10)

    z = torch.zeros((), dtype=torch.float64)
    i_err = fun(batch["i_data"], I)[torch.as_tensor(iaw)].sum() if ext["fit_IAW"] else z
    e_err = z
    if ext["fit_EPWb"]:
        e_err = e_err + fun(batch["e_data"], E)[torch.as_tensor(blue)].sum()
    if ext["fit_EPWr"]:
        e_err = e_err + fun(batch["e_data"], E)[torch.as_tensor(red)].sum()
        if ext["fit_EPWb"]:
            e_err = e_err * 0.5
    return i_err + e_err


def test_gn_yardstick_is_the_hessian_at_zero_residual():
    """With data = model the residual-weighted second derivatives of the model drop out of the exact Hessian: what is left is
    2 sum_k w_k J J^T / u -- the definition of gn, weights and the halving of the two EPW ranges included."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    cfg = decks.deck_fit(active=("Te", "ne", "Ti", "lam", "amp1"))
    assert cfg["optimizer"]["loss_method"] == "l2"
    sa = util.sa_fit(1)
    batch = util.synthetic_batch(cfg, sa, 1, seed=13)
    batch["noise_e"] = np.zeros((1, 1024))
    batch["noise_i"] = np.zeros((1, 1024))
    normed = util.random_lineouts(cfg, 1, seed=14)
    _, names, _ = _leaves(cfg)
    JE, JI, E, I, lamE, lamI = _twin_jacobian_1(cfg, normed, batch, names)
    batch["e_data"], batch["i_data"] = E[None].copy(), I[None].copy()
    base = {k: ot._t(v).clone() for k, v in normed.items()}

    def f(vec):
        nm = dict(base)
        for i, k in enumerate(names):
            nm[k] = vec[i:i + 1]
        return _twin_hess_loss(cfg, sa, nm, batch)

    H = torch.autograd.functional.hessian(f, torch.cat([base[k].reshape(1) for k in names])).numpy()
    w = _weights(cfg)
    assert w[1] == 0.5 and w[2] == 0.5 and w[0] == 1.0
    gn = _gn_reference(cfg, batch, w, JE[None], JI[None], E[None], I[None], lamE[None], lamI[None])[2][0]
    assert np.max(np.abs(H - gn)) <= 1e-9 * np.max(np.abs(H)), np.max(np.abs(H - gn)) / np.max(np.abs(H))


def test_refusals_before_device_work():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    active = ("Te", "ne", "Ti", "lam", "amp1")
    sa = util.sa_fit(2)
    batch = util.synthetic_batch(decks.deck_fit(active=active), sa, 2, seed=5)

    def refused(lf, tp, match, calls):
        before = copy.deepcopy(lf.cfg)
        for call in calls:
            with pytest.raises(NotImplementedError, match=match):
                getattr(lf, call)(tp, batch)
        assert lf.cfg == before
        assert not lf.ts_diag._engines   # (no engine was created: nothing reached the device)

    cfg = decks.deck_angular(1, 64, (128, 256), 10, 100)   # a real angular_full deck
    lfa = LossFunction(cfg, util._angular_sa(cfg), batch)
    assert lfa.angular
    refused(lfa, ThomsonParams(cfg["parameters"], 1, batch=True, activate=True), "angular", ("jacobian", "gn_loss_wrt_params"))

    cfg = decks.deck_fit(active=active)
    nvx = cfg["parameters"]["electron"]["fe"]["nvx"]
    cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": nvx, "params": {"init_m": 2.4}}
    tp = ThomsonParams(cfg["parameters"], 2, batch=True, activate=True)
    assert tp.fval is not None and tp.slots.fval_active
    refused(LossFunction(cfg, sa, batch), tp, "free-form", ("jacobian", "gn_loss_wrt_params"))

    cfg = decks.deck_fit(active=active)
    cfg["optimizer"]["loss_method"] = "l1"
    refused(LossFunction(cfg, sa, batch), ThomsonParams(cfg["parameters"], 2, batch=True, activate=True), "l1", ("gn_loss_wrt_params",))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _engine(s, **kw):
    from tsadar_amd.engine import Engine

    if s["fe"] is not None:
        kw.setdefault("fe_mode", L.FE_PER_LINEOUT)
    return Engine(s["cfg"], s["sa"], activate=s["activate"], **kw)


def _sync():
    import torch

    torch.cuda.synchronize()


def _record(key, text):
    """One line per case in profiles/jacobian_pytest.txt: the case's previous line is replaced."""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    lines = {}
    if os.path.exists(RECORD):
        lines = {l.split(" ", 1)[0]: l.rstrip("\n") for l in open(RECORD) if l.strip()}
    lines[key] = f"{key} {text}"
    with open(RECORD, "w") as f:
        f.write("".join(v + "\n" for _, v in sorted(lines.items())))


def _row_ratios(Jd, Jt):
    """max_j |Jd - Jt| / max_j |Jt| per (lineout, leaf) row; a row that is identically zero in the twin must be exactly zero."""
    scale = np.max(np.abs(Jt), axis=-1)
    err = np.max(np.abs(Jd - Jt), axis=-1)
    zero = scale == 0.0
    assert not np.any(Jd[zero]), "a row that is zero in the twin is not exactly zero on the device"
    return np.where(zero, 0.0, err / np.where(zero, 1.0, scale))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_jacobian_matches_twin(cid):
    s = _inputs(cid)
    eng = _engine(s)
    JE, JI = eng.spectrum_jacobian(s["X"], s["batch"]["e_amps"], s["batch"]["i_amps"], s["act"], fe=s["fe"])
    _sync()
    launched = eng.last_launch()
    mine = [k for k in launched if k.startswith("k_jac_")]
    assert len(mine) == 1 and mine[0] in JAC_KERNELS, launched
    for k, case in JAC_KERNELS.items():
        if case == f"test_jacobian_matches_twin[{cid}]":
            assert mine[0] == k, (launched, k)
    assert all(k.startswith(("k_jac_", "k_fe_", "k_wgemm")) for k in launched), launched
    width = int(mine[0].split(",")[1])   # k_jac_sweep<NI, W, ROWS>
    if cid == "wide":
        assert width == JAC_WIDTH and len(s["act"]) > width and len(s["act"]) % width != 0, (mine[0], len(s["act"]))
    tJE, tJI = _twin(cid)[:2]
    rE, rI = _row_ratios(JE.cpu().numpy(), tJE), _row_ratios(JI.cpu().numpy(), tJI)
    worst = max(rE.max(), rI.max())
    print(f"{cid}: largest row ratio {worst:.3e} (ele {rE.max():.3e}, ion {rI.max():.3e}), {mine[0]}")
    _record(f"test_jacobian_matches_twin[{cid}]", f"{mine[0].replace(' ', '')} n={len(s['act'])} max_row_ratio={worst:.3e} ele={rE.max():.3e} ion={rI.max():.3e}")
    assert worst <= ROW_TOL, (cid, s["names"], rE, rI)


@pytest.mark.gpu
def test_jacobian_is_the_derivative_of_forward():
    """J against central differences of the shipped forward itself (not only the twin)."""
    s = _inputs("ions1")
    eng = _engine(s)
    ea, ia = s["batch"]["e_amps"], s["batch"]["i_amps"]
    JE, JI = [t.cpu().numpy() for t in eng.spectrum_jacobian(s["X"], ea, ia, s["act"])]

    def cd(slot, h):
        Xp, Xm = s["X"].copy(), s["X"].copy()
        Xp[:, slot] += h
        Xm[:, slot] -= h
        Ep, Ip = [t.cpu().numpy() for t in eng.forward(Xp, ea, ia)]
        Em, Im = [t.cpu().numpy() for t in eng.forward(Xm, ea, ia)]
        return (Ep - Em) / (2 * h), (Ip - Im) / (2 * h)

    for i, slot in enumerate(s["act"]):
        quotients = [cd(slot, h) for h in FD_LADDER]
        for f, J in enumerate((JE[:, i], JI[:, i])):
            _assert_row_is_the_quotient(J, [q[f] for q in quotients], s["names"][i])


def _with_method(s, method):
    cfg = copy.deepcopy(s["cfg"])
    cfg["optimizer"]["loss_method"] = method
    return dict(s, cfg=cfg)


# the three loss functionals on ions1 (two full groups), and the rows parked by a partial last group (wide: 3 + 3 + 2 leaves) and with
# several ion species, tied Ti and renormalised fractions (ions3_tied: 8 leaves): the twin's J of those cases is shared with test 5
GN_CASES = {"l2": ("ions1", "l2"), "log-cosh": ("ions1", "log-cosh"), "poisson": ("ions1", "poisson"),
            "l2-wide": ("wide", "l2"), "l2-ions3_tied": ("ions3_tied", "l2")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GN_CASES))
def test_gauss_newton_matches_twin(case):
    cid, method = GN_CASES[case]
    s = _with_method(_inputs(cid), method)   # (the twin's J and spectra do not depend on the loss: those of the Jacobian case)
    eng = _engine(s)
    w = _weights(s["cfg"])
    terms, grad, gn = [t.cpu().numpy() for t in eng.loss_gauss_newton(s["X"], s["batch"], w, s["act"])]
    launched = eng.last_launch()
    mine = [k for k in launched if k.startswith(f"k_jac_sweep<{s['n_ion']}, ")]
    assert len(mine) == 1 and "k_loss_reduce" in launched, launched
    assert len(s["act"]) % int(mine[0].split(",")[1]) != 0 or cid == "ions1"
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
    S, g_ref, gn_ref = _gn_reference(s["cfg"], s["batch"], w, *_twin(cid))
    assert np.max(np.abs(terms - S)) <= GN_TOL * np.max(np.abs(S)), (terms, S)
    gh = eng.loss_hess(s["X"], s["batch"], w, s["act"])[1].cpu().numpy()
    for b in range(B):
        assert np.max(np.abs(gn[b] - gn_ref[b])) <= GN_TOL * np.max(np.abs(gn_ref[b])), (b, np.max(np.abs(gn[b] - gn_ref[b])) / np.max(np.abs(gn_ref[b])))
        assert np.max(np.abs(grad[b] - g_ref[b])) <= GN_TOL * np.max(np.abs(g_ref[b])), (b, grad[b], g_ref[b])
        assert np.max(np.abs(grad[b] - gh[b])) <= GN_TOL * np.max(np.abs(gh[b])), (b, grad[b], gh[b])
        assert np.all(np.linalg.eigvalsh(gn[b]) >= -1e-12 * np.max(np.abs(gn[b])))   # positive semi-definite


@pytest.mark.gpu
def test_gauss_newton_is_the_exact_hessian_at_zero_residual():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    s = _inputs("ions1")
    cfg = s["cfg"]
    assert cfg["optimizer"]["loss_method"] == "l2"
    eng = _engine(s)
    batch = dict(s["batch"], noise_e=np.zeros((B, 1024)), noise_i=np.zeros((B, 1024)))
    E, I = eng.forward(s["X"], batch["e_amps"], batch["i_amps"])
    batch["e_data"], batch["i_data"] = E.cpu().numpy(), I.cpu().numpy()
    w = _weights(cfg)
    gn = eng.loss_gauss_newton(s["X"], batch, w, s["act"])[2].cpu().numpy()
    H = eng.loss_hess(s["X"], batch, w, s["act"])[2].cpu().numpy()
    for b in range(B):
        assert np.max(np.abs(gn[b] - H[b])) <= GN_TOL * np.max(np.abs(H[b])), (b, np.max(np.abs(gn[b] - H[b])) / np.max(np.abs(H[b])))
    lf = LossFunction(cfg, s["sa"], batch)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    tp.X[:] = s["X"]
    hg = lf.gn_loss_wrt_params(tp, batch)
    he = lf.h_loss_wrt_params(tp, batch, method="exact")
    assert [(sp, k) for sp in hg for k in hg[sp]] == [(sp, k) for sp in he for k in he[sp]]
    for (sp, k), _ in s["leaves"]:
        assert hg[sp][k][sp][k].shape == (B, B)
    np.testing.assert_allclose(_sigmas_of(hg, B), _sigmas_of(he, B), rtol=SIGMA_RTOL)
    jd = lf.jacobian(tp, batch)
    assert jd["leaves"] == [l for l, _ in s["leaves"]] and jd["ele"].shape == (B, len(s["act"]), 1024) == jd["ion"].shape


def _raw_jacobian(eng, X, ea, ia, act, JE, JI, B_=None):
    import ctypes as C

    a = None if act is None else np.ascontiguousarray(act, dtype=np.int32)
    n = 0 if a is None else a.size
    p = eng._ptr
    return eng.lib.tsff_spectrum_jacobian(eng.h, p(X), p(None), p(ea), p(ia), X.shape[0] if B_ is None else B_,
                                          None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)), n, p(JE), p(JI))


def _raw_gauss_newton(eng, X, db, w, act, out):
    import ctypes as C

    a = np.ascontiguousarray(act, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    p = eng._ptr
    return eng.lib.tsff_loss_gauss_newton(eng.h, p(X), p(None), p(db["e_data"]), p(db["i_data"]), p(db["e_amps"]), p(db["i_amps"]),
                                          p(db["noise_e"]), p(db["noise_i"]), X.shape[0], w.ctypes.data_as(L.c_double_p),
                                          a.ctypes.data_as(C.POINTER(C.c_int32)), a.size, p(out[0]), p(out[1]), p(out[2]))


@pytest.mark.gpu
def test_jacobian_calls_are_reproducible_and_refuse_cleanly():
    import torch
    from tsadar_amd.engine import Engine

    s = _inputs("ions1")
    eng = _engine(s)
    ea, ia = s["batch"]["e_amps"], s["batch"]["i_amps"]
    w = _weights(s["cfg"])
    act, n = s["act"], len(s["act"])
    # two calls: bit-identical
    a = [t.cpu().numpy() for t in eng.spectrum_jacobian(s["X"], ea, ia, act)]
    b = [t.cpu().numpy() for t in eng.spectrum_jacobian(s["X"], ea, ia, act)]
    g1 = [t.cpu().numpy() for t in eng.loss_gauss_newton(s["X"], s["batch"], w, act)]
    g2 = [t.cpu().numpy() for t in eng.loss_gauss_newton(s["X"], s["batch"], w, act)]
    for x, y in zip(a + g1, b + g2):
        assert np.array_equal(x, y)
    # one output missing: the other one bit for bit, the missing one untouched
    X = eng.dev(s["X"])
    ead, iad = eng._vec(ea, B), eng._vec(ia, B)
    eng._sync_stream()
    for keep in (0, 1):
        out = [torch.full((B, n, 1024), -7.0, dtype=torch.float64, device=eng.device) for _ in range(2)]
        rc = _raw_jacobian(eng, X, ead, iad, act, out[0] if keep == 0 else None, out[1] if keep == 1 else None)
        assert rc == 0, eng.lib.tsff_last_error(eng.h)
        _sync()
        assert np.array_equal(out[keep].cpu().numpy(), a[keep])
        assert torch.all(out[1 - keep] == -7.0)
    # refusals: the code, and nothing enqueued
    JE = torch.empty((B, n, 1024), dtype=torch.float64, device=eng.device)
    JI = torch.empty_like(JE)
    db = dict(e_amps=ead, i_amps=iad, e_data=eng._mat(s["batch"]["e_data"], B), i_data=eng._mat(s["batch"]["i_data"], B),
              noise_e=None, noise_i=None)
    gout = [torch.empty(3, dtype=torch.float64, device=eng.device), torch.empty((B, n), dtype=torch.float64, device=eng.device),
            torch.empty((B, n, n), dtype=torch.float64, device=eng.device)]

    def refused(e, rc, code):
        assert rc == code, (rc, code, e.lib.tsff_last_error(e.h))
        assert e.last_launch() == [], e.last_launch()

    refused(eng, _raw_jacobian(eng, X, ead, iad, None, JE, JI), -1)                      # null slot list
    refused(eng, _raw_jacobian(eng, X, ead, iad, act, None, None), -1)                   # no output at all
    refused(eng, _raw_jacobian(eng, None, ead, iad, act, JE, JI, B_=B), -1)              # null params
    refused(eng, _raw_jacobian(eng, X, ead, iad, [L.P_TE, L.P_TE], JE, JI), -1)          # repeated slot
    refused(eng, _raw_jacobian(eng, X, ead, iad, [L.P_TE, 99], JE, JI), -1)              # slot out of range
    refused(eng, _raw_jacobian(eng, X, ead, iad, [L.P_M], JE, JI), -2)                   # m without a DLM
    refused(eng, _raw_jacobian(eng, X, ead, iad, [L.P_TE, L.P_ION0 + L.ION_A], JE, JI), -3)
    refused(eng, _raw_gauss_newton(eng, X, db, w, [L.P_TE, L.P_TE], gout), -1)
    refused(eng, _raw_gauss_newton(eng, X, db, w, [L.P_M], gout), -2)
    refused(eng, _raw_gauss_newton(eng, X, db, w, [L.P_ION0 + L.ION_A], gout), -3)
    refused(eng, _raw_gauss_newton(eng, X, dict(db, e_data=None), w, act, gout), -1)     # data missing
    # l1: the Gauss-Newton matrix vanishes
    l1 = _with_method(s, "l1")
    e1 = _engine(l1)
    e1._sync_stream()
    refused(e1, _raw_gauss_newton(e1, X, db, w, act, gout), -2)
    assert b"l1" in e1.lib.tsff_last_error(e1.h)
    # a feature that is not loaded
    cfg = copy.deepcopy(s["cfg"])
    cfg["other"]["extraoptions"].update(load_ion_spec=False, fit_IAW=False)
    eo = Engine(cfg, s["sa"])
    eo._sync_stream()
    refused(eo, _raw_jacobian(eo, X, ead, None, act, JE, JI), -1)
    je, ji = eo.spectrum_jacobian(s["X"], ea, ia, act)
    assert ji is None and np.array_equal(je.cpu().numpy(), a[0])
    # LDS budget: ten points per pixel do not fit with even one tangent
    big = Engine(decks.deck_fit(points_per_pixel=10), s["sa"])
    big._sync_stream()
    refused(big, _raw_jacobian(big, X, ead, iad, act, JE, JI), -2)
    assert b"LDS" in big.lib.tsff_last_error(big.h)
    # a non-default stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = [t for t in eng.spectrum_jacobian(s["X"], ea, ia, act)]
        g3 = [t for t in eng.loss_gauss_newton(s["X"], s["batch"], w, act)]
    st.synchronize()
    for x, y in zip(a + g1, c + g3):
        assert np.array_equal(x, y.cpu().numpy())
