"""The SphericalHarmonics f_e generator on the device: tsff_sph_table / tsff_sph_table_vjp (Engine.sph_table, sph_table_vjp),
the TSFF_ANG_SPH generator of tsff_angular_fit and loops.angular_loop(train_generator=True).

The independent check is ``_twin``: a torch-float64 CPU restatement of ``SphericalHarmonics.__call__`` (its own gamma through
``torch.lgamma``, its own interpolation), differentiated by autograd.  It reproduces the host generator to a few 1e-16 of the
table's maximum (asserted to 1e-14 below); its derivative is exact, where ``SphericalHarmonics.vjp`` takes central differences
for the order of f00 and the Mora-Yahi gradient lengths and misses them by 1e-9 .. 3e-8.

Bounds.  Table: 1e-13 of its maximum (the twin's 4e-16 plus a few ulp of the device's pow / exp / tgamma).  Gradient: 1e-11 of
the largest entry of each parameter group -- two exact CPU derivations agree to 8e-16, a central difference misses by >= 1e-9,
so only an exact adjoint passes.  Loop: the project's own bounds for the angular loop, 1e-9 relative on every epoch's loss and
1e-8 on the final and best leaves, against the host loop with ``SphericalHarmonics.vjp`` replaced by the twin's autograd (both
sides then take exact gradients)."""
import copy
import functools
import inspect

import numpy as np
import pytest

import decks
import util
from util import _angular_sa, _host_loop, _rel

N_EPOCHS = 30
ROWS = (10, 110)   # lineouts of the 128 x 256 CCD (as tests/test_angular_loop_device.py)


def _fe_cfg(flm_type, nvx, nvr, init_m=2.2, Nl=1, active=True):
    p = {"flm_type": flm_type, "init_m": init_m, "Nl": Nl, "nvr": nvr}
    if flm_type == "mora-yahi":
        p.update(LTx=225000.0, LTy=400000.0)
    return {"active": active, "dim": 2, "type": "sphericalharmonic", "nvx": nvx, "params": p}


# (name, flm_type, nvx, nvr, init_m, Nl): the settings of the table and gradient tests
CASES = [("my48", "mora-yahi", 48, 48, 2.2, 1), ("my64", "mora-yahi", 64, 64, 3.4, 1), ("free", "arbitrary", 48, 40, 2.2, 1),
         ("free_l2", "arbitrary", 48, 40, 3.4, 2)]


def _make(name):
    """The host generator of a case.  Free radial functions: flm_sign ~ normal(0, 1), flm_mag ~ normal(0, 1) - 3 (a setting
    that floors about half of the points at 1e-32, none of them within rounding of the floor)."""
    from tsadar_amd import distribution as Dist

    _, flm_type, nvx, nvr, init_m, Nl = next(c for c in CASES if c[0] == name)
    sph = Dist.SphericalHarmonics(_fe_cfg(flm_type, nvx, nvr, init_m, Nl))
    if flm_type == "arbitrary":
        rng = np.random.default_rng(11)
        for key in sorted(sph.flm):
            sph.flm[key]["flm_sign"] = rng.normal(0.0, 1.0, nvr)
            sph.flm[key]["flm_mag"] = rng.normal(0.0, 1.0, nvr) - 3.0
    return sph


# ---------------------------------------------------------------------------------------------------------------------
# the torch-f64 twin
# ---------------------------------------------------------------------------------------------------------------------
def _twin(sph, theta):
    """SphericalHarmonics.__call__ restated in torch float64 for ``theta`` (a tensor in get_params() order)."""
    import torch
    from tsadar_amd import distribution as Dist

    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    gam = lambda x: torch.exp(torch.lgamma(x))
    vr, nvr = T(sph.vr), sph.vr.size
    m = torch.sigmoid(theta[-1]) * 3.0 + 2.0
    v0 = 1.0 / torch.sqrt(gam(5.0 / m) / 3.0 / gam(3.0 / m))
    f00 = m / (4 * np.pi * gam(3.0 / m)) / v0**3 * torch.exp(-((vr / v0) ** m))
    f00 = f00 / (torch.sum(f00 * 4 * np.pi * vr**2) * (vr[1] - vr[0]))
    # np.interp(vr_vxvy, vr, a, right=r): below the first node its value, above the last the constant
    q = sph.vr_vxvy.ravel()
    hi = np.clip(np.searchsorted(sph.vr, q, side="right"), 1, nvr - 1)
    x0, x1 = sph.vr[hi - 1], sph.vr[hi]
    t = T(np.clip((q - x0) / (x1 - x0), 0.0, 1.0))
    inside = torch.as_tensor(q <= sph.vr[-1])
    lo, hi = torch.as_tensor(hi - 1), torch.as_tensor(hi)

    def interp(a, right):
        return torch.where(inside, a[lo] + (a[hi] - a[lo]) * t, torch.full_like(t, right))

    f = interp(f00, 1e-16)
    o = 0
    for (l, mm) in sorted(sph.flm):
        if sph.flm_type == "mora-yahi":
            ve = gam(5.0 / m) / 3 / gam(3.0 / m)
            lam_v = (vr / ve) ** 4.0
            coeff = (m / 2 * vr**m - 5 * m / 12 * gam(8 / m) / gam(6 / m) * vr ** (m - 2) - 1.5) * lam_v
            rad = coeff / 10 ** theta[o] * f00
            o += 1
        else:
            w = np.hanning(nvr // 4)
            w = w / w.sum()
            M = T(np.stack([np.convolve(e, w, mode="same") for e in np.eye(nvr)], axis=1))
            sign, mag = theta[o : o + nvr], theta[o + nvr : o + 2 * nvr]
            o += 2 * nvr
            rad = 10 ** (-torch.sigmoid(M @ mag) * 10) * torch.tanh(M @ sign)
        f = f + interp(rad, 1e-32) * T(Dist.real_sph_harm(l, mm, sph.phi, sph.th).ravel())
    f = torch.where(f > 1e-32, f, torch.full_like(f, 1e-32))
    f = f / (torch.sum(f) * (sph.vx[1] - sph.vx[0]) ** 2)
    return f.reshape(sph.nvx, sph.nvx)


def _twin_vjp(sph, fe_bar):
    import torch

    theta = torch.tensor(sph.get_params(), dtype=torch.float64, requires_grad=True)
    loss = torch.sum(_twin(sph, theta) * torch.as_tensor(np.asarray(fe_bar, dtype=np.float64)))
    (g,) = torch.autograd.grad(loss, theta)
    return g.numpy().copy()


def _groups(sph):
    """name -> slice of get_params(): the parameter groups the gradient bound is taken over."""
    nvr, out, o = sph.vr.size, {}, 0
    for key in sorted(sph.flm):
        if sph.flm_type == "mora-yahi":
            out.setdefault("log_10_LT", []).append(o)
            o += 1
        else:
            out.setdefault("flm_sign", []).extend(range(o, o + nvr))
            out.setdefault("flm_mag", []).extend(range(o + nvr, o + 2 * nvr))
            o += 2 * nvr
    out["normed_m"] = [o]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_twin_matches_the_host_generator(name):
    import torch

    sph = _make(name)
    want = sph()
    got = _twin(sph, torch.tensor(sph.get_params(), dtype=torch.float64)).numpy()
    err = np.max(np.abs(got - want)) / np.max(want)
    print(name, "twin vs host generator:", err)
    assert err <= 1e-14


def _unpack(sph):
    from tsadar_amd import distribution as Dist

    gd, meta = Dist.sph_gen_data(sph)
    lay = Dist.sph_gen_layout(meta["sph_type"], meta["n_harm"], meta["nv"], meta["nvr"])
    assert gd.dtype == np.float64 and gd.size == lay["size"]
    return {k: gd[v[0] : v[0] + int(np.prod(v[1]))].reshape(v[1]) for k, v in lay.items() if k != "size"}, meta


@pytest.mark.parametrize("name", ["my48", "free"])
def test_gen_data_reproduces_the_host_generator(name):
    """The packed constants, evaluated in NumPy the way the kernels evaluate them (cell, weight, inside flag, Y; for the free
    radial functions M and the CSR list), give the host generator's table and the np.bincount pair of SphericalHarmonics.vjp."""
    from tsadar_amd import distribution as Dist

    sph = _make(name)
    D, meta = _unpack(sph)
    nvr, keys = sph.vr.size, sorted(sph.flm)
    assert meta == dict(sph_type=Dist.SPH_MORA_YAHI if name == "my48" else Dist.SPH_ARBITRARY, n_harm=len(keys), nv=sph.nvx, nvr=nvr,
                        n_gen=sph.get_params().size)
    assert np.array_equal(D["vr"], sph.vr)
    i, t, ins = D["cell"].astype(int), D["wt"], D["inside"] != 0
    assert i.min() >= 0 and i.max() <= nvr - 2 and t.min() >= 0.0 and t.max() <= 1.0
    f00 = sph.get_f00()
    lerp = lambda a, right: np.where(ins, a[i] + t * (a[i + 1] - a[i]), right)
    f = lerp(f00, 1e-16)
    for h, (l, m) in enumerate(keys):
        if name == "free":   # the radial function through the packed smoothing matrix
            prm = sph.flm[(l, m)]
            rad = 10.0 ** (-10.0 / (1.0 + np.exp(-(D["M"] @ prm["flm_mag"])))) * np.tanh(D["M"] @ prm["flm_sign"])
            assert np.max(np.abs(rad - sph.radial(l, m, f00))) <= 1e-15 * np.max(np.abs(rad))
        else:
            rad = sph.radial(l, m, f00)
        f = f + lerp(rad, 1e-32) * D["Y"][h]
    f = np.maximum(f, 1e-32)
    f = f / (np.sum(f) * (sph.vx[1] - sph.vx[0]) ** 2)
    want = sph()
    assert np.max(np.abs(f.reshape(want.shape) - want)) <= 1e-14 * np.max(want)
    if name == "free":
        # the transposed interpolation: CSR list against the np.bincount pair
        g = np.random.default_rng(2).normal(size=i.size)
        ptr, pt, cw = D["ptr"].astype(int), D["pt"].astype(int), D["cw"]
        assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == 2 * int(ins.sum()) <= pt.size
        assert pt[: ptr[-1]].min() >= 0 and pt[: ptr[-1]].max() < i.size and not pt[ptr[-1] :].any() and not cw[ptr[-1] :].any()
        got = np.array([np.sum(cw[ptr[k] : ptr[k + 1]] * g[pt[ptr[k] : ptr[k + 1]]]) for k in range(nvr)])
        gi = g * ins
        want = np.bincount(i, weights=gi * (1.0 - t), minlength=nvr) + np.bincount(i + 1, weights=gi * t, minlength=nvr)
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
        for k in range(nvr):   # every list in the order of the grid points
            assert np.all(np.diff(pt[ptr[k] : ptr[k + 1]]) >= 0)


def test_gen_data_refuses_the_nn_radial_functions():
    from tsadar_amd import distribution as Dist

    cfg = _fe_cfg("nn", 48, 48)
    with pytest.raises(NotImplementedError):
        Dist.sph_gen_data(Dist.SphericalHarmonics(cfg))


def test_interface_has_the_generator():
    from tsadar_amd import _lib as L
    from tsadar_amd import loops
    from tsadar_amd.engine import Engine

    p = inspect.signature(loops.angular_loop).parameters
    assert "train_generator" in p and p["train_generator"].default is False
    assert list(p)[:3] == ["config", "all_data", "sa"]
    assert L.ANG_SPH == 3 and (L.SPH_MORA_YAHI, L.SPH_ARBITRARY) == (0, 1)
    assert "tsff_sph_table" in L.EXPORTS and "tsff_sph_table_vjp" in L.EXPORTS
    assert callable(Engine.sph_table) and callable(Engine.sph_table_vjp)
    fields = [f[0] for f in L.TsffAngularSpec._fields_]
    assert fields[-4:] == ["sph_type", "n_harm", "nvr", "n_gen"]


def test_angular_spec_layout_matches_c():
    """sizeof / offsetof of tsff_angular_spec from a gcc probe against the ctypes mirror (the new fields sit at the end)."""
    import ctypes as C
    import os
    import subprocess
    import tempfile

    from tsadar_amd import _lib as L

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f[0] for f in L.TsffAngularSpec._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "tsff.h"\nint main(){\nprintf("%zu\\n", sizeof(tsff_angular_spec));\n'
    prog += "".join(f'printf("%zu\\n", offsetof(tsff_angular_spec, {f}));\n' for f in fields) + "return 0;}\n"
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "p.c"), os.path.join(td, "p")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe], check=True)
        vals = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert vals[0] == C.sizeof(L.TsffAngularSpec)
    for f, off in zip(fields, vals[1:]):
        assert getattr(L.TsffAngularSpec, f).offset == off, f


def test_train_generator_refuses_nn_before_device_work():
    """flm_type nn stays on the host: refused before the config is mutated and before an engine is created (on a machine
    without a device, creating one raises TsffError, not NotImplementedError)."""
    from tsadar_amd import loops

    cfg = decks.deck_angular(2, 48, (128, 256), *ROWS)
    cfg["optimizer"]["method"] = "adam"
    cfg["parameters"]["electron"]["fe"] = _fe_cfg("nn", 48, 48)
    before = copy.deepcopy(cfg)
    with pytest.raises(NotImplementedError, match="nn"):
        loops.angular_loop(cfg, {}, {}, train_generator=True)
    assert cfg == before
    # and the default still refuses a trainable generator of a type the device builds
    cfg["parameters"]["electron"]["fe"] = _fe_cfg("mora-yahi", 48, 48)
    before = copy.deepcopy(cfg)
    with pytest.raises(NotImplementedError, match="trainable SphericalHarmonics"):
        loops.angular_loop(cfg, {}, {})
    assert cfg == before


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def eng(torch_mod):
    """One engine for the stand-alone generator calls (they use the handle's stream and scratch only)."""
    from tsadar_amd.engine import Engine

    cfg = decks.deck_angular(2, 48, (128, 256), *ROWS)
    return Engine(cfg, _angular_sa(cfg))


@pytest.fixture(scope="module")
def refs():
    """name -> (sph, gen_data, meta, host table, fe_bar, the twin's gradient), computed once."""
    from tsadar_amd import distribution as Dist

    out = {}
    for name, *_ in CASES:
        sph = _make(name)
        gd, meta = Dist.sph_gen_data(sph)
        fe_bar = np.random.default_rng(7).normal(size=(sph.nvx, sph.nvx))
        out[name] = (sph, gd, meta, sph(), fe_bar, _twin_vjp(sph, fe_bar))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_sph_table_matches_the_host_generator(eng, refs, name):
    sph, gd, meta, want, _, _ = refs[name]
    got = eng.download(eng.sph_table(sph.get_params(), gd, meta))
    if name.startswith("free"):   # the setting floors a large part of the table
        floored = np.sum(want == want.min())
        assert floored > want.size // 4, floored
    err = np.max(np.abs(got - want)) / np.max(want)
    print(name, "device table vs host generator:", err)
    assert err <= 1e-13


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_sph_table_vjp_matches_autograd_and_is_reproducible(eng, refs, name):
    sph, gd, meta, _, fe_bar, want = refs[name]
    theta = eng.dev(sph.get_params())
    gdd, fb = eng.dev(gd), eng.dev(fe_bar)
    got = eng.download(eng.sph_table_vjp(theta, gdd, meta, fb))
    again = eng.download(eng.sph_table_vjp(theta, gdd, meta, fb))
    assert np.array_equal(got, again), "two calls on the same input differ"
    assert np.all(np.isfinite(got))
    for group, idx in _groups(sph).items():
        err = np.max(np.abs(got[idx] - want[idx])) / np.max(np.abs(want[idx]))
        print(name, group, "device vjp vs autograd:", err)
        assert err <= 1e-11, (group, err)


@pytest.mark.gpu
def test_sph_entry_points_refuse_inconsistent_sizes(eng, refs):
    from tsadar_amd import _lib as L

    sph, gd, meta, _, fe_bar, _ = refs["my48"]
    eng.sph_table(sph.get_params(), gd, meta)
    torch = eng.torch
    torch.cuda.synchronize()
    th, gdd = eng.dev(sph.get_params()), eng.dev(gd)
    fe = torch.empty((48, 48), dtype=torch.float64, device=eng.device)
    for bad in (dict(sph_type=7), dict(n_harm=3), dict(n_gen=4), dict(nvr=1), dict(sph_type=L.SPH_ARBITRARY)):
        m = dict(meta, **bad)
        eng._sync_stream()
        rc = eng.lib.tsff_sph_table(eng.h, *eng._sph_args(m, 0.25), eng._ptr(th), eng._ptr(gdd), eng._ptr(fe))
        assert rc == -2, (bad, rc)
        assert eng.last_launch() == []
    rc = eng.lib.tsff_sph_table_vjp(eng.h, *eng._sph_args(meta, 0.25), eng._ptr(th), eng._ptr(gdd), None, eng._ptr(fe))
    assert rc == -1


# ---- the fit -----------------------------------------------------------------------------------------------------------
def _case(flm_type, method, n_epochs=N_EPOCHS):
    """(config, all_data, sa): a 128 x 256 ARTS image made from a 'truth' with another Te, another order of f00 and other
    radial functions (Mora-Yahi: another log_10_LT; free: smooth flm_sign and a flm_mag of -3 in both harmonics), and a deck
    that starts elsewhere."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L
    from tsadar_amd.loss_function import LossFunction

    cfg = decks.deck_angular(2, 48, (128, 256), *ROWS)
    cfg["parameters"]["electron"]["fe"] = _fe_cfg(flm_type, 48, 48 if flm_type == "mora-yahi" else 40)
    cfg["other"]["ang_res_unit"] = 1
    cfg["optimizer"].update(method=method, learning_rate=0.002 if method == "adam" else 2e-4, num_epochs=n_epochs, loss_method="l2",
                            save_state=False, save_state_freq=5)
    sa = _angular_sa(cfg)
    rows = ROWS[1] - ROWS[0]
    batch = dict(e_data=np.ones((rows, 256)), i_data=np.zeros((rows, 256)), e_amps=np.ones((rows, 1)), i_amps=np.zeros(rows),
                 noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    truth = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    truth.X[0, L.P_TE] -= 0.3
    truth.sph.normed_m += 0.4
    if flm_type == "mora-yahi":
        truth.sph.flm[(1, 0)]["log_10_LT"] -= 0.2
    else:
        # every harmonic of the truth carries an anisotropy the data can see (10^(-10 sigmoid(-3)) = 0.34 of tanh(sign)): a
        # harmonic the truth leaves at zero has a gradient that cancels by symmetry, and its leaves are rounding noise in both loops
        u = np.linspace(0.0, np.pi, 40)
        for key, shape in (((1, 0), 0.5 * np.sin(u)), ((1, 1), -0.3 * np.sin(2.0 * u))):
            truth.sph.flm[key]["flm_sign"] = shape
            truth.sph.flm[key]["flm_mag"] = np.full(40, -3.0)
    E = LossFunction(copy.deepcopy(cfg), sa, batch).ts_diag(truth, batch)[0]
    e_data = np.ones((128, 256))
    e_data[ROWS[0]:ROWS[1]] = E
    all_data = dict(e_data=e_data, e_amps=np.ones((128, 1)), i_data=np.zeros((128, 256)), i_amps=np.zeros(128),
                    noiseE=np.zeros((128, 256)), noiseI=np.zeros((128, 256)))
    return cfg, all_data, sa


def _leaves(tp):
    return np.concatenate([tp.X[0], tp.sph.get_params()])


_device = functools.partial(util._device, train_generator=True)


@pytest.fixture
def exact_host_vjp(monkeypatch):
    """SphericalHarmonics.vjp -> the twin's autograd: the host loop then takes exact gradients, as the device does."""
    from tsadar_amd import distribution as Dist

    monkeypatch.setattr(Dist.SphericalHarmonics, "vjp", lambda self, fe_bar, step=1e-6: _twin_vjp(self, fe_bar))


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["adam", "rmsprop"])
@pytest.mark.parametrize("flm_type", ["mora-yahi", "arbitrary"])
def test_trained_generator_matches_the_host_loop(torch_mod, exact_host_vjp, flm_type, method):
    from tsadar_amd import _lib as L

    cfg, all_data, sa = _case(flm_type, method)
    host = _host_loop(cfg, all_data, sa)
    best, epoch_loss, loss_fn, info = _device(cfg, all_data, sa)
    n = len(host["losses"])
    assert info["stopped_after"] == host["stopped"]
    print(flm_type, method, "loss:", _rel(info["loss_hist"][:n], host["losses"]), "best leaves:", _rel(_leaves(best), _leaves(host["best"])),
          "final leaves:", _rel(info["leaves"], _leaves(host["final"])))
    assert _rel(info["loss_hist"][:n], host["losses"]) < 1e-9, (info["loss_hist"][:n], host["losses"])
    assert abs(epoch_loss - host["epoch_loss"]) <= 1e-9 * abs(host["epoch_loss"])
    assert host["best"] != {} and best != {}
    assert _rel(_leaves(best), _leaves(host["best"])) < 1e-8
    assert _rel(info["leaves"], _leaves(host["final"])) < 1e-8
    assert host["losses"][-1] < host["losses"][0]
    # the generator moved, and the epoch ran the generator's kernels around the existing ones
    start = cfg["parameters"]["electron"]["fe"]
    from tsadar_amd import distribution as Dist

    assert np.max(np.abs(best.sph.get_params() - Dist.SphericalHarmonics(start).get_params())) > 1e-4
    rec = loss_fn.ts_diag.engine(True).last_launch()
    assert "k_sph_table" in rec and "k_sph_vjp" in rec
    assert rec.index("k_sph_table") == 1 and rec[0].startswith("k_ang_leaves<")


@pytest.mark.gpu
def test_trained_generator_chunks_and_saved_states(torch_mod, exact_host_vjp):
    """The loop in chunks of 7 epochs is bit for bit the loop in one chunk of 30 (uneven chunks: the next test); with save_state
    the saved radial functions are the host loop's at the reference's epochs."""
    cfg, all_data, sa = _case("mora-yahi", "rmsprop")
    cfg["optimizer"].update(save_state=True, save_state_freq=5)
    host = _host_loop(cfg, all_data, sa)
    states = {}
    one = _device(cfg, all_data, sa, chunk=30)
    parts = _device(cfg, all_data, sa, chunk=7, states=states)
    assert np.array_equal(parts[3]["loss_hist"], one[3]["loss_hist"])
    assert np.array_equal(parts[3]["leaves"], one[3]["leaves"])
    assert np.array_equal(_leaves(parts[0]), _leaves(one[0])) and parts[1] == one[1]
    assert sorted(states) == sorted(host["states"]) == [0, 5, 10, 15, 20, 25]
    for i, s in states.items():
        h = host["states"][i]
        for l in h["electron"]["flm"]:
            for m in h["electron"]["flm"][l]:
                a, b = s["electron"]["flm"][l][m], h["electron"]["flm"][l][m]
                assert np.max(np.abs(a - b)) <= 1e-8 * np.max(np.abs(b)), (i, l, m)
        for sp in h:
            for k in h[sp]:
                if k != "flm":
                    assert _rel(s[sp][k], h[sp][k]) < 1e-8, (i, sp, k)


@pytest.mark.gpu
def test_angular_fit_generator_in_uneven_chunks(torch_mod, monkeypatch):
    """Engine.angular_fit with the TSFF_ANG_SPH generator in chunks of 7 + 7 + 7 + 9 epochs against one call of 30, bit for
    bit in what the fit returns (leaves, best, control words, loss history, best history), under Adam (whose bias correction
    depends on epoch0), on the reference's kind of deck (Mora-Yahi).

    What limits bit-identity is not the chunking and not the generator's kernels (tsff_sph_table_vjp is bit-reproducible,
    asserted above) but the 2-D table adjoint that feeds them: it accumulates with LDS atomics (k_form_factor_2d.inc), and two
    calls of form_factor_2d_grad on one input differ in the last bits of about 1450 of 2304 entries.  Measured on an MI355X:
    - free radial functions (one sum per radial node): 30 Adam epochs end 4e-16 .. 8e-13 apart from RUN to run, whole or in
      chunks -- not asserted for them;
    - Mora-Yahi (three sums over the whole table): the optimiser's moments keep those last bits (48 runs of 30 epochs, Adam
      and RMSProp, whole and in chunks: the moments differed from the first run's in every one, by up to 7e-16 relative) and
      are not compared; leaves, best and losses were identical in all 48, because an update that differs by 1e-15 of itself
      is far below the leaves' last bit.
    The same limit holds for a trained Arbitrary2V table; DESIGN.md section 4.7."""
    from tsadar_amd import loops
    from tsadar_amd.engine import Engine

    cfg, all_data, sa = _case("mora-yahi", "adam")
    calls = []
    fit = Engine.angular_fit

    def record(self, leaves, spec, data, n_epochs, **kw):   # the loop's own arguments of its first (and only) chunk
        calls.append((self, self.download(self.dev(leaves)).copy(), dict(spec), data))
        return fit(self, leaves, spec, data, n_epochs, **kw)

    monkeypatch.setattr(Engine, "angular_fit", record)
    loops.angular_loop(copy.deepcopy(cfg), all_data, sa, chunk=30, train_generator=True)
    monkeypatch.setattr(Engine, "angular_fit", fit)
    e, x0, spec, data = calls[0]
    assert spec["generator"] == 3 and x0.size == e.NP + spec["n_gen"]

    def run(chunks):
        x, state, done, hs, bhs = e.dev(x0.copy()), None, 0, [], []
        for k in chunks:
            x, state, h, bh = e.angular_fit(x, spec, data, k, state=state, epoch0=done, best_hist=True)
            hs.append(h)
            bhs.append(bh)
            done += k
        t = e.torch
        return [e.download(v) for v in (x, state[1], state[2].to(t.float64), t.cat(hs), t.cat(bhs))]

    a, b = run([30]), run([7, 7, 7, 9])
    assert a[4].shape == (30, e.NP + spec["n_gen"])
    for name, u, v in zip(("leaves", "best", "ctl", "loss_hist", "best_hist"), a, b):
        assert np.array_equal(u, v, equal_nan=True), name
    assert np.isfinite(a[3]).all() and a[3][-1] < a[3][0]
