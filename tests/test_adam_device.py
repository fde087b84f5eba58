"""tsff_adam_fit / Engine.adam_fit / loops.adam_loop: the reference's 1-D Adam loop (_1d_adam_loop_, inverse/loops.py:59-95)
run on the device, against the host loop it replaces.

The host loop of the bitwise tests is Engine.loss_grad_packed (the l-bfgs-b convention: no spectra) followed by tree.Adam's
update and tree.apply_updates in NumPy, with the loss (w0 S0 + w1 S1) + w2 S2 of the packed sums.  The device loop runs the
same kernels plus k_adam_step, whose arithmetic is the host's operation for operation, so the two agree bit for bit: loss
history, final parameters, the optimiser state and the best loss and parameters."""
import inspect
import types

import numpy as np
import pytest

import decks
import util

LR = 0.02
HYPER = (LR, 0.9, 0.999, 1e-8)
ACTIVE = ("Te", "ne", "Ti", "Va", "lam", "amp1")

# the decks of the bitwise test: the default one-sweep kernel, the DLM order as a leaf (tables rebuilt every step), two and
# three ion species (ion-3's Ti tied to ion-1's), five points per pixel (k_spectrum_rows)
DECKS = {
    "default": dict(),
    "m": dict(active=ACTIVE + ("m",), m=3.0),
    "ions2": dict(n_ion=2),
    "ions3_tied": dict(n_ion=3, active=ACTIVE + ("Ti_same_3",)),
    "ppp5": dict(points_per_pixel=5),
}


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the module and its refusals (they come before any device work)
# ---------------------------------------------------------------------------------------------------------------------
def test_adam_loop_has_the_reference_signature():
    from tsadar_amd import loops

    names = list(inspect.signature(loops.adam_loop).parameters)
    # _1d_adam_loop_(config, loss_fn, previous_weights, batch, tbatch): the progress bar becomes an optional keyword
    assert names[:4] == ["config", "loss_fn", "previous_weights", "batch"], names
    assert set(names[4:]) == {"chunk", "progress"}, names


def _fval_deck():
    cfg = decks.deck_fit()
    cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": 64, "params": {"init_m": 2.0}}
    return cfg


def test_adam_loop_refuses_what_it_does_not_build():
    from tsadar_amd import ThomsonParams, loops

    stub = types.SimpleNamespace(angular=False, distributed=False)
    with pytest.raises(NotImplementedError, match="angular"):
        loops.adam_loop(decks.deck_angular(), types.SimpleNamespace(angular=True, distributed=False), None, {})
    with pytest.raises(NotImplementedError, match="distributed"):
        loops.adam_loop(decks.deck_fit(), types.SimpleNamespace(angular=False, distributed=True), None, {})
    cfg = _fval_deck()
    tp = ThomsonParams(cfg["parameters"], 2, batch=True, activate=True)
    with pytest.raises(NotImplementedError, match="free-form"):
        loops.adam_loop(cfg, stub, tp, {})


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


def _setup(deck, B, seed=5, tile_from=None):
    """-> (cfg, engine, X0 [B, NP], device batch, weights, active slots).  tile_from: the synthetic data of that many lineouts
    repeated to B (the oracle that makes them is slow at thousands of lineouts); every lineout starts at its own point."""
    from oracle import tsadar_oracle as orc
    from tsadar_amd import ThomsonParams
    from tsadar_amd.engine import Engine

    cfg = decks.deck_fit(**deck)
    nb = tile_from or B
    sa = util.sa_fit(B)
    small = util.synthetic_batch(cfg, util.sa_fit(nb), nb, seed=seed)
    rep = lambda a: np.tile(a, (B // nb,) + (1,) * (np.ndim(a) - 1))
    batch = {k: rep(v) for k, v in small.items()}
    eng = Engine(cfg, sa)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    act = [s for _, s in tp.slots.active_leaves]
    X0 = tp.to_matrix().copy()
    rng = np.random.default_rng(seed)
    X0[:, act] += rng.normal(0.0, 0.05, (B, len(act)))
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    w = eng.loss_weights(B, i_norm, e_norm, cfg["data"]["ion_loss_scale"])
    db = {k: (eng._vec(batch[k], B) if k.endswith("amps") else eng._mat(batch[k], B)) for k in batch}
    return cfg, eng, X0, db, w, act


def _host_loop(eng, X0, db, w, act, n):
    """loss_grad_packed + tree.Adam / tree.apply_updates in NumPy: -> dict of the quantities the device loop returns."""
    from tsadar_amd import tree

    B, P = X0.shape[0], len(act)
    gm = np.zeros(eng.NP, dtype=np.uint8)
    gm[act] = 1
    slots = [(str(s), s) for s in act]
    X = X0.copy()
    opt = tree.Adam(LR)
    diff = tree.DiffParams(slots, [X[:, s].copy() for s in act])
    state = opt.init(diff)
    hist, best_loss, best_X = [], 1e16, X0.copy()
    for _ in range(n):
        packed, _, _ = eng.loss_grad_packed(X, db, w, gm, act)
        host = eng.download(packed)
        L = (w[0] * host[0] + w[1] * host[1]) + w[2] * host[2]
        g = host[3:].reshape(P, B)
        updates, state = opt.update(tree.DiffParams(slots, [g[k].copy() for k in range(P)]), state)
        diff = tree.apply_updates(diff, updates)
        for k, s in enumerate(act):
            X[:, s] = diff.values[k]
        hist.append(L)
        if L < best_loss:
            best_loss, best_X = L, X.copy()
    mu = np.stack(state[1].values)
    nu = np.stack(state[2].values)
    return dict(hist=np.array(hist), X=X, mu=mu, nu=nu, best_loss=best_loss, best_X=best_X)


def _device(out, B, NP):
    X, state, hist, best = (t.cpu().numpy() for t in out)
    return dict(hist=hist, X=X.reshape(B, NP), mu=state[0], nu=state[1], best_loss=best[0], best_X=best[1:].reshape(B, NP))


def _assert_bitwise(dev, host):
    for k in ("hist", "X", "mu", "nu", "best_loss", "best_X"):
        a, b = np.asarray(dev[k]), np.asarray(host[k])
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.max(np.abs(a - b)) if a.shape == b.shape else (a.shape, b.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("deck", list(DECKS))
def test_device_adam_matches_host_loop_bitwise(deck):
    torch = _torch()
    B, n = 4, 30
    cfg, eng, X0, db, w, act = _setup(DECKS[deck], B)
    host = _host_loop(eng, X0, db, w, act, n)
    dev = _device(eng.adam_fit(X0, db, w, act, n, HYPER), B, eng.NP)
    torch.cuda.synchronize()
    assert host["hist"][-1] < host["hist"][0], host["hist"]   # (the fit does something)
    _assert_bitwise(dev, host)


@pytest.mark.gpu
def test_device_adam_chunks_equal_one_call():
    torch = _torch()
    B = 4
    cfg, eng, X0, db, w, act = _setup({}, B)
    one = _device(eng.adam_fit(X0, db, w, act, 30, HYPER), B, eng.NP)
    Xd, state, best, hists = eng.dev(X0), None, None, []
    for c in range(3):
        Xd, state, hist, best = eng.adam_fit(Xd, db, w, act, 10, HYPER, state=state, best=best, step0=10 * c)
        hists.append(hist.cpu().numpy())
    torch.cuda.synchronize()
    chunks = _device((Xd, state, torch.from_numpy(np.concatenate(hists)), best), B, eng.NP)
    _assert_bitwise(chunks, one)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [256, 4096])
def test_device_adam_large_batch(B):
    torch = _torch()
    cfg, eng, X0, db, w, act = _setup({}, B, tile_from=16)
    host = _host_loop(eng, X0, db, w, act, 5)
    dev = _device(eng.adam_fit(X0, db, w, act, 5, HYPER), B, eng.NP)
    torch.cuda.synchronize()
    _assert_bitwise(dev, host)


def _ref_adam_loop(cfg, loss_fn, previous_weights, batch):
    """_1d_adam_loop_'s body (loops.py:74-93) over vg_loss in the adam convention and tree.Adam; also every loss and iterate."""
    from tsadar_amd import ThomsonParams, tree

    opt = tree.Adam(cfg["optimizer"]["learning_rate"])
    ts_params = previous_weights if previous_weights is not None else \
        ThomsonParams(cfg["parameters"], cfg["optimizer"]["batch_size"], activate=True)
    diff, static = tree.partition(ts_params, tree.get_filter_spec(cfg["parameters"], ts_params))
    state = opt.init(diff)
    best_loss, best_weights, losses, iterates = 1e16, None, [], []
    for _ in range(cfg["optimizer"]["num_epochs"]):
        (epoch_loss, aux), grad = loss_fn.vg_loss(diff, static, batch)
        updates, state = opt.update(grad, state)
        diff = tree.apply_updates(diff, updates)
        if epoch_loss < best_loss:
            best_loss = epoch_loss
            best_weights = tree.combine(diff, static)
        losses.append(epoch_loss)
        iterates.append(tree.combine(diff, static))
    return best_loss, best_weights, losses, iterates


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.gpu
def test_adam_loop_drop_in():
    _torch()
    from tsadar_amd import ThomsonParams, loops
    from tsadar_amd.loss_function import LossFunction

    B = 4
    cfg = decks.deck_fit()
    cfg["optimizer"].update(method="adam", learning_rate=LR, num_epochs=30, batch_size=B)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=17)
    loss_fn = LossFunction(cfg, sa, batch)
    ref_loss, ref_w, losses, iterates = _ref_adam_loop(cfg, loss_fn, None, batch)
    seen = []
    best_loss, best_w = loops.adam_loop(cfg, loss_fn, None, batch, chunk=10, progress=lambda k, v: seen.append((k, v)))
    assert isinstance(best_w, ThomsonParams)
    assert abs(best_loss - ref_loss) <= 1e-12 * abs(ref_loss), (best_loss, ref_loss)
    assert _rel(best_w.X, ref_w.X) <= 1e-12, _rel(best_w.X, ref_w.X)
    # the best weights are the iterate AFTER the update of the arg-min step (the reference's quirk), not the one it measured
    i = int(np.argmin(losses))
    assert _rel(best_w.X, iterates[i].X) <= 1e-12
    before = iterates[i - 1].X if i > 0 else ThomsonParams(cfg["parameters"], B, batch=True, activate=True).X
    assert _rel(best_w.X, before) > 1e-9
    # one report per chunk, with the chunk's last loss
    assert [k for k, _ in seen] == [10, 20, 30]
    for k, v in seen:
        assert abs(v - losses[k - 1]) <= 1e-12 * abs(losses[k - 1]), (k, v, losses[k - 1])
    # previous_weights resumes from a ThomsonParams (one_d_loop's sequential option); a fresh optimiser state, as there
    cfg["optimizer"]["num_epochs"] = 10
    ref2, ref2_w, _, _ = _ref_adam_loop(cfg, loss_fn, ref_w, batch)
    got2, got2_w = loops.adam_loop(cfg, loss_fn, best_w, batch)
    assert ref2 < ref_loss
    assert abs(got2 - ref2) <= 1e-12 * abs(ref2), (got2, ref2)
    assert _rel(got2_w.X, ref2_w.X) <= 1e-12


@pytest.mark.gpu
def test_device_adam_refusals():
    import ctypes as C

    torch = _torch()
    from tsadar_amd import _lib as L
    from tsadar_amd import loops
    from tsadar_amd.loss_function import LossFunction

    B = 4
    cfg, eng, X0, db, w, act = _setup({}, B)
    NP, P = eng.NP, len(act)
    X = eng.dev(X0)
    state = torch.zeros((2, P, B), dtype=torch.float64, device=eng.device)
    best = torch.cat([torch.full((1,), 1e16, dtype=torch.float64, device=eng.device), X.reshape(-1)])
    hist = torch.zeros(3, dtype=torch.float64, device=eng.device)
    p = eng._ptr
    wa = np.ascontiguousarray(w, dtype=np.float64)
    hy = np.ascontiguousarray(HYPER, dtype=np.float64)

    def call(slots, n_steps=3, st=state, bs=best):
        a = np.ascontiguousarray(slots, dtype=np.int32)
        eng._sync_stream()
        return eng.lib.tsff_adam_fit(eng.h, p(X), None, p(db["e_data"]), p(db["i_data"]), p(db["e_amps"]), p(db["i_amps"]),
                                     p(db["noise_e"]), p(db["noise_i"]), B, wa.ctypes.data_as(L.c_double_p),
                                     a.ctypes.data_as(C.POINTER(C.c_int32)), int(a.size), n_steps, 0, hy.ctypes.data_as(L.c_double_p),
                                     p(st), p(hist), p(bs))

    X_before = X.cpu().numpy().copy()
    refusals = [
        ("slot out of range", lambda: call(act + [NP]), -1),
        ("repeated slot", lambda: call(act + act[:1]), -1),
        ("A slot", lambda: call(act + [L.P_ION0 + L.ION_A]), -3),
        ("m without DLM", lambda: call(act + [L.P_M]), -2),
        ("n_steps < 0", lambda: call(act, n_steps=-1), -1),
        ("null state", lambda: call(act, st=None), -1),
        ("null best", lambda: call(act, bs=None), -1),
    ]
    assert eng.fe_mode != L.FE_DLM
    for what, fn, code in refusals:
        rc = fn()
        assert rc == code, (what, rc, eng.lib.tsff_last_error(eng.h))
        assert eng.last_launch() == [], (what, eng.last_launch())
    assert call(act, n_steps=0) == 0 and eng.last_launch() == []
    torch.cuda.synchronize()
    assert np.array_equal(X.cpu().numpy(), X_before)   # nothing ran
    # the Python layer: angular, trainable free-form f_e and distributed loss functions
    cfg["optimizer"].update(method="adam", learning_rate=LR, num_epochs=2, batch_size=B)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=3)
    lf = LossFunction(cfg, sa, batch)
    lf.distributed = True
    with pytest.raises(NotImplementedError, match="distributed"):
        loops.adam_loop(cfg, lf, None, batch)
    lf.distributed = False
    with pytest.raises(NotImplementedError, match="angular"):
        loops.adam_loop(decks.deck_angular(), lf, None, batch)
    cfg_f = _fval_deck()
    from tsadar_amd import ThomsonParams

    with pytest.raises(NotImplementedError, match="free-form"):
        loops.adam_loop(cfg_f, lf, ThomsonParams(cfg_f["parameters"], B, batch=True, activate=True), batch)


@pytest.mark.gpu
def test_device_adam_launch_record():
    _torch()
    B = 4
    cfg, eng, X0, db, w, act = _setup({}, B)
    gm = np.zeros(eng.NP, dtype=np.uint8)
    gm[act] = 1
    eng.loss_grad_packed(X0, db, w, gm, act)
    step = eng.last_launch()
    assert step and "k_adam_step" not in step
    eng.adam_fit(X0, db, w, act, 3, HYPER)
    assert eng.last_launch() == (step + ["k_adam_step"]) * 3, eng.last_launch()
