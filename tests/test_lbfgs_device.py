"""tsadar_amd.lbfgs / tsff_lbfgs_fit / Engine.lbfgs_fit / loops.lbfgs_loop: the reference's default 1-D loop
(_1d_scipy_loop_, inverse/loops.py:20-56: scipy L-BFGS-B, bounds=None) run on the device.

CPU: the host restatement against scipy itself (same iteration and evaluation counts, same termination class, the same
iterates up to rounding), its fixed-order reduction, and the drop-in's signature and refusals.
GPU: the device loop against the host restatement driven by Engine.loss_grad_packed, bit for bit (loss per evaluation,
parameters, counts and status), chunked calls, large batches, the drop-in against the reference-shaped scipy loop, the
reference's round-trip protocol, refusals and the launch record."""
import inspect
import types

import numpy as np
import pytest
import scipy.optimize as spopt

import decks
import util


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the host restatement against scipy
# ---------------------------------------------------------------------------------------------------------------------
def _rosen(x):
    return float(spopt.rosen(x)), spopt.rosen_der(x)


def _quadratic():
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.normal(size=(100, 100)))
    A = (Q * np.logspace(0, 3, 100)) @ Q.T   # condition number 1e3
    b = rng.normal(size=100)
    return lambda x: (float(0.5 * x @ A @ x - b @ x), A @ x - b)


# name -> (fg, x0, options, what the run must show).  The quadratic and the 20-D Rosenbrock runs stop at loosened gtol: run to
# scipy's default gtol they part from scipy by rounding on a long path (20-D Rosenbrock: iterates equal to 1e-12 up to about
# iteration 40, then nit 123 / nfev 153 here against scipy's 124 / 154), so equal counts are claimed for these stops only.
PROBLEMS = {
    "quadratic_100": (_quadratic(), np.zeros(100), dict(gtol=1e-2), None),
    "rosenbrock_2": (_rosen, np.array([-1.2, 1.0]), {}, None),
    "rosenbrock_20": (_rosen, np.tile([-1.2, 1.0], 10), dict(gtol=0.5), None),
    "maxiter": (_rosen, np.tile([-1.2, 1.0], 10), dict(maxiter=15), None),
    "restart": (_rosen, np.array([-1.2, 1.0]), dict(maxls=2), "restart"),          # maxls evaluations: memory reset
    "abnormal": (_rosen, np.tile([-1.2, 1.0], 10), dict(maxls=1, maxiter=40), "abnormal"),   # ... then with an empty memory
}


def _drive(fg, x0, **opts):
    """lbfgs.Lbfgs one evaluation at a time (as the device runs it) -> (optimiser, accepted iterates)."""
    from tsadar_amd import lbfgs

    opt = lbfgs.Lbfgs(len(x0), **opts)
    x, its = np.array(x0, dtype=np.float64), []
    while True:
        f, g = fg(x)
        nit = opt.nit
        nxt = opt.step(x, f, g)
        if opt.nit > nit:
            its.append(opt.x.copy())
        if nxt is None:
            return opt, its
        x = nxt


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_host_restatement_matches_scipy(name):
    from tsadar_amd import lbfgs

    fg, x0, opts, shows = PROBLEMS[name]
    ref_its = []
    res = spopt.minimize(fg, x0, jac=True, method="L-BFGS-B", options=opts, callback=lambda xk: ref_its.append(np.copy(xk)))
    x, f, nit, nfev, status = lbfgs.minimize(fg, x0, **opts)
    opt, its = _drive(fg, x0, **opts)
    assert (nit, nfev, status) == (res.nit, res.nfev, res.status), ((nit, nfev, status), (res.nit, res.nfev, res.status, res.message))
    assert (opt.nit, opt.nfev, lbfgs.SCIPY_STATUS[opt.status]) == (nit, nfev, status) and np.array_equal(opt.x, x)
    assert len(its) == len(ref_its) == nit
    for k, (a, b) in enumerate(zip(its[:20], ref_its[:20])):
        assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b)), (k, np.max(np.abs(a - b)))
    assert np.max(np.abs(x - res.x)) <= 1e-6 * max(np.max(np.abs(res.x)), 1.0)
    # scipy's res.fun after an abnormal end is the last trial's f, not f(res.x): compare with the loss of its iterate
    f_ref = res.fun if res.status != 2 else fg(res.x)[0]
    assert abs(f - f_ref) <= 1e-10 * max(abs(f_ref), 1.0), (f, f_ref)
    assert f == fg(x)[0]   # the result is the last accepted iterate and its own loss
    if shows == "restart":
        assert opt.nreset >= 1 and status == 0
    elif shows == "abnormal":
        assert opt.nreset >= 1 and opt.status == lbfgs.ABNORMAL and res.status == 2


def test_fixed_order_reduction():
    from tsadar_amd import lbfgs

    rng = np.random.default_rng(3)
    differs = False
    for n in (1, 5, 511, 513, 1024, 1025, 4096 + 17, 24576, 40000):
        a = rng.normal(size=n) * np.exp(rng.normal(scale=8.0, size=n))
        b = rng.normal(size=n)
        # the documented order, spelled out in plain Python floats: G workgroups of 256 threads, strided partials, the halving
        # tree inside each workgroup, then over the workgroups
        G = lbfgs.blocks(n)
        assert G == min(64, 1 << max(0, (-(-n // 512) - 1).bit_length()))
        NT = 256 * G
        part = [0.0] * NT
        for i in range(n):
            part[i % NT] = part[i % NT] + float(a[i]) * float(b[i])

        def tree(v):
            h = len(v) // 2
            while h >= 1:
                v[:h] = [v[i] + v[i + h] for i in range(h)]
                h //= 2
            return v[0]

        wg = [tree(part[256 * w:256 * (w + 1)]) for w in range(G)]
        assert lbfgs.dot(a, b) == tree(wg), n
        differs |= lbfgs.dot(a, b) != float(np.dot(a, b))
    assert differs, "the fixed order never differed from np.dot: the test inputs do not show that the order is pinned"


def test_lbfgs_loop_has_the_reference_signature():
    from tsadar_amd import loops

    names = list(inspect.signature(loops.lbfgs_loop).parameters)
    # _1d_scipy_loop_(config, loss_fn, previous_weights, batch)
    assert names[:4] == ["config", "loss_fn", "previous_weights", "batch"], names


def _fval_deck():
    cfg = decks.deck_fit()
    cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": 64, "params": {"init_m": 2.0}}
    return cfg


def test_lbfgs_loop_refuses_what_it_does_not_build():
    """Every refusal comes before any device work: the stub loss functions have no engine to reach."""
    from tsadar_amd import ThomsonParams, loops

    stub = types.SimpleNamespace(angular=False, distributed=False)
    with pytest.raises(NotImplementedError, match="angular"):
        loops.lbfgs_loop(decks.deck_angular(), types.SimpleNamespace(angular=True, distributed=False), None, {})
    with pytest.raises(NotImplementedError, match="distributed"):
        loops.lbfgs_loop(decks.deck_fit(), types.SimpleNamespace(angular=False, distributed=True), None, {})
    for method in ("adam", "L-BFGS", "bfgs"):
        cfg = decks.deck_fit()
        cfg["optimizer"]["method"] = method
        with pytest.raises(NotImplementedError, match="method"):
            loops.lbfgs_loop(cfg, stub, None, {})
    cfg = decks.deck_fit()
    cfg["optimizer"]["grad_method"] = "FD"
    with pytest.raises(NotImplementedError, match="grad_method"):
        loops.lbfgs_loop(cfg, stub, None, {})
    cfg = _fval_deck()
    tp = ThomsonParams(cfg["parameters"], 2, batch=True, activate=True)
    with pytest.raises(NotImplementedError, match="free-form"):
        loops.lbfgs_loop(cfg, stub, tp, {})
    # any letter case of l-bfgs-b passes the method check (and then needs the loss function's engine)
    cfg = decks.deck_fit()
    cfg["optimizer"]["method"] = "L-BFGS-B"
    with pytest.raises(AttributeError):
        loops.lbfgs_loop(cfg, stub, None, {})


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch


def _setup(deck, B, seed=5, tile_from=None):
    from test_adam_device import _setup as adam_setup

    return adam_setup(deck, B, seed=seed, tile_from=tile_from)


OPTS = (10, 2.220446049250313e-09, 1e-5, 15000, 15000, 20)


def _host_loop(eng, X0, db, w, act, n_evals, opts=OPTS):
    """Engine.loss_grad_packed + lbfgs.Lbfgs, one evaluation at a time -> dict of what the device loop returns."""
    from tsadar_amd import lbfgs

    B, P = X0.shape[0], len(act)
    gm = np.zeros(eng.NP, dtype=np.uint8)
    gm[act] = 1
    maxcor, ftol, gtol, maxiter, maxfun, maxls = opts
    opt = lbfgs.Lbfgs(P * B, int(maxcor), ftol, gtol, int(maxiter), int(maxfun), int(maxls))
    X = X0.copy()
    hist = []
    for _ in range(n_evals):
        packed, _, _ = eng.loss_grad_packed(X, db, w, gm, act)
        host = eng.download(packed)
        f = (w[0] * host[0] + w[1] * host[1]) + w[2] * host[2]
        hist.append(f)
        nxt = opt.step(X[:, act].T.ravel(), f, host[3:])
        x = opt.x if nxt is None else nxt
        X[:, act] = x.reshape(P, B).T
        if nxt is None:
            break
    return dict(hist=np.array(hist), X=X, status=opt.status, nit=opt.nit, nfev=opt.nfev, nskip=opt.nskip, f=opt.f,
                nreset=opt.nreset)


def _device(eng, out, n_host):
    X, state, hist, info = out
    d = eng.lbfgs_info(info, state)
    h = hist.cpu().numpy()
    return dict(hist=h[:n_host], tail=h[n_host:], X=X.cpu().numpy(), status=d["status"], nit=d["nit"], nfev=d["nfev"],
                nskip=d["nskip"], f=d["f"])


def _assert_bitwise(dev, host):
    for k in ("status", "nit", "nfev", "nskip"):
        assert dev[k] == host[k], (k, dev[k], host[k])
    for k in ("hist", "X", "f"):
        a, b = np.asarray(dev[k]), np.asarray(host[k])
        assert a.shape == b.shape and np.array_equal(a, b), (k, np.max(np.abs(a - b)) if a.shape == b.shape else (a.shape, b.shape))


@pytest.mark.gpu
@pytest.mark.parametrize("deck", ["default", "m", "ions2", "ions3_tied", "ppp5"])
def test_device_lbfgs_matches_host_loop_bitwise(deck):
    torch = _torch()
    from test_adam_device import DECKS
    from tsadar_amd import lbfgs

    B, n = 4, 48
    cfg, eng, X0, db, w, act = _setup(DECKS[deck], B)
    host = _host_loop(eng, X0, db, w, act, n)
    dev = _device(eng, eng.lbfgs_fit(X0, db, w, act, n, OPTS), len(host["hist"]))
    torch.cuda.synchronize()
    assert host["nit"] >= 5 and host["f"] < host["hist"][0], host   # (the fit does something)
    _assert_bitwise(dev, host)
    if host["status"] != lbfgs.RUNNING:   # evaluations after the end: reported as NaN, nothing else changes
        assert np.all(np.isnan(dev["tail"]))


# opts that drive the device through the branches the ordinary path does not reach; name -> (opts, status the host must end in)
BRANCHES = {
    "maxls_restart": ((10, 2.220446049250313e-09, 1e-5, 15000, 15000, 2), None),        # line searches cut at 2: memory resets
    "abnormal": ((10, 2.220446049250313e-09, 1e-5, 15000, 15000, 1), "ABNORMAL"),       # ... at 1, up to the abnormal end
    "maxiter": ((10, 2.220446049250313e-09, 1e-5, 4, 15000, 20), "STOP_ITER"),
    "maxfun": ((10, 2.220446049250313e-09, 1e-5, 15000, 6, 20), "STOP_FUN"),
    "maxcor1": ((1, 2.220446049250313e-09, 1e-5, 15000, 15000, 20), None),              # a ring of one pair
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(BRANCHES))
def test_device_lbfgs_branches_match_host_bitwise(case):
    torch = _torch()
    from tsadar_amd import lbfgs

    opts, want = BRANCHES[case]
    B, n = 4, 60
    cfg, eng, X0, db, w, act = _setup({}, B)
    host = _host_loop(eng, X0, db, w, act, n, opts)
    dev = _device(eng, eng.lbfgs_fit(X0, db, w, act, n, opts), len(host["hist"]))
    torch.cuda.synchronize()
    if want is not None:
        assert host["status"] == getattr(lbfgs, want), host
    if case == "maxls_restart":
        assert host["nreset"] >= 1, host
    if case == "abnormal":   # the result is the last accepted iterate, restored on the device
        assert host["nit"] >= 1
    _assert_bitwise(dev, host)


@pytest.mark.gpu
def test_device_lbfgs_chunks_equal_one_call():
    torch = _torch()
    B, n = 4, 21
    cfg, eng, X0, db, w, act = _setup({}, B)
    X1, s1, h1, i1 = eng.lbfgs_fit(X0, db, w, act, n, OPTS)
    one = (X1.cpu().numpy(), s1.cpu().numpy(), h1.cpu().numpy(), i1.cpu().numpy())
    Xd, state, info, hists = eng.dev(X0), None, None, []
    for k in (1, 7, n - 8):
        Xd, state, hist, info = eng.lbfgs_fit(Xd, db, w, act, k, OPTS, state=state, info=info)
        hists.append(hist.cpu().numpy())
    torch.cuda.synchronize()
    chunks = (Xd.cpu().numpy(), state.cpu().numpy(), np.concatenate(hists), info.cpu().numpy())
    for a, b in zip(chunks, one):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [256, 4096])
def test_device_lbfgs_large_batch(B):
    torch = _torch()
    cfg, eng, X0, db, w, act = _setup({}, B, tile_from=16)
    host = _host_loop(eng, X0, db, w, act, 10)
    dev = _device(eng, eng.lbfgs_fit(X0, db, w, act, 10, OPTS), len(host["hist"]))
    torch.cuda.synchronize()
    _assert_bitwise(dev, host)


def _ref_scipy_loop(cfg, loss_fn, previous_weights, batch):
    """_1d_scipy_loop_'s body (loops.py:31-55) over vg_loss in the l-bfgs-b convention; also f at every iteration."""
    from tsadar_amd import ThomsonParams, tree

    ts_params = previous_weights if previous_weights is not None else \
        ThomsonParams(cfg["parameters"], cfg["optimizer"]["batch_size"], activate=True)
    diff, static = tree.partition(ts_params, tree.get_filter_spec(cfg["parameters"], ts_params))
    x0, loss_fn.unravel_weights = tree.ravel_pytree(diff)
    fs = []
    res = spopt.minimize(loss_fn.vg_loss, x0, args=(static, batch), method="L-BFGS-B", jac=True, bounds=None,
                         options={"maxiter": cfg["optimizer"]["num_epochs"]},
                         callback=lambda intermediate_result: fs.append(float(intermediate_result.fun)))
    return res, tree.combine(loss_fn.unravel_weights(res["x"]), static), fs


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.gpu
def test_lbfgs_loop_drop_in():
    _torch()
    from tsadar_amd import ThomsonParams, loops
    from tsadar_amd.loss_function import LossFunction

    B = 2
    cfg = decks.deck_fit(active=("Te", "ne", "lam", "amp1"))
    cfg["optimizer"].update(method="l-bfgs-b", num_epochs=200, batch_size=B)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=17)   # synthetic data from known parameters (plus 1 % noise)
    loss_fn = LossFunction(cfg, sa, batch)
    # start near the truth, so that the fit converges to its one minimum there
    start = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    act = [s for _, s in start.slots.active_leaves]
    start.X = util.normed_to_matrix(util.random_lineouts(cfg, B, seed=17 + 1000), 1)
    start.X[:, act] += 0.05
    res, ref_w, ref_fs = _ref_scipy_loop(cfg, loss_fn, start, batch)
    seen, info = {}, {}
    got, got_w = loops.lbfgs_loop(cfg, loss_fn, start, batch, chunk=1, progress=lambda k, v: seen.setdefault(k, v), info=info)
    assert isinstance(got_w, ThomsonParams)
    assert res.status == 0 and info["scipy_status"] == res.status, (res.message, info)
    # vg_loss sums the three loss terms with np.dot, the device as (w0 S0 + w1 S1) + w2 S2: an ulp apart, which the line
    # search's cubic interpolation (differences of nearly equal f) can amplify until the two paths part (seen on a deck started
    # far from its truth: 1e-10 over the first three iterations, 8.5e-7 at the sixth).  When both see the same f, the host
    # restatement follows scipy to 1e-9 in x over 20 iterations (test_host_restatement_matches_scipy).
    for k in range(1, 11):
        if k <= len(ref_fs):
            assert _rel(seen[k], ref_fs[k - 1]) <= 1e-10, (k, seen[k], ref_fs[k - 1])
    assert _rel(got, res.fun) <= 1e-8, (got, res.fun)
    assert np.max(np.abs(got_w.X - ref_w.X)) <= 1e-4 * np.max(np.abs(ref_w.X))
    # previous_weights continues from a ThomsonParams (one_d_loop's sequential option), with a fresh optimiser, as there
    cfg["optimizer"]["num_epochs"] = 5
    res2, ref2_w, _ = _ref_scipy_loop(cfg, loss_fn, ref_w, batch)
    got2, got2_w = loops.lbfgs_loop(cfg, loss_fn, ref_w, batch)
    assert _rel(got2, res2.fun) <= 1e-8, (got2, res2.fun)


@pytest.mark.gpu
def test_lbfgs_loop_round_trip_like_reference():
    """The reference's tests/test_inverse/test_1d_random.py protocol as test_gpu_parity.test_inverse_round_trip_like_reference
    sets it up (seed 42, DLM f_e, five points per pixel, six leaves), refitted through lbfgs_loop."""
    _torch()
    from tsadar_amd import ThomsonParams, loops
    from tsadar_amd.loss_function import LossFunction

    def perturb(rng, P):
        P["electron"]["fe"]["params"]["m"]["val"] = float(rng.uniform(2.0, 3.5))
        P["electron"]["Te"]["val"] = float(rng.uniform(0.5, 1.5))
        P["electron"]["ne"]["val"] = float(rng.uniform(0.1, 0.7))
        P["general"]["amp1"]["val"] = float(rng.uniform(0.5, 2.5))
        P["general"]["amp2"]["val"] = float(rng.uniform(0.5, 2.5))
        P["general"]["lam"]["val"] = float(rng.uniform(523, 527))

    cfg = decks.deck_1d()
    ext = cfg["other"]["extraoptions"]
    ext["fit_EPWb"], ext["fit_EPWr"], ext["fit_IAW"] = True, False, False
    cfg["data"]["fit_rng"].update(blue_min=0.0, blue_max=1e4)
    cfg["optimizer"].update(y_norm=False, batch_size=1, method="l-bfgs-b", num_epochs=15000)   # scipy's default maxiter
    dummy = dict(i_data=np.array([1]), e_data=np.array([1]), noise_e=np.array([0]), noise_i=np.array([0]),
                 e_amps=np.array([1]), i_amps=np.array([1]))
    rng = np.random.default_rng(42)
    perturb(rng, cfg["parameters"])
    gt = ThomsonParams(cfg["parameters"], num_params=1, batch=True, activate=True)
    lf = LossFunction(cfg, util.P9, dummy)
    ThryE, _, _, _ = lf.ts_diag(gt, dummy)
    batch = dict(dummy, e_data=ThryE, i_data=np.zeros((1, 1024)))
    perturb(rng, cfg["parameters"])
    fit = ThomsonParams(cfg["parameters"], num_params=1, batch=True, activate=True)
    assert len(fit.slots.active_leaves) == 6
    loss, got = loops.lbfgs_loop(cfg, lf, fit, batch)
    learned, truth = got.get_unnormed_params(), gt.get_unnormed_params()
    for sp, k in (("electron", "Te"), ("electron", "ne"), ("electron", "m"), ("general", "amp1"), ("general", "amp2"), ("general", "lam")):
        np.testing.assert_allclose(learned[sp][k], truth[sp][k], atol=0, rtol=0.1, err_msg=f"{sp}.{k} (loss {loss:.3e})")


@pytest.mark.gpu
def test_device_lbfgs_refusals_and_launch_record():
    import ctypes as C

    torch = _torch()
    from tsadar_amd import _lib as L

    B = 4
    cfg, eng, X0, db, w, act = _setup({}, B)
    NP, P = eng.NP, len(act)
    X = eng.dev(X0)
    need = C.c_int64(0)
    assert eng.lib.tsff_lbfgs_state_size(B, P, 10, C.byref(need)) == 0 and need.value > 20 * P * B
    assert eng.lib.tsff_lbfgs_state_size(B, P, 65, C.byref(need)) == -1
    assert eng.lib.tsff_lbfgs_state_size(B, P, 10, C.byref(need)) == 0
    state = torch.zeros(need.value, dtype=torch.float64, device=eng.device)
    hist = torch.zeros(3, dtype=torch.float64, device=eng.device)
    info = torch.zeros(4, dtype=torch.int32, device=eng.device)
    p = eng._ptr
    wa = np.ascontiguousarray(w, dtype=np.float64)

    def call(slots, n_evals=3, st=state, n_state=None, opts=OPTS):
        a = np.ascontiguousarray(slots, dtype=np.int32)
        o = np.ascontiguousarray(opts, dtype=np.float64)
        eng._sync_stream()
        return eng.lib.tsff_lbfgs_fit(eng.h, p(X), None, p(db["e_data"]), p(db["i_data"]), p(db["e_amps"]), p(db["i_amps"]),
                                      p(db["noise_e"]), p(db["noise_i"]), B, wa.ctypes.data_as(L.c_double_p),
                                      a.ctypes.data_as(C.POINTER(C.c_int32)), int(a.size), n_evals, o.ctypes.data_as(L.c_double_p),
                                      p(st), need.value if n_state is None else n_state, p(hist), p(info))

    X_before = X.cpu().numpy().copy()
    refusals = [
        ("slot out of range", lambda: call(act + [NP]), -1),
        ("repeated slot", lambda: call(act + act[:1]), -1),
        ("A slot", lambda: call(act + [L.P_ION0 + L.ION_A]), -3),
        ("m without DLM", lambda: call(act + [L.P_M]), -2),
        ("n_evals < 0", lambda: call(act, n_evals=-1), -1),
        ("null state", lambda: call(act, st=None), -1),
        ("state too small", lambda: call(act, n_state=need.value - 1), -1),
        ("maxcor 0", lambda: call(act, opts=(0,) + OPTS[1:]), -1),
        ("maxls 0", lambda: call(act, opts=OPTS[:5] + (0,)), -1),
    ]
    assert eng.fe_mode != L.FE_DLM
    for what, fn, code in refusals:
        rc = fn()
        assert rc == code, (what, rc, eng.lib.tsff_last_error(eng.h))
        assert eng.last_launch() == [], (what, eng.last_launch())
    assert call(act, n_evals=0) == 0 and eng.last_launch() == []
    torch.cuda.synchronize()
    assert np.array_equal(X.cpu().numpy(), X_before) and not state.abs().max().item()   # nothing ran
    # the launch record: the packed evaluation's kernels, then k_lbfgs_step, per evaluation
    gm = np.zeros(NP, dtype=np.uint8)
    gm[act] = 1
    eng.loss_grad_packed(X0, db, w, gm, act)
    step = eng.last_launch()
    assert step and "k_lbfgs_step" not in step
    assert call(act, n_evals=3) == 0
    passes = 2 * OPTS[0] + 6   # launches of k_lbfgs_step per evaluation
    assert eng.last_launch() == (step + ["k_lbfgs_step"] * passes) * 3, eng.last_launch()
    torch.cuda.synchronize()
