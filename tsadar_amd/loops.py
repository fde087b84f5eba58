"""Drop-ins for the reference's fit loops, run on the device: ``_1d_adam_loop_`` (tsadar/inverse/loops.py:59-95) as
``adam_loop``, the default ``_1d_scipy_loop_`` (loops.py:20-56, scipy L-BFGS-B) as ``lbfgs_loop`` and the angular (ARTS)
``angular_optax`` (loops.py:167-275) as ``angular_loop``.

The reference alternates ``LossFunction.vg_loss`` (spectra and gradient to the host) with ``optax.adam`` and
``eqx.apply_updates`` on the host, once per epoch.  ``adam_loop`` enqueues the whole fit at once through
``Engine.adam_fit`` (tsff_adam_fit: packed loss + gradient and one Adam update per step, k_adam.inc) and synchronises once per
chunk.  The steps are those of ``tsadar_amd.tree.Adam`` + ``tree.apply_updates`` bit for bit (see include/tsff.h), and the best
weights are tracked as the reference tracks them: the iterate AFTER the update of the step whose loss was the lowest.

``lm_loop`` has the shape of ``lbfgs_loop`` but is not a drop-in for a loop of the reference: it fits every lineout of the batch
on its own by Levenberg-Marquardt (tsadar_amd.lm, tsff_lm_fit), where the reference's 1-D loops fit the batch jointly.
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional, Tuple

import numpy as np

from . import tree
from .params import ThomsonParams

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8   # optax.adam's defaults (the reference passes the learning rate only)


def _one_d_setup(name: str, config: Dict, loss_fn, previous_weights: Optional[ThomsonParams], batch: Dict):
    """What ``adam_loop`` and ``lbfgs_loop`` share before their first enqueue: the refusals (NotImplementedError, before any
    device work), the weights, their trained part and its slots, and the engine with the batch on the device.
    -> (ts_params, diff, act, eng, X, B, w, db, fe); fe: the constant table of a free-form f_e that is not trained, else None."""
    if getattr(loss_fn, "angular", False) or "angular" in config["other"]["extraoptions"]["spectype"]:
        raise NotImplementedError(f"{name}: angular decks run through the reference's angular loop, not a 1-D loop")
    if getattr(loss_fn, "distributed", False):
        raise NotImplementedError(f"{name}: distributed=True is not built (each step would all-reduce its packed buffer)")
    ts_params = previous_weights if previous_weights is not None else \
        ThomsonParams(config["parameters"], config["optimizer"]["batch_size"], activate=True)
    sm = ts_params.slots
    if sm.fval_active or sm.gen2d_active or getattr(sm, "fval2d_active", False):
        raise NotImplementedError(f"{name}: a trainable free-form distribution function (Arbitrary1V.fval) is not built on the "
                                  "device: its chain rule runs on the host (use vg_loss with a host optimiser)")
    diff, _ = tree.partition(ts_params, tree.get_filter_spec(config["parameters"], ts_params))
    act = [s for _, s in diff.slots]
    eng = loss_fn.ts_diag.engine(ts_params.activate)
    X = ts_params.to_matrix()
    B = X.shape[0]
    w = eng.loss_weights(B, loss_fn.i_norm, loss_fn.e_norm, config["data"]["ion_loss_scale"])
    return ts_params, diff, act, eng, X, B, w, loss_fn._device_batch(eng, batch, B), ts_params.fe_table()


def _report(progress, done: int, loss: float, text: str) -> None:
    """One report to ``progress``: a tqdm-like object (``set_description``) gets ``text``, a callable ``(done, loss)``."""
    if hasattr(progress, "set_description"):
        progress.set_description(text)
    else:
        progress(done, loss)


def adam_loop(config: Dict, loss_fn, previous_weights: Optional[ThomsonParams], batch: Dict, chunk: Optional[int] = None,
              progress=None) -> Tuple[float, ThomsonParams]:
    """``_1d_adam_loop_(config, loss_fn, previous_weights, batch, tbatch)`` -> (best_loss, best_weights).

    ``config["optimizer"]``: ``num_epochs`` steps at ``learning_rate``.  ``previous_weights``: a ThomsonParams to continue from
    (the ``sequential`` option of one_d_loop), else a fresh one of ``batch_size`` lineouts.  ``chunk``: steps per enqueued
    chunk (default: all of them); after each chunk the loop synchronises once and reports to ``progress`` -- a tqdm-like
    object (``set_description``, the reference's ``tbatch``) or a callable ``progress(steps_done, last_loss)``.

    Not built (NotImplementedError): angular decks (the reference runs them through another loop), a trainable free-form f_e
    (Arbitrary1V.fval: its chain rule runs on the host) and ``distributed=True`` loss functions."""
    opt = config["optimizer"]
    ts_params, _, act, eng, X, B, w, db, fe = _one_d_setup("adam_loop", config, loss_fn, previous_weights, batch)
    n_epochs = int(opt["num_epochs"])
    hyper = (float(opt["learning_rate"]), ADAM_B1, ADAM_B2, ADAM_EPS)
    step = max(1, int(chunk)) if chunk else max(1, n_epochs)
    Xd, state, best = eng.dev(X), None, None
    done, last = 0, 1e19
    while done < n_epochs:
        k = min(step, n_epochs - done)
        Xd, state, hist, best = eng.adam_fit(Xd, db, w, act, k, hyper, state=state, best=best, step0=done, fe=fe)
        done += k
        if progress is not None:
            last = float(eng.download(hist[-1:])[0])   # the chunk's one synchronisation
            _report(progress, done, last, f"Epoch {done}, Prev Epoch Loss {last:.2e}")
    out = ts_params.copy()
    if best is None:   # (no epoch: the reference leaves best_weights unbound; here the starting point)
        return 1e16, out
    host = eng.download(best)
    out.X = host[1:].reshape(B, -1).copy()
    return float(host[0]), out


LBFGS_CHUNK = 16   # evaluations per enqueued chunk of lbfgs_loop (at most this many minus one run after the fit has ended)


def lbfgs_loop(config: Dict, loss_fn, previous_weights: Optional[ThomsonParams], batch: Dict, chunk: Optional[int] = None,
               progress=None, info: Optional[Dict] = None) -> Tuple[float, ThomsonParams]:
    """``_1d_scipy_loop_(config, loss_fn, previous_weights, batch)`` -> (res.fun, combine(unravel(res.x), static)).

    scipy's L-BFGS-B with ``maxiter = num_epochs`` and its other defaults (maxcor 10, ftol 2.22e-9, gtol 1e-5, maxfun 15000,
    maxls 20), unbounded on the activated leaves, run on the device by ``Engine.lbfgs_fit`` (tsff_lbfgs_fit, k_lbfgs.inc): the
    iterates are tsadar_amd.lbfgs's bit for bit and scipy's up to rounding.  ``previous_weights``: a ThomsonParams to continue
    from (the ``sequential`` option of one_d_loop), else a fresh one of ``batch_size`` lineouts.  ``chunk``: evaluations per
    enqueued chunk (default 16); after each chunk the loop synchronises once, stops if the fit has ended, and reports to
    ``progress`` -- a tqdm-like object (``set_description``) or a callable ``progress(iterations_done, loss)``.  The loss
    returned is that of the returned iterate (scipy's ``res.fun`` after an abnormal line-search end is the last trial's).
    ``info``: a dict that receives ``Engine.lbfgs_info`` of the end (status, scipy_status, nit, nfev, nskip, f).

    Not built (NotImplementedError, raised before any device work): angular decks, ``distributed=True`` loss functions, a
    trainable free-form f_e (Arbitrary1V.fval), ``grad_method`` other than "AD" and any ``method`` other than l-bfgs-b."""
    opt = config["optimizer"]
    if str(opt.get("method", "l-bfgs-b")).lower() != "l-bfgs-b":
        raise NotImplementedError(f"lbfgs_loop: method {opt.get('method')!r} -- only l-bfgs-b is built on the device")
    if opt.get("grad_method", "AD") != "AD":
        raise NotImplementedError(f"lbfgs_loop: grad_method {opt.get('grad_method')!r} -- only the analytic gradient (AD) is built")
    ts_params, diff, act, eng, X, B, w, db, fe = _one_d_setup("lbfgs_loop", config, loss_fn, previous_weights, batch)
    _, loss_fn.unravel_weights = tree.ravel_pytree(diff)   # (as the reference leaves it)
    from .lbfgs import RUNNING

    opts = (10, 2.220446049250313e-09, 1e-5, int(opt["num_epochs"]), 15000, 20)
    step = max(1, int(chunk)) if chunk else LBFGS_CHUNK
    Xd, state, dinfo = eng.dev(X), None, None
    while True:
        Xd, state, _, dinfo = eng.lbfgs_fit(Xd, db, w, act, step, opts, state=state, f_hist=False, info=dinfo, fe=fe)
        res = eng.lbfgs_info(dinfo, state)   # the chunk's one synchronisation
        if progress is not None:
            _report(progress, res["nit"], res["f"], f"Iteration {res['nit']}, Loss {res['f']:.2e}")
        if res["status"] != RUNNING:
            break
    if info is not None:
        info.update(res)
    out = ts_params.copy()
    out.X = eng.download(Xd).reshape(B, -1).copy()
    return res["f"], out


LM_CHUNK = 8   # evaluations per enqueued chunk of lm_loop (a lineout that has ended costs the later ones of its chunk nothing)


def lm_loop(config: Dict, loss_fn, previous_weights: Optional[ThomsonParams], batch: Dict, chunk: Optional[int] = None,
            progress=None, info: Optional[Dict] = None) -> Tuple[float, ThomsonParams]:
    """An opt-in replacement for ``_1d_scipy_loop_`` with its shape -> (best_loss, best_weights): every lineout of the batch is
    fitted on its own by Levenberg-Marquardt (tsadar_amd.lm; Nielsen's damping on the Gauss-Newton matrix of its loss), run on
    the device by ``Engine.lm_fit`` (tsff_lm_fit, k_lm.inc).  This is not the reference's optimiser: its 1-D loops minimise the
    batch's mean loss as one joint problem, although the lineouts do not couple; here each lineout has its own step length and
    its own stopping point.  A local method: from a start far from the minimum it can end in a side minimum, as any other.

    ``maxiter = num_epochs`` accepted steps and ``maxfun = 2 num_epochs + 10`` evaluations per lineout, tau 1e-3, gtol 1e-8,
    ftol 1e-12, xtol 1e-10, lam_max 1e12.  The loss of lineout b is its own mean loss (the weights of a batch of one), so the
    tolerances do not depend on the batch size.  ``best_loss`` is the batch's mean loss at ``best_weights`` as ``vg_loss``
    returns it there: one evaluation of its loss kernels at the end (the mean of the fit's own f_b is the same quantity from the
    Jacobian sweep's sums, which lie some 1e-11 of it away -- the two value the narrow ion feature by different kernels -- and
    ``progress`` and ``info`` report those).  ``previous_weights``: a ThomsonParams to continue from, else a fresh one of ``batch_size`` lineouts.
    ``chunk``: evaluations per enqueued chunk (default 8); after each chunk the loop synchronises once, stops when every lineout
    has ended, and reports to ``progress`` -- a tqdm-like object (``set_description``) or a callable ``progress(evaluations,
    mean loss)``.  ``info``: a dict that receives ``Engine.lm_info`` of the end (x, f, lam, status, nit, nfev per lineout) and
    ``n_evals``, the evaluations enqueued.

    Not built (NotImplementedError, raised before any device work): ``loss_method`` l1 (its Gauss-Newton matrix vanishes),
    angular decks, ``distributed=True`` loss functions and a trainable free-form f_e (Arbitrary1V.fval)."""
    from . import lm

    opt = config["optimizer"]
    if opt.get("loss_method", "l2") == "l1":
        raise NotImplementedError("lm_loop: loss_method l1 has no curvature, its Gauss-Newton matrix vanishes (use l2, log-cosh or poisson)")
    ts_params, diff, act, eng, X, B, w_batch, db, fe = _one_d_setup("lm_loop", config, loss_fn, previous_weights, batch)
    _, loss_fn.unravel_weights = tree.ravel_pytree(diff)   # (as lbfgs_loop leaves it: vg_loss takes the flat vector)
    w = eng.loss_weights(1, loss_fn.i_norm, loss_fn.e_norm, config["data"]["ion_loss_scale"])
    n_epochs = int(opt["num_epochs"])
    opts = lm.Options(maxiter=n_epochs, maxfun=2 * n_epochs + 10)
    step = max(1, int(chunk)) if chunk else LM_CHUNK
    Xd, state, done = eng.dev(X), None, 0
    while True:
        Xd, state, _, _ = eng.lm_fit(Xd, db, w, act, step, opts, state=state, fe=fe)
        done += step
        res = eng.lm_info(state)   # the chunk's one synchronisation
        loss = float(np.mean(res["f"]))
        if progress is not None:
            _report(progress, done, loss, f"Evaluation {done}, Loss {loss:.2e}")
        if not np.any(res["status"] == lm.RUNNING):
            break
    if info is not None:
        info.update(res, n_evals=done)
    gm = np.zeros(eng.NP, dtype=np.uint8)
    gm[act] = 1
    host = eng.download(eng.loss_grad(Xd, db, w_batch, gm, fe=fe)[0])   # the loss terms of vg_loss's kernels at the returned weights
    out = ts_params.copy()
    out.X = eng.download(Xd).reshape(B, -1).copy()
    return float(np.dot(host, w_batch)), out


class _Generator(NamedTuple):
    """An angular deck's f_e generator as ``angular_loop`` uses it: a row of tsff_angular_fit's table (include/tsff.h)."""
    code: int                                      # L.ANG_*
    spec: Dict                                     # the fields of tsff_angular_spec it adds
    gen_data: Optional[np.ndarray]                 # its constants (``data["gen_data"]`` of Engine.angular_fit)
    tail: np.ndarray = np.zeros(0)                 # its leaves, behind the NP scalars
    write_back: Callable = lambda tp, tail: None   # (ThomsonParams, such a tail): the tail into the weights
    state_extra: Callable = lambda tp: {}          # ThomsonParams -> what ["electron"] of a saved state gains


def _generator(config: Dict, ts_params: ThomsonParams, train_generator: bool) -> Optional[_Generator]:
    """The generator of ``config``'s f_e at the values of ``ts_params``; None: the device builds none for this f_e."""
    from . import _lib as L
    from . import distribution as Dist

    fecfg, sm, gen = config["parameters"]["electron"]["fe"], ts_params.slots, config["parameters"]["general"]
    nvx, dim = int(fecfg["nvx"]), int(fecfg.get("dim", 1))
    if (dim == 1 and not (sm.has_m or sm.fval_active)) or ((sm.fval_active or sm.gen2d_active) and not train_generator):
        return None
    if sm.fval_active:   # a trained Arbitrary1V
        return _Generator(L.ANG_ARB1V, {}, Dist.arb1v_gen_data(nvx), ts_params.fval.ravel(),
                          lambda tp, tail: setattr(tp, "fval", tail.reshape(tp.fval.shape).copy()))
    if dim == 1:
        return _Generator(L.ANG_DLM, {}, np.concatenate([Dist.dlm_table(nvx).ravel(), Dist.M_AXIS]))
    angles = dict(ud_angle=gen["ud"]["angle"], va_angle=gen["Va"]["angle"])
    if sm.fval2d_active:   # a trained Arbitrary2V table
        return _Generator(L.ANG_ARB2V, dict(angles, learn_log=ts_params.learn_log), None, ts_params.fval2d.ravel(),
                          lambda tp, tail: setattr(tp, "fval2d", tail.reshape(tp.fval2d.shape).copy()))
    if sm.gen2d_active:   # a trained SphericalHarmonics
        gen_data, meta = Dist.sph_gen_data(ts_params.sph)
        return _Generator(L.ANG_SPH, dict(angles, **meta), gen_data, ts_params.sph.get_params(), lambda tp, tail: tp.sph.set_params(tail),
                          lambda tp: {"flm": tp.sph.get_unnormed_params()["flm"]})
    # a constant table (SphericalHarmonics or Arbitrary2V not trained), built once on the host
    return _Generator(L.ANG_TABLE2D, angles, np.ascontiguousarray(ts_params()["electron"]["fe"], dtype=np.float64))


ANGULAR_CHUNK = 16   # epochs per enqueued chunk of angular_loop (at most this many minus one run after the early stop)
RMSPROP_DECAY, RMSPROP_EPS = 0.9, 1e-8   # optax.rmsprop's defaults


def angular_loop(config: Dict, all_data: Dict, sa: Dict, chunk: Optional[int] = None, progress=None, states: Optional[Dict] = None,
                 info: Optional[Dict] = None, distributed: bool = False, train_generator: bool = False):
    """``angular_optax(config, all_data, sa)`` -> (best_weights, epoch_loss, loss_fn), run on the device by
    ``Engine.angular_fit`` (tsff_angular_fit, k_angular.inc).

    The same config mutations (``batch_size = 1``, lineout start / end over ``ang_res_unit``), the same ``batch1`` slice of
    ``all_data``, ``LossFunction(config, sa, batch1)`` and ``ThomsonParams(..., num_params=1, batch=False, activate=True)``;
    ``optimizer.method`` "adam" (tree.Adam) or "rmsprop" (tree.RMSProp, optax's defaults), ``num_epochs`` epochs at
    ``learning_rate``.  The early stop is the reference's as written: best_loss starts at 100.0 and best_weights at ``{}``
    (returned as is when no epoch improves); an epoch whose loss is below the best takes the updated iterate as the best; an
    improvement below 1e-6 counts towards the stop (after more than 5), a larger one resets the counters; the branch "stop on
    increase" never runs.  ``epoch_loss`` is the LAST epoch's loss.

    ``chunk``: epochs per enqueued chunk (default 16); after each chunk the loop synchronises once, stops once the fit has
    ended, and reports to ``progress`` -- a tqdm-like object (``set_description``) or a callable ``progress(epochs_done,
    last_loss)``.  ``states``: with ``save_state``, receives ``best_weights.get_unnormed_params()`` at the reference's epochs
    (every ``save_state_freq``-th epoch that does not end the fit; an epoch before any best exists, where the reference would
    fail on ``{}``, is skipped); writing the file and logging stay with the caller.  ``info``: a dict that receives
    ``loss_hist`` (the loss of every epoch run, NaN after the end: the reference's per-epoch "epoch loss" metric),
    ``stopped_after`` (the epoch of the early stop, or None) and ``leaves`` (the final normalised leaves, then fval or the
    generator's parameters).

    ``train_generator=True`` trains two more generators on the device, exactly (``LossFunction.vg_loss`` takes central differences
    for the order of f00 and the Mora-Yahi gradient lengths) and with f_e rebuilt from their parameters every epoch: a trainable
    ``sphericalharmonic`` f_e of ``flm_type`` "mora-yahi" or "arbitrary" (the reference's arts2v deck; k_sph.inc) -- ``best_weights.sph``
    is the best iterate's, each saved state carries its radial functions under ``["electron"]["flm"]`` (the reference's layout) --
    and a trained free-form 1-D f_e (``fe: {dim: 1, type: arbitrary, active: true}``, the reference's Arbitrary1V; k_arb1v.inc) --
    ``best_weights.fval`` is the best iterate's, each saved state's ``["electron"]["f"]`` the f_e of that epoch's best fval.
    ``info["leaves"]`` is then the scalars followed by those parameters.  The default refuses both decks, as before.

    Not built (NotImplementedError, raised before any device work): methods other than adam and rmsprop, multiplexed decks
    (``shotnum`` a list), ``distributed=True``, trainable SphericalHarmonics generators without ``train_generator`` or of
    ``flm_type`` "nn", 1-D decks other than DLM1V and, with ``train_generator``, a trained free-form f_e (a free-form 1-D f_e
    that is not trained stays refused)."""
    from . import _lib as L
    from . import distribution as Dist
    from .loss_function import LossFunction

    opt = config["optimizer"]
    method = opt["method"]
    if method not in ("adam", "rmsprop"):
        raise NotImplementedError(f"angular_loop: method {method!r} -- only adam and rmsprop are built on the device")
    if isinstance(config["data"].get("shotnum"), list):
        raise NotImplementedError("angular_loop: multiplexed decks (shotnum a list) are not built")
    if distributed:
        raise NotImplementedError("angular_loop: distributed=True is not built")
    fecfg = config["parameters"]["electron"]["fe"]
    dim = int(fecfg.get("dim", 1))
    if dim == 2 and "sph" in str(fecfg["type"]).casefold() and fecfg.get("active", False):
        if not train_generator:
            raise NotImplementedError("angular_loop: a trainable SphericalHarmonics generator is not built on the device (use the "
                                      "host loop over LossFunction.vg_loss)")
        flm_type = str(fecfg["params"].get("flm_type", "arbitrary")).casefold()
        if flm_type not in ("mora-yahi", "arbitrary"):
            raise NotImplementedError(f"angular_loop: train_generator with flm_type {flm_type!r} -- only mora-yahi and arbitrary "
                                      "radial functions are built on the device; flm_type nn stays on the host (the loop over "
                                      "LossFunction.vg_loss)")
    arb1v = train_generator and dim == 1 and str(fecfg.get("type", "dlm")).casefold() == "arbitrary"
    if dim == 1 and str(fecfg.get("type", "dlm")).casefold() != "dlm" and not arb1v:
        raise NotImplementedError(f"angular_loop: 1-D f_e of type {fecfg.get('type')!r} -- only DLM1V is built")
    if arb1v and not fecfg.get("active", False):
        raise NotImplementedError("angular_loop: a free-form 1-D f_e that is not trained (a constant table) is not built on the "
                                  "device (use the host loop over LossFunction.vg_loss)")

    # loops.py:197-227, as written
    config["optimizer"]["batch_size"] = 1
    lo = config["data"]["lineouts"]
    lo["start"] = int(lo["start"] / config["other"]["ang_res_unit"])
    lo["end"] = int(lo["end"] / config["other"]["ang_res_unit"])
    a, b = lo["start"], lo["end"]
    batch1 = {"e_data": all_data["e_data"][a:b, :], "e_amps": all_data["e_amps"][a:b, :], "i_data": all_data["i_data"],
              "i_amps": all_data["i_amps"], "noise_e": all_data["noiseE"][a:b, :], "noise_i": all_data["noiseI"][a:b, :]}
    loss_fn = LossFunction(config, sa, batch1)
    ts_params = ThomsonParams(config["parameters"], num_params=1, batch=False, activate=True)
    g = _generator(config, ts_params, train_generator)
    if g is None:
        raise NotImplementedError("angular_loop: this distribution function is not built on the device")
    diff, _ = tree.partition(ts_params, tree.get_filter_spec(config["parameters"], ts_params))
    act = [s for _, s in diff.slots if s >= 0]

    eng = loss_fn.ts_diag.engine(ts_params.activate)
    torch = eng.torch
    diag = loss_fn.ts_diag
    lam_step = diag._ats_prepare(eng, batch1)
    rows, nJ = eng._ats_shape
    wcol = loss_fn._angular_wcol(diag._ats_lam_axis(eng, lam_step), rows)
    nvx = int(fecfg["nvx"])
    vx = Dist.velocity_grid(nvx)
    leaves = np.concatenate([ts_params.X[0], g.tail])
    spec = dict(g.spec, generator=g.code, nv=nvx, active_slots=act, loss_method=L.LOSS_METHODS[opt["loss_method"]], un=loss_fn.e_norm**2,
                dvx=vx[1] - vx[0], lr=float(opt["learning_rate"]))
    spec.update(dict(method=L.ANG_ADAM, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS) if method == "adam" else
                dict(method=L.ANG_RMSPROP, decay=RMSPROP_DECAY, eps=RMSPROP_EPS))
    img = lambda v: eng.dev(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (rows, nJ))))
    data = dict(gen_data=eng.dev(g.gen_data), e_data=img(batch1["e_data"]), noise_e=img(np.atleast_1d(batch1["noise_e"])),
                wcol=eng.dev(wcol), e_amps=eng.dev(np.broadcast_to(np.asarray(batch1["e_amps"], dtype=np.float64).reshape(-1, 1),
                                                                   (rows, 1)).reshape(-1)))

    n_epochs = int(opt["num_epochs"])
    save = bool(opt.get("save_state", False))
    step = max(1, int(chunk)) if chunk else ANGULAR_CHUNK
    x, state, done = eng.dev(leaves), None, 0
    hists, bhs, ended = [], [], False
    while done < n_epochs and not ended:
        k = min(step, n_epochs - done)
        x, state, hist, bh = eng.angular_fit(x, spec, data, k, state=state, epoch0=done, best_hist=save)
        hists.append(hist)
        if save:
            bhs.append(bh)
        done += k
        host = eng.download(torch.cat([state[2][:2].to(torch.float64), hist]))   # the chunk's one synchronisation
        ended = host[0] != 0
        if progress is not None:
            last = float(host[2 + int(host[1]) - (done - k)] if ended else host[-1])   # (an ended fit ended in this chunk)
            _report(progress, done, last, f"Loss {last:.2e}")
    if n_epochs == 0:
        if info is not None:
            info.update(loss_hist=np.zeros(0), stopped_after=None, leaves=leaves)
        return {}, 0.0, loss_fn
    ctl = eng.download(state[2].to(torch.float64))
    hist = eng.download(torch.cat(hists))
    last_epoch = int(ctl[1]) if ctl[0] != 0 else n_epochs - 1
    epoch_loss = float(hist[last_epoch])
    if info is not None:
        info.update(loss_hist=hist, stopped_after=int(ctl[1]) if ctl[0] != 0 else None, leaves=eng.download(x))
    if save and states is not None:
        bh = eng.download(torch.cat(bhs))
        freq = int(opt["save_state_freq"])
        for i in range(last_epoch if ctl[0] != 0 else n_epochs):
            if i % freq == 0 and not np.isnan(bh[i, 0]):
                snap = ts_params.copy()
                snap.X[0] = bh[i, : eng.NP]
                if bh.shape[1] > eng.NP:   # (the generators whose leaves best_hist keeps)
                    g.write_back(snap, bh[i, eng.NP :])
                states[i] = snap.get_unnormed_params()
                states[i]["electron"].update(g.state_extra(snap))
    if ctl[4] == 0:   # (no epoch improved on 100.0: the reference returns the dict it started with)
        return {}, epoch_loss, loss_fn
    best = eng.download(state[1])
    best_weights = ts_params.copy()
    best_weights.X[0] = best[1 : 1 + eng.NP]
    g.write_back(best_weights, best[1 + eng.NP :])
    return best_weights, epoch_loss, loss_fn
