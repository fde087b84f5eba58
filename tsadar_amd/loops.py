"""Drop-ins for the reference's 1-D loops, run on the device: ``_1d_adam_loop_`` (tsadar/inverse/loops.py:59-95) as
``adam_loop`` and the default ``_1d_scipy_loop_`` (loops.py:20-56, scipy L-BFGS-B) as ``lbfgs_loop``.

The reference alternates ``LossFunction.vg_loss`` (spectra and gradient to the host) with ``optax.adam`` and
``eqx.apply_updates`` on the host, once per epoch.  ``adam_loop`` enqueues the whole fit at once through
``Engine.adam_fit`` (tsff_adam_fit: packed loss + gradient and one Adam update per step, k_adam.inc) and synchronises once per
chunk.  The steps are those of ``tsadar_amd.tree.Adam`` + ``tree.apply_updates`` bit for bit (see include/tsff.h), and the best
weights are tracked as the reference tracks them: the iterate AFTER the update of the step whose loss was the lowest.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

from . import tree
from .params import ThomsonParams

ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8   # optax.adam's defaults (the reference passes the learning rate only)


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
    if getattr(loss_fn, "angular", False) or "angular" in config["other"]["extraoptions"]["spectype"]:
        raise NotImplementedError("adam_loop: angular decks run through the reference's angular loop, not the 1-D Adam loop")
    if getattr(loss_fn, "distributed", False):
        raise NotImplementedError("adam_loop: distributed=True is not built (each step would all-reduce the 3 loss sums)")
    ts_params = previous_weights if previous_weights is not None else \
        ThomsonParams(config["parameters"], opt["batch_size"], activate=True)
    sm = ts_params.slots
    if sm.fval_active or sm.gen2d_active or getattr(sm, "fval2d_active", False):
        raise NotImplementedError("adam_loop: a trainable free-form distribution function (Arbitrary1V.fval) is not built on the "
                                  "device: its chain rule runs on the host (use vg_loss with tree.Adam)")
    diff, _ = tree.partition(ts_params, tree.get_filter_spec(config["parameters"], ts_params))
    act = [s for _, s in diff.slots]
    n_epochs = int(opt["num_epochs"])
    eng = loss_fn.ts_diag.engine(ts_params.activate)
    X = ts_params.to_matrix()
    B = X.shape[0]
    w = eng.loss_weights(B, loss_fn.i_norm, loss_fn.e_norm, config["data"]["ion_loss_scale"])
    db = loss_fn._device_batch(eng, batch, B)
    fe = None
    if ts_params.fval is not None:   # (a free-form f_e that is not trained: a constant table)
        from . import distribution as Dist

        fe = Dist.arbitrary_1v(ts_params.fval)
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
            if hasattr(progress, "set_description"):
                progress.set_description(f"Epoch {done}, Prev Epoch Loss {last:.2e}")
            else:
                progress(done, last)
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
    if getattr(loss_fn, "angular", False) or "angular" in config["other"]["extraoptions"]["spectype"]:
        raise NotImplementedError("lbfgs_loop: angular decks run through the reference's angular loop, not the 1-D scipy loop")
    if getattr(loss_fn, "distributed", False):
        raise NotImplementedError("lbfgs_loop: distributed=True is not built (each evaluation would all-reduce the packed buffer)")
    if str(opt.get("method", "l-bfgs-b")).lower() != "l-bfgs-b":
        raise NotImplementedError(f"lbfgs_loop: method {opt.get('method')!r} -- only l-bfgs-b is built on the device")
    if opt.get("grad_method", "AD") != "AD":
        raise NotImplementedError(f"lbfgs_loop: grad_method {opt.get('grad_method')!r} -- only the analytic gradient (AD) is built")
    ts_params = previous_weights if previous_weights is not None else \
        ThomsonParams(config["parameters"], opt["batch_size"], activate=True)
    sm = ts_params.slots
    if sm.fval_active or sm.gen2d_active or getattr(sm, "fval2d_active", False):
        raise NotImplementedError("lbfgs_loop: a trainable free-form distribution function (Arbitrary1V.fval) is not built on the "
                                  "device: its chain rule runs on the host (use vg_loss with scipy)")
    diff, static = tree.partition(ts_params, tree.get_filter_spec(config["parameters"], ts_params))
    _, loss_fn.unravel_weights = tree.ravel_pytree(diff)   # (as the reference leaves it)
    act = [s for _, s in diff.slots]
    eng = loss_fn.ts_diag.engine(ts_params.activate)
    X = ts_params.to_matrix()
    B = X.shape[0]
    w = eng.loss_weights(B, loss_fn.i_norm, loss_fn.e_norm, config["data"]["ion_loss_scale"])
    db = loss_fn._device_batch(eng, batch, B)
    fe = None
    if ts_params.fval is not None:   # (a free-form f_e that is not trained: a constant table)
        from . import distribution as Dist

        fe = Dist.arbitrary_1v(ts_params.fval)
    from .lbfgs import RUNNING

    opts = (10, 2.220446049250313e-09, 1e-5, int(opt["num_epochs"]), 15000, 20)
    step = max(1, int(chunk)) if chunk else LBFGS_CHUNK
    Xd, state, dinfo = eng.dev(X), None, None
    while True:
        Xd, state, _, dinfo = eng.lbfgs_fit(Xd, db, w, act, step, opts, state=state, f_hist=False, info=dinfo, fe=fe)
        res = eng.lbfgs_info(dinfo, state)   # the chunk's one synchronisation
        if progress is not None:
            if hasattr(progress, "set_description"):
                progress.set_description(f"Iteration {res['nit']}, Loss {res['f']:.2e}")
            else:
                progress(res["nit"], res["f"])
        if res["status"] != RUNNING:
            break
    if info is not None:
        info.update(res)
    out = ts_params.copy()
    out.X = eng.download(Xd).reshape(B, -1).copy()
    return res["f"], out
