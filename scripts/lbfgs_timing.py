"""Wall time of the 1-D L-BFGS-B fit (the reference's default _1d_scipy_loop_, inverse/loops.py:20-56) two ways, at B = 256 and
B = 4096 on the baseline deck (6 trainable leaves per lineout), num_epochs = 120, after a warm-up fit:
  (a) host_reference: scipy.optimize.minimize(LossFunction.vg_loss, ..., method="L-BFGS-B", jac=True), the reference's loop;
  (b) device:         loops.lbfgs_loop -- tsff_lbfgs_fit, chunks of 16 evaluations, one synchronisation per chunk.
Plus the wall time per evaluation of (b) against Engine.loss_grad_packed alone (the same evaluations enqueued back to back without
the optimiser step).  Writes JSON to <out>.
usage: python scripts/lbfgs_timing.py <out.json> [epochs] [B ...]
       python scripts/lbfgs_timing.py --device-only B epochs   (a warm-up fit and one fit: for rocprofv3 --kernel-trace --stats)
       python scripts/lbfgs_timing.py --merge-stats <out.json> <B> <kernel_stats.csv>   (adds k_lbfgs_step's rocprofv3 time)"""
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scipy.optimize import minimize  # noqa: E402

from tsadar_amd import loops, synthetic as S, tree  # noqa: E402
from tsadar_amd.calibration import sa_lookup  # noqa: E402
from tsadar_amd.engine import Engine  # noqa: E402
from tsadar_amd.loss_function import LossFunction  # noqa: E402


def setup(B, epochs):
    cfg = S.baseline_deck(points_per_pixel=1, batch_size=B)
    cfg["optimizer"].update(method="l-bfgs-b", num_epochs=epochs)
    sa = sa_lookup("P9")
    sa = dict(sa=sa["sa"], weights=sa["weights"] * np.ones([B, 10]))
    rng = np.random.default_rng(S.SEED)
    truth = S.draw_params(cfg, B, rng)
    eng0 = Engine(cfg, sa)
    batch = S.make_batch(eng0, truth, rng)
    hb = {k: (v.cpu().numpy() if v is not None else None) for k, v in batch.items()}
    hb["noise_e"] = np.zeros((B, 1024))
    hb["noise_i"] = np.zeros((B, 1024))
    del eng0
    lf = LossFunction(cfg, sa, hb)
    tp = S.draw_params(cfg, B, rng)
    return cfg, lf, tp, hb


def host_reference(cfg, lf, tp, hb):
    diff, static = tree.partition(tp, tree.get_filter_spec(cfg["parameters"], tp))
    x0, lf.unravel_weights = tree.ravel_pytree(diff)
    res = minimize(lf.vg_loss, x0, args=(static, hb), method="L-BFGS-B", jac=True, bounds=None,
                   options={"maxiter": cfg["optimizer"]["num_epochs"]})
    return dict(f=float(res.fun), nit=int(res.nit), nfev=int(res.nfev), status=int(res.status))


def device(cfg, lf, tp, hb):
    info = {}
    f, _ = loops.lbfgs_loop(cfg, lf, tp, hb, info=info)
    return dict(f=float(f), nit=info["nit"], nfev=info["nfev"], status=info["scipy_status"])


def timed(fn, *a):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn(*a)
    torch.cuda.synchronize()
    return time.perf_counter() - t, r


def packed_only_ms(lf, tp, hb, n):
    eng = lf.ts_diag.engine(tp.activate)
    B = tp.X.shape[0]
    act = [s for _, s in tp.slots.active_leaves]
    w = eng.loss_weights(B, lf.i_norm, lf.e_norm, lf.cfg["data"]["ion_loss_scale"])
    db = lf._device_batch(eng, hb, B)
    X = eng.upload(tp.X)
    gm = tp.grad_mask()
    eng.loss_grad_packed(X, db, w, gm, act)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        eng.loss_grad_packed(X, db, w, gm, act)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def merge_stats(out, B, path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    row = next(r for r in rows if r["Name"].startswith("tsff::k_lbfgs_step") or r["Name"].startswith("k_lbfgs_step"))
    res = json.load(open(out))
    r = res["sizes"][str(B)]
    passes = 2 * 10 + 6   # launches of k_lbfgs_step per evaluation at maxcor 10
    evals = int(row["Calls"]) / passes
    r["k_lbfgs_step_rocprof_calls"] = int(row["Calls"])
    r["k_lbfgs_step_rocprof_avg_us_per_launch"] = float(row["AverageNs"]) / 1e3
    r["k_lbfgs_step_rocprof_us_per_evaluation"] = float(row["TotalDurationNs"]) / evals / 1e3
    # the optimiser's kernel time per evaluation over loss_grad_packed's wall time per evaluation
    r["k_lbfgs_step_over_loss_grad_packed"] = r["k_lbfgs_step_rocprof_us_per_evaluation"] / 1e3 / r["loss_grad_packed_ms_per_evaluation"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(r))


def main():
    if sys.argv[1] == "--device-only":
        B, n = int(sys.argv[2]), int(sys.argv[3])
        cfg, lf, tp, hb = setup(B, n)
        device(cfg, lf, tp, hb)
        device(cfg, lf, tp, hb)
        torch.cuda.synchronize()
        return
    if sys.argv[1] == "--merge-stats":
        merge_stats(sys.argv[2], int(sys.argv[3]), sys.argv[4])
        return
    out = sys.argv[1]
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 120
    sizes = [int(b) for b in sys.argv[3:]] or [256, 4096]
    res = {"epochs": epochs, "deck": "synthetic.baseline_deck, 6 trainable leaves per lineout, l2, points_per_pixel 1",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for B in sizes:
        cfg, lf, tp, hb = setup(B, epochs)
        device(cfg, lf, tp, hb)   # warm-up (kernels loaded, buffers sized)
        t_dev, d = timed(device, cfg, lf, tp, hb)
        t_host, h = timed(host_reference, cfg, lf, tp, hb)
        # lbfgs_loop enqueues whole chunks of 16: evaluations after the end run too and are counted here
        n_run = -(-d["nfev"] // loops.LBFGS_CHUNK) * loops.LBFGS_CHUNK
        r = dict(device_fit_s=t_dev, host_reference_fit_s=t_host, speedup_fit=t_host / t_dev, device=d, host_reference=h,
                 device_evaluations_enqueued=n_run, device_ms_per_evaluation=t_dev / n_run * 1e3,
                 loss_grad_packed_ms_per_evaluation=packed_only_ms(lf, tp, hb, 50))
        r["device_overhead_per_evaluation"] = r["device_ms_per_evaluation"] / r["loss_grad_packed_ms_per_evaluation"] - 1.0
        res["sizes"][str(B)] = r
        print(B, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
