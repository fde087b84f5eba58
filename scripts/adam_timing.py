"""Wall time per step of the 1-D Adam fit (the reference's _1d_adam_loop_, inverse/loops.py:59-95) three ways, at B = 256 and
B = 4096 on the baseline deck (6 trainable leaves per lineout), N steps after a warm-up:
  (a) host_reference: LossFunction.vg_loss in the adam convention (spectra to the host) + tree.Adam, the reference's loop body;
  (b) host_packed:    Engine.loss_grad_packed (no spectra) + tree.Adam in NumPy, one download per step;
  (c) device:         loops.adam_loop -- the whole fit enqueued by tsff_adam_fit, one synchronisation.
Plus the main kernel's HIP-event time per step of (c) in a separate pass (tsff_enable_timing).  Writes JSON to <out>.
usage: python scripts/adam_timing.py <out.json> [steps] [B ...]
       python scripts/adam_timing.py --device-only B steps   (one warm-up fit and one fit of `steps` steps: for rocprofv3 --stats)"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tsadar_amd import loops, synthetic as S, tree  # noqa: E402
from tsadar_amd.calibration import sa_lookup  # noqa: E402
from tsadar_amd.engine import Engine  # noqa: E402
from tsadar_amd.loss_function import LossFunction  # noqa: E402

LR, WARM = 0.02, 10


def setup(B, steps):
    cfg = S.baseline_deck(points_per_pixel=1, batch_size=B)
    cfg["optimizer"].update(method="adam", learning_rate=LR, num_epochs=steps)
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


def host_reference(cfg, lf, tp, hb, n):
    opt = tree.Adam(LR)
    diff, static = tree.partition(tp, tree.get_filter_spec(cfg["parameters"], tp))
    state = opt.init(diff)
    best = 1e16
    for _ in range(n):
        (loss, aux), grad = lf.vg_loss(diff, static, hb)
        updates, state = opt.update(grad, state)
        diff = tree.apply_updates(diff, updates)
        if loss < best:
            best, best_w = loss, tree.combine(diff, static)
    return best


def host_packed(cfg, lf, tp, hb, n):
    eng = lf.ts_diag.engine(tp.activate)
    B = tp.X.shape[0]
    act = [s for _, s in tp.slots.active_leaves]
    w = eng.loss_weights(B, lf.i_norm, lf.e_norm, cfg["data"]["ion_loss_scale"])
    db = lf._device_batch(eng, hb, B)
    gm = tp.grad_mask()
    opt = tree.Adam(LR)
    diff, static = tree.partition(tp, tree.get_filter_spec(cfg["parameters"], tp))
    state = opt.init(diff)
    X = tp.X.copy()
    best = 1e16
    for _ in range(n):
        packed, _, _ = eng.loss_grad_packed(eng.upload(X), db, w, gm, act)
        host = eng.download(packed)
        loss = (w[0] * host[0] + w[1] * host[1]) + w[2] * host[2]
        updates, state = opt.update(diff.like(host[3:]), state)
        diff = tree.apply_updates(diff, updates)
        for k, s in enumerate(act):
            X[:, s] = diff.values[k]
        if loss < best:
            best, best_X = loss, X.copy()
    return best


def device(cfg, lf, tp, hb, n):
    cfg["optimizer"]["num_epochs"] = n
    return loops.adam_loop(cfg, lf, tp, hb)[0]


def per_step(fn, cfg, lf, tp, hb, n):
    fn(cfg, lf, tp, hb, WARM)
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn(cfg, lf, tp, hb, n)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def main():
    if sys.argv[1] == "--device-only":
        B, n = int(sys.argv[2]), int(sys.argv[3])
        cfg, lf, tp, hb = setup(B, n)
        device(cfg, lf, tp, hb, WARM)
        device(cfg, lf, tp, hb, n)
        torch.cuda.synchronize()
        return
    out = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    sizes = [int(b) for b in sys.argv[3:]] or [256, 4096]
    res = {"steps": n, "warmup": WARM, "deck": "synthetic.baseline_deck, 6 trainable leaves per lineout, l2, points_per_pixel 1",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for B in sizes:
        cfg, lf, tp, hb = setup(B, n)
        r = {name + "_ms_per_step": per_step(fn, cfg, lf, tp, hb, n)
             for name, fn in (("host_reference", host_reference), ("host_packed", host_packed), ("device", device))}
        eng = lf.ts_diag.engine(tp.activate)
        eng.enable_timing(n)
        device(cfg, lf, tp, hb, n)
        kt = eng.kernel_times_ms()
        eng.enable_timing(0)
        r["device_main_kernel_ms_per_step"] = float(np.mean(kt))
        r["speedup_device_over_host_reference"] = r["host_reference_ms_per_step"] / r["device_ms_per_step"]
        r["speedup_device_over_host_packed"] = r["host_packed_ms_per_step"] / r["device_ms_per_step"]
        res["sizes"][str(B)] = r
        print(B, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
