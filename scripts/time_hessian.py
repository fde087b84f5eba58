"""Time LossFunction.h_loss_wrt_params(method="exact") against method="central" in one process, on the same seeded inputs,
with a device synchronisation around every call.  Shapes: (a) the reference's shipped deck -- B = 2, 5 points per pixel,
nvx 128; (b) B = 4096, 1 point per pixel.  Leaves {Te, ne, m, amp1, amp2, lam} (the reference's production leaves).
Prints one JSON line per shape."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import decks  # noqa: E402
import util  # noqa: E402
from tsadar_amd import ThomsonParams  # noqa: E402
from tsadar_amd.loss_function import LossFunction  # noqa: E402

LEAVES = ("Te", "ne", "m", "amp1", "amp2", "lam")


def run(name, B, ppp, reps):
    cfg = decks.deck_fit(points_per_pixel=ppp, nvx=128, active=LEAVES)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=3)
    normed = util.random_lineouts(cfg, B, seed=4)
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    tp.X[:] = util.normed_to_matrix(normed, 1)
    res = {"shape": name, "B": B, "points_per_pixel": ppp, "nvx": 128, "leaves": list(LEAVES)}
    for method in ("exact", "central"):
        lf.h_loss_wrt_params(tp, batch, method=method)   # warm-up (tables, workspaces)
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lf.h_loss_wrt_params(tp, batch, method=method)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[f"{method}_ms_median"] = 1e3 * float(np.median(ts))
        res[f"{method}_ms_min"] = 1e3 * float(np.min(ts))
    res["faster"] = "exact" if res["exact_ms_median"] < res["central_ms_median"] else "central"
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    run("a", 2, 5, 20)
    run("b", 4096, 1, 3)
