"""Time tsff_lm_fit (the per-lineout Levenberg-Marquardt fit, k_lm.inc) at bench.py's headline shape -- batch 4096,
tests/decks.deck_fit defaults and its six active leaves -- and write profiles/lm_timing.json:

  * ``per_evaluation``: the device time of one evaluation of tsff_lm_fit (k_jac_sweep + k_lm_step) over a 16-evaluation chunk,
    by device events, against the stand-alone Engine.loss_gauss_newton call at the same shape, alternated in the same run.
    The tolerances of the timed fits are zero and lam_max is 1e300, so every lineout runs all 16 evaluations.  The
    requirement: ratio = lm_eval_ms / gauss_newton_ms <= 1.10;
  * ``seven_eighths_terminal``: the same chunk with the status of seven lineouts in eight, drawn at random, set to terminal
    (no gate; the sweep's persistent workgroups keep their fixed share of the lineouts, so the slowest one sets the time);
  * ``loops``: loops.lm_loop against loops.lbfgs_loop (120 iterations), same start and batch: evaluations, wall time and final
    mean loss of each (no gate);
  * ``--kernel-share``: k_lm_step's share of the chunk's kernel time from a rocprofv3 --kernel-trace --stats run of its own
    (the program goes after ``--``; no counters are collected).

Clocks are warm as in bench.py: every timed window follows an untimed spin of the same call and lasts at least --window-ms.

``--oracle-probe`` needs no GPU: lm.minimize on the NumPy oracle with central-difference Jacobians for the inputs of
tests/test_lm_device.py's D1 deck (p = 0.01), 16 evaluations -- the check of the bound test_fit_makes_progress asserts."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

CHUNK = 16


def oracle_probe(n_evals=16, h=1e-6, seed=None):
    import test_lm_device as T
    from oracle import tsadar_oracle as orc
    from tsadar_amd import lm

    s = T._case("D1") if seed is None else T._case("D1", seed=seed)
    cfg, sa, batch, names = s["cfg"], s["sa"], s["batch"], s["names"]
    iaw, blue, red = s["masks"]
    i_norm, e_norm = s["norms"]
    # Engine.loss_weights(1, ...) of this deck: iaw + (blue + red) / 2, each a mean over its range
    w = [cfg["data"]["ion_loss_scale"] / (iaw[0].sum() * i_norm ** 2), 0.5 / (blue[0].sum() * e_norm ** 2), 0.5 / (red[0].sum() * e_norm ** 2)]
    start = orc.init_normed_params(cfg["parameters"], T.B, True)

    def spectra(x):
        nm = {k: np.array(v, dtype=np.float64, copy=True) for k, v in start.items()}
        for a, k in enumerate(names):
            nm[k] = x[:, a].copy()
        return orc.ts_diag(cfg, sa, nm, batch, True)[:2]

    def fgh(x):
        E, I = spectra(x)
        JE, JI = [], []
        for a in range(len(names)):
            xp, xm = x.copy(), x.copy()
            xp[:, a] += h
            xm[:, a] -= h
            (Ep, Ip), (Em, Im) = spectra(xp), spectra(xm)
            JE.append((Ep - Em) / (2 * h))
            JI.append((Ip - Im) / (2 * h))
        JE, JI = np.stack(JE, axis=1), np.stack(JI, axis=1)   # [B, n, 1024]
        F, G, H = np.zeros(T.B), np.zeros((T.B, len(names))), np.zeros((T.B, len(names), len(names)))
        for k, (mask, J, d, t) in enumerate(((iaw, JI, batch["i_data"], I), (blue, JE, batch["e_data"], E), (red, JE, batch["e_data"], E))):
            for b in range(T.B):
                m = mask[b]
                r = d[b][m] - t[b][m]
                F[b] += w[k] * np.sum(r * r)
                G[b] += w[k] * (J[b][:, m] @ (-2.0 * r))
                H[b] += w[k] * 2.0 * (J[b][:, m] @ J[b][:, m].T)
        return F, G, H

    x = np.stack([start[k] for k in names], axis=1)
    st, f0 = lm.State(*x.shape), None
    for k in range(n_evals):
        if not np.any(st.status == lm.RUNNING):
            break
        F, G, H = fgh(x)
        f0 = F if f0 is None else f0
        x = lm.step(st, x, F, G, H, T.OPTS)
        print(f"evaluation {k + 1}: f {st.f}, status {st.status}", flush=True)
    out = dict(f0=f0.tolist(), f=st.f.tolist(), ratio=(st.f / f0).tolist(), status=st.status.tolist(), nit=st.nit.tolist(), nfev=st.nfev.tolist())
    print(json.dumps(out))
    return out


def setup(B):
    import decks
    import util
    from oracle import tsadar_oracle as orc
    from tsadar_amd import ThomsonParams
    from tsadar_amd.engine import Engine

    cfg = decks.deck_fit()
    cfg["optimizer"].update(batch_size=B, num_epochs=120)
    nb = 64   # (the data of 64 oracle lineouts, tiled: the timing does not depend on the values)
    small = util.synthetic_batch(cfg, util.sa_fit(nb), nb, seed=3)
    batch = {k: np.tile(v, (B // nb,) + (1,) * (np.ndim(v) - 1)) for k, v in small.items()}
    sa = util.sa_fit(B)
    eng = Engine(cfg, sa)
    tp = ThomsonParams(cfg["parameters"], B, batch=True, activate=True)
    act = [s for _, s in tp.slots.active_leaves]
    X0 = tp.to_matrix().copy()
    X0[:, act] += np.random.default_rng(5).normal(0.0, 0.05, (B, len(act)))
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    w = eng.loss_weights(1, i_norm, e_norm, cfg["data"]["ion_loss_scale"])
    db = {k: (eng._vec(v, B) if k.endswith("amps") else eng._mat(v, B)) for k, v in batch.items()}
    return cfg, sa, batch, eng, X0, db, w, act


def window_ms(fn, min_ms):
    """fn() between two device events, repeated until the window lasts min_ms -> ms per call"""
    import torch

    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_ms:
            return ms / n
        n = max(n + 1, int(np.ceil(n * 1.2 * min_ms / max(ms, 1e-3))))


def chunk_fn(eng, X0, db, w, act, opts, poke=None):
    """One 16-evaluation chunk of a fresh fit (the state and the start restored on the device, inside the window: two copies)."""
    from tsadar_amd import lm

    torch = eng.torch
    B, n = X0.shape[0], len(act)
    Xs = eng.dev(X0)
    X, state = Xs.clone(), torch.zeros(lm.state_size(B, n), dtype=torch.float64, device=eng.device)
    s0 = state.clone()
    if poke is not None:
        poke(s0)

    def fn():
        X.copy_(Xs)
        state.copy_(s0)
        eng.lm_fit(X, db, w, act, CHUNK, opts, state=state)
    return fn, state


def measure(args):
    from tsadar_amd import lm

    cfg, sa, batch, eng, X0, db, w, act = setup(args.batch)
    torch = eng.torch
    B = args.batch
    opts = lm.Options(tau=1e-3, gtol=0.0, ftol=0.0, xtol=0.0, maxiter=10 ** 6, maxfun=10 ** 6, lam_max=1e300)
    Xd = eng.dev(X0)
    gn = lambda: eng.loss_gauss_newton(Xd, db, w, act)
    fit, state = chunk_fn(eng, X0, db, w, act, opts)
    for fn in (gn, fit):   # warm-up: buffers, clocks
        window_ms(fn, args.window_ms)
    rounds = []
    for _ in range(args.rounds):   # alternated in the same run
        rounds.append((window_ms(fit, args.window_ms) / CHUNK, window_ms(gn, args.window_ms)))
    fit()
    kernels = eng.last_launch()[-2:]
    torch.cuda.synchronize()
    st = lm.unpack(eng.download(state), B, len(act))
    lm_ms, gn_ms = float(np.median([r[0] for r in rounds])), float(np.median([r[1] for r in rounds]))
    res = {"per_evaluation": {"lm_eval_ms": lm_ms, "gauss_newton_ms": gn_ms, "ratio": lm_ms / gn_ms, "requirement_ratio_le_1.10": bool(lm_ms / gn_ms <= 1.10),
                              "rounds": rounds, "running_after_chunk": int(np.sum(st.status == lm.RUNNING)), "kernels_per_evaluation": kernels}}

    def poke(s0):   # seven lineouts in eight terminal from the start, drawn at random (a stride would fall on the sweep's own)
        flags = np.full(B, lm.STOP_COUNT, dtype=np.int32)
        flags[np.random.default_rng(8).choice(B, B // 8, replace=False)] = 0
        s0[:(B + 1) // 2].view(torch.int32)[:B] = torch.from_numpy(flags).to(eng.device)
    fit8, _ = chunk_fn(eng, X0, db, w, act, opts, poke)
    window_ms(fit8, args.window_ms)
    res["seven_eighths_terminal"] = {"lm_eval_ms": window_ms(fit8, args.window_ms) / CHUNK}
    res["loops"] = loops(cfg, sa, batch, X0)
    return res


def loops(cfg, sa, batch, X0):
    import copy

    import torch
    from tsadar_amd import ThomsonParams, loops as Lp
    from tsadar_amd.loss_function import LossFunction

    B = X0.shape[0]
    out = {}
    for name, fn in (("lm_loop", Lp.lm_loop), ("lbfgs_loop", Lp.lbfgs_loop)):
        c = copy.deepcopy(cfg)
        loss_fn = LossFunction(c, sa, batch)
        start = ThomsonParams(c["parameters"], B, batch=True, activate=True)
        start.X = X0.copy()
        info = {}
        fn(c, loss_fn, start.copy(), batch, info={})   # warm-up: buffers, clocks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, _ = fn(c, loss_fn, start.copy(), batch, info=info)
        torch.cuda.synchronize()
        out[name] = {"wall_ms": 1e3 * (time.perf_counter() - t0), "final_mean_loss": float(loss),
                     "evaluations": int(info["n_evals"] if name == "lm_loop" else info["nfev"])}
        if name == "lm_loop":
            out[name]["status_counts"] = np.bincount(info["status"], minlength=7).tolist()
            out[name]["median_lineout_loss"] = float(np.median(info["f"]))
    return out


def once(args):
    """what the rocprofv3 run traces: a few timed chunks behind the clock warm-up"""
    from tsadar_amd import lm

    cfg, sa, batch, eng, X0, db, w, act = setup(args.batch)
    opts = lm.Options(tau=1e-3, gtol=0.0, ftol=0.0, xtol=0.0, maxiter=10 ** 6, maxfun=10 ** 6, lam_max=1e300)
    fit, _ = chunk_fn(eng, X0, db, w, act, opts)
    window_ms(fit, args.window_ms)
    window_ms(fit, args.window_ms)


def kernel_share(args):
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"error": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="lm_prof_")
    cmd = [sys.executable, os.path.abspath(__file__), "--once", "--batch", str(args.batch), "--window-ms", str(args.window_ms)]
    r = subprocess.run([prof, "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--"] + cmd, capture_output=True, text=True)
    tot = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row.get("Kernel_Name", "").replace("void ", "").replace("tsff::", "").split("(")[0]
            tot[name] = tot.get(name, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
    shutil.rmtree(d, ignore_errors=True)
    both = {k: v for k, v in tot.items() if k.startswith(("k_jac_sweep", "k_lm_step"))}
    if not both:
        return {"error": "no kernel trace", "rc": r.returncode, "stderr": r.stderr[-400:]}
    s = sum(both.values())
    return {k: {"total_ms": v * 1e-6, "share": v / s} for k, v in both.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--kernel-share", action="store_true", help="add k_lm_step's share from a rocprofv3 --kernel-trace --stats run of its own")
    ap.add_argument("--oracle-probe", action="store_true", help="CPU only: lm.minimize on the NumPy oracle for the test's D1 inputs")
    ap.add_argument("--seed", type=int, default=None, help="--oracle-probe: another seed than the test's for the draw of the truth")
    ap.add_argument("--once", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_timing.json"))
    args = ap.parse_args()
    if args.oracle_probe:
        oracle_probe(seed=args.seed)
        return 0
    if args.once:
        once(args)
        return 0
    res = {"shape": {"B": args.batch, "deck": "tests/decks.deck_fit()", "points_per_pixel": 1, "nvx": 128, "n_active": 6}, "chunk": CHUNK,
           "window_ms": args.window_ms, "rounds": args.rounds}
    res.update(measure(args))
    if args.kernel_share:
        res["rocprofv3_kernel_share"] = kernel_share(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
