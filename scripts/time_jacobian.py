"""Time tsff_spectrum_jacobian and tsff_loss_gauss_newton at bench.py's headline shape -- batch 4096, tests/decks.deck_fit
defaults and its six active leaves -- against what they replace, and write profiles/jacobian_timing.json:

  * ``jacobian``: one Engine.spectrum_jacobian call (both features);
  * ``gauss_newton``: one Engine.loss_gauss_newton call, and Engine.loss_hess at the same shape (a recorded number, no threshold);
  * ``central``: the same J by central differences -- 2 n_active Engine.forward calls and the subtraction on the device.  With
    ``--parent-tree DIR`` (a checkout of the parent commit with its library built) this part runs in a child process on that
    tree's package and library, on the same machine in the same invocation; without it, on this tree's forward (unchanged code).

``--tangent`` adds the DLM order to the leaves at the same batch, so that the planner picks the tangent form of the sweep
(k_jac_sweep<1, 3, false>) instead of the row form.  With ``--parent-tree`` every timed part of --what runs on both trees, each in a
child process of its own under a time limit, parent and this tree alternating for ``--rounds`` rounds; the first non-zero exit ends
the run.  ``ab`` then holds per part both trees' rounds and medians, s = the largest relative deviation of the parent's own rounds
from its median, and ``within`` = (this tree's median <= the parent's median x (1 + s)); the parts' top-level ms are this tree's medians.

Clocks are warm as in bench.py: every timed region follows an untimed spin of the same call (--spin-ms), and is K calls between
two device synchronisations.  ``--kernel-times`` adds the device time of the sweep kernel from rocprofv3 --kernel-trace runs of
their own, one per call type (the Jacobian call and the Gauss-Newton call run different tails of the same kernel), each averaged
over the last K dispatches behind the same clock warm-up (the program goes after ``--``; no counters are collected).

The requirement this script checks: ratio = jacobian_ms / central_ms <= 1.0."""
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
ROOT = os.environ.get("TSFF_TREE") or os.path.dirname(HERE)
THIS = os.path.dirname(HERE)
for p in (os.path.join(THIS, "tests"), ROOT):   # (decks and util are this tree's; the package is the tree's under test)
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


TANGENT_LEAVES = ("Te", "ne", "Ti", "Va", "lam", "amp1", "m")


def setup(B, tangent=False):
    import decks
    import util
    from tsadar_amd.engine import Engine
    from tsadar_amd.params import SlotMap

    cfg = decks.deck_fit(active=TANGENT_LEAVES) if tangent else decks.deck_fit()
    sa = util.sa_fit(B)
    nb = 64   # (the data of 64 oracle lineouts, tiled: the timing does not depend on the values)
    small = util.synthetic_batch(cfg, util.sa_fit(nb), nb, seed=3)
    batch = {k: np.tile(v, (B // nb,) + (1,) * (np.ndim(v) - 1)) for k, v in small.items()}
    normed = util.random_lineouts(cfg, B, seed=4, ranges=dict(m=(2.1, 4.3)) if tangent else None)
    act = [s for _, s in SlotMap(cfg["parameters"], True).active_leaves]
    eng = Engine(cfg, sa)
    X = eng.dev(util.normed_to_matrix(normed, 1))
    db = {k: (eng._vec(v, B) if k.endswith("amps") else eng._mat(v, B)) for k, v in batch.items()}
    ext = cfg["other"]["extraoptions"]
    c = 0.5 if (ext["fit_EPWb"] and ext["fit_EPWr"]) else 1.0
    w = np.array([1.0 if ext["fit_IAW"] else 0.0, c if ext["fit_EPWb"] else 0.0, c if ext["fit_EPWr"] else 0.0])
    return eng, X, db, w, act


def timed(fn, steps, spin_ms):
    import torch

    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    for _ in range(int(np.ceil(spin_ms * 1e-3 / max(one, 1e-6)))):   # untimed clock warm-up
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def central_fn(eng, X, db, act, h=1e-6):
    import torch

    B = X.shape[0]
    JE = torch.empty((B, len(act), 1024), dtype=torch.float64, device=X.device)
    JI = torch.empty_like(JE)

    def fn():
        for i, s in enumerate(act):
            Xp, Xm = X.clone(), X.clone()
            Xp[:, s] += h
            Xm[:, s] -= h
            Ep, Ip = eng.forward(Xp, db["e_amps"], db["i_amps"])
            Em, Im = eng.forward(Xm, db["e_amps"], db["i_amps"])
            torch.sub(Ep, Em, out=JE[:, i]).mul_(0.5 / h)
            torch.sub(Ip, Im, out=JI[:, i]).mul_(0.5 / h)
        return JE, JI
    return fn


def calls(args):
    eng, X, db, w, act = setup(args.batch, args.tangent)
    out = {}
    if "central" in args.what:
        out["central"] = (central_fn(eng, X, db, act), eng)
    if "jacobian" in args.what:
        out["jacobian"] = (lambda: eng.spectrum_jacobian(X, db["e_amps"], db["i_amps"], act), eng)
    if "gauss_newton" in args.what:
        out["gauss_newton"] = (lambda: eng.loss_gauss_newton(X, db, w, act), eng)
    if "loss_hess" in args.what:
        out["loss_hess"] = (lambda: eng.loss_hess(X, db, w, act), eng)
    return out, len(act)


def measure(args):
    res = {}
    fns, n = calls(args)
    for name, (fn, eng) in fns.items():
        steps = 1 if name == "loss_hess" else args.steps   # (hundreds of ms per call: its own warm-up)
        res[f"{name}_ms"] = timed(fn, steps, 0.0 if name == "loss_hess" else args.spin_ms)
        res[f"{name}_kernels"] = eng.last_launch()
    res["n_active"] = n
    return res


def once(args):
    """what a rocprofv3 run traces: the call type(s) of --what, each behind the same untimed clock warm-up as the timed runs, then
    args.steps calls -- the trace's last args.steps dispatches of the sweep are the ones at warm clocks"""
    fns, _ = calls(args)
    for name, (fn, _) in fns.items():
        timed(fn, args.steps, args.spin_ms)


def child(args, what, tree=None, extra=()):
    env = dict(os.environ)
    if tree:
        env["TSFF_TREE"] = os.path.abspath(tree)
        env.pop("TSFF_LIBRARY", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--what", *what, "--batch", str(args.batch), "--steps", str(args.steps),
           "--spin-ms", str(args.spin_ms), *(["--tangent"] if args.tangent else []), *extra]
    return cmd, env


def run_child(args, what, tree=None):
    """measure() of ``what`` in a child process on ``tree`` (None: this tree), under a time limit -> its result, or None"""
    cmd, env = child(args, what, tree=tree)
    r = subprocess.run(["timeout", "-k", "10", str(args.child_timeout)] + cmd, env=env, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"child on {tree or THIS}: exit {r.returncode}", r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
        return None
    return json.loads(line[-1][7:])


def both_trees(args, res):
    """every part of --what on the parent's tree and on this one, alternating for args.rounds rounds (central: parent, first round)"""
    parts = [w for w in args.what if w != "central"]
    ms = {"parent": {}, "new": {}}
    for rnd in range(args.rounds):
        for tag, tree in (("parent", args.parent_tree), ("new", None)):
            what = parts + (["central"] if tag == "parent" and rnd == 0 and "central" in args.what else [])
            out = run_child(args, what, tree)
            if out is None:
                return False
            for k, v in out.items():
                if k == "central_ms" or not k.endswith("_ms"):
                    res[k if k.startswith("central") or tag == "new" else "parent_" + k] = v
                else:
                    ms[tag].setdefault(k[:-3], []).append(v)
    res["ab"] = {}
    for part in parts:
        p, n = ms["parent"][part], ms["new"][part]
        pm, nm = float(np.median(p)), float(np.median(n))
        s = max(abs(v - pm) / pm for v in p)
        res[part + "_ms"] = nm
        res["ab"][part] = {"parent_ms": p, "new_ms": n, "parent_median_ms": pm, "new_median_ms": nm, "s": s, "within": bool(nm <= pm * (1.0 + s))}
    return True


def kernel_times(args, what):
    """Device time of the sweep kernel for ONE call type (``what``), from a rocprofv3 --kernel-trace run of its own: the mean over
    the last args.steps dispatches (behind the clock warm-up), and the number of dispatches traced."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"error": "rocprofv3 not found"}
    d = tempfile.mkdtemp(prefix="jac_prof_")
    cmd, env = child(args, [what], extra=["--once"])
    r = subprocess.run([prof, "--kernel-trace", "-d", d, "--output-format", "csv", "--"] + cmd, env=env, capture_output=True, text=True)
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "k_jac_sweep" in row.get("Kernel_Name", ""):
                rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    shutil.rmtree(d, ignore_errors=True)
    if len(rows) < args.steps:
        return {"error": "no kernel trace", "rc": r.returncode, "stderr": r.stderr[-400:]}
    rows.sort()
    last = rows[-args.steps:]
    name = last[-1][2].replace("void ", "").replace("tsff::", "").split("(")[0]
    return {"kernel": name, "call": what, "dispatches_traced": len(rows), "averaged_over_last": len(last),
            "avg_ms": float(np.mean([e - b for b, e, _ in last])) * 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--spin-ms", type=float, default=300.0)
    ap.add_argument("--what", nargs="+", default=["jacobian", "gauss_newton", "loss_hess", "central"])
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit with its library built: the central differences run there")
    ap.add_argument("--tangent", action="store_true", help="the DLM order among the leaves: the tangent form of the sweep")
    ap.add_argument("--rounds", type=int, default=3, help="with --parent-tree: rounds of (parent, this tree)")
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--kernel-times", action="store_true", help="add rocprofv3 kernel times from a separate run")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--once", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(THIS, "profiles", "jacobian_timing.json"))
    args = ap.parse_args()
    if args.child:
        if args.once:
            once(args)
        else:
            print("RESULT " + json.dumps(measure(args)), flush=True)
        return 0
    deck = "tests/decks.deck_fit(active=%r), m drawn in [2.1, 4.3]" % (TANGENT_LEAVES,) if args.tangent else "tests/decks.deck_fit()"
    res = {"shape": {"B": args.batch, "deck": deck, "points_per_pixel": 1, "nvx": 128}, "steps": args.steps,
           "clock_warmup_ms": args.spin_ms}
    if args.parent_tree:
        if not both_trees(args, res):
            return 1
        res["rounds"] = args.rounds
        res["central_on"] = "the parent commit's package and library (child process, same machine, same invocation)"
    else:
        res["central_on"] = "this tree's tsff_forward"
        res.update(measure(args))
    n = res["n_active"]
    res["central_forward_calls"] = 2 * n
    if "jacobian_ms" in res and "central_ms" in res:
        res["ratio_jacobian_over_central"] = res["jacobian_ms"] / res["central_ms"]
        res["requirement_ratio_le_1"] = bool(res["ratio_jacobian_over_central"] <= 1.0)
    if "gauss_newton_ms" in res and "loss_hess_ms" in res:
        res["ratio_gauss_newton_over_loss_hess"] = res["gauss_newton_ms"] / res["loss_hess_ms"]
    if args.kernel_times:
        res["rocprofv3_sweep_kernel"] = {w: kernel_times(args, w) for w in ("jacobian", "gauss_newton")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
