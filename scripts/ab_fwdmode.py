"""A/B of the forward-mode kernels (k_hess_pairs, k_jac_sweep, k_ffjvp) and of the per-lineout table kernels between two builds of the
library, bit for bit:

    python scripts/ab_fwdmode.py --parent-lib ab_prev/tsadar_amd/libtsff.so [--twin] [--out profiles/fwdmode_bits.txt]

Engine.loss_hess, Engine.spectrum_jacobian and Engine.loss_gauss_newton run on every deck of CASES in tests/test_hessian_exact.py
(B = 2) and tests/test_jacobian.py (B = 3), at the tests' own seeds; Engine.form_factor_jvp (value and tangents) on every deck of
CASES in tests/test_form_factor_jvp.py with that test's inputs, with its fe_dot and without any; Engine.loss_grad (terms, gradient,
spectra and, on the free-form deck, the f_e gradient) on the DLM deck at B = 33 and the free-form deck at B = 65 of
tests/test_per_lineout_tables_gpu.py (k_fe_vectors, k_fe_adjoint and the W-table GEMMs around them).  Each library runs in a fresh child process of its own,
selected with TSFF_LIBRARY, under its own `timeout -k 10`, one after the other; the first non-zero exit ends the run.  A child
catches nothing: a refusal, a HIP error or a fault that surfaces at a synchronise ends it there, with a non-zero exit, before
anything else starts on the device.  Each child saves its arrays (.npz); this process compares them and prints the report (--out
also writes it to a file).  Per case and output: `equal` (np.array_equal), or the largest deviation from the parent relative to the
largest entry, which fails the run.  The only fallback is for the Jacobian rows of the test_jacobian.py decks: with --twin such an
output passes if the new library is no farther from that test's twin than max(2 x the parent's distance, 1e-12 x the largest entry)
(the form of the rule at tests/test_hessian_exact.py:529-531).  A Hessian, Gauss-Newton matrix, gradient or loss term that differs
always fails: no twin distance is computed for them."""
import argparse
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def child(out):
    import torch

    import test_form_factor_jvp as tf
    import test_hessian_exact as th
    import test_jacobian as tj
    import test_per_lineout_tables_gpu as tp
    import util

    res = {}

    def put(key, tensors):
        torch.cuda.synchronize()
        for name, t in zip(("a", "b", "c"), tensors):
            if t is not None:
                res[f"{key}/{name}"] = t.cpu().numpy()

    for cid, builder in th.CASES:
        cfg = builder()
        sa, batch, normed = th._setup(cfg, 2, seed=53)
        act = th._leaves(cfg)[2]
        n_ion = sum(1 for k in cfg["parameters"] if k.startswith("ion-"))
        X = util.normed_to_matrix(normed, n_ion)
        eng = th._engine(cfg, sa)
        w = th._weights(cfg)
        put(f"hess_cases/{cid}/loss_hess", eng.loss_hess(X, batch, w, act))
        put(f"hess_cases/{cid}/jacobian", eng.spectrum_jacobian(X, batch["e_amps"], batch["i_amps"], act))
        if cid != "l1":   # (l'' = 0: the Gauss-Newton call refuses l1)
            put(f"hess_cases/{cid}/gauss_newton", eng.loss_gauss_newton(X, batch, w, act))
        print(f"hess_cases/{cid}: {[k for k in eng.last_launch() if k.startswith(('k_hess_pairs', 'k_jac_sweep'))]}", flush=True)
    for cid in tj.CASES:
        s = tj._inputs(cid)
        eng = tj._engine(s)
        w = tj._weights(s["cfg"])
        put(f"jac_cases/{cid}/jacobian", eng.spectrum_jacobian(s["X"], s["batch"]["e_amps"], s["batch"]["i_amps"], s["act"], fe=s["fe"]))
        form = [k for k in eng.last_launch() if k.startswith("k_jac_sweep")]
        put(f"jac_cases/{cid}/gauss_newton", eng.loss_gauss_newton(s["X"], s["batch"], w, s["act"], fe=s["fe"]))
        put(f"jac_cases/{cid}/loss_hess", eng.loss_hess(s["X"], s["batch"], w, s["act"], fe=s["fe"]))
        print(f"jac_cases/{cid}: {form + [k for k in eng.last_launch() if k.startswith('k_hess_pairs')]}", flush=True)
    for cid in tf.CASES:
        s, eng = tf._inputs(cid), tf._engine(cid)
        if s["fd"] is not None:
            put(f"ffjvp_cases/{cid}/with_fe_dot", eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"], want_P=True))
        put(f"ffjvp_cases/{cid}/without_fe_dot", eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], None, want_P=True))
        print(f"ffjvp_cases/{cid}: {[k for k in eng.last_launch() if k.startswith(('k_ffjvp', 'k_fe_direction'))]}", flush=True)
    for name in ("dlm33", "fe65"):
        r = tp.run(name)   # (the test's own call: loss_grad with the spectra, want_fe_grad on the free-form deck)
        for k, v in r["host"].items():
            res[f"table_cases/{name}/loss_grad/{k}"] = v
        print(f"table_cases/{name}: {[k for k in r['launched'] if k.startswith(('k_fe_', 'k_wgemm'))]}", flush=True)
    np.savez(out, **res)
    return 0


def twin_rule(key, p, n, largest):
    """The fallback for Jacobian rows that differ: new no farther from the twin than max(2 x parent's distance, 1e-12 x largest).
    -> None for every other output (no fallback: it fails)."""
    import test_jacobian as tj

    group, cid, call, name = key.split("/")
    if group != "jac_cases" or call != "jacobian":
        return None
    JE, JI = tj._twin(cid)[:2]
    t = {"a": JE, "b": JI}[name]
    dp, dn = np.max(np.abs(p - t)), np.max(np.abs(n - t))
    return dn <= max(2.0 * dp, 1e-12 * largest), dp, dn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libtsff.so (same ABI)")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "tsadar_amd", "libtsff.so"))
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child")
    ap.add_argument("--twin", action="store_true", help="judge Jacobian rows (test_jacobian.py decks) that differ by their distance to the twin")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    with tempfile.TemporaryDirectory(prefix="ab_fwdmode_") as tmp:
        files = {}
        for tag, lib in (("parent", args.parent_lib), ("new", args.new_lib)):
            files[tag] = os.path.join(tmp, tag + ".npz")
            env = dict(os.environ, TSFF_LIBRARY=os.path.abspath(lib))
            r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", files[tag]],
                               env=env)
            if r.returncode != 0:
                print(f"{tag}: exit {r.returncode}; stopping", file=sys.stderr)
                return r.returncode
        return compare(files["parent"], files["new"], args.twin, args.out)


def compare(parent_npz, new_npz, twin, out):
    P, N = np.load(parent_npz), np.load(new_npz)
    only = sorted(set(P.files) ^ set(N.files))
    if only:
        print("outputs that only one library produced: " + ", ".join(only), file=sys.stderr)
        return 1
    lines, bad, n_equal = [], 0, 0
    for key in sorted(P.files):
        p, n = P[key], N[key]
        if np.array_equal(p, n):
            n_equal += 1
            lines.append(f"{key} equal")
            continue
        largest = float(np.max(np.abs(p)))
        dev = float(np.max(np.abs(n - p))) / largest if largest > 0 else float("inf")
        verdict = twin_rule(key, p, n, largest) if twin else None
        if verdict is None:
            bad += 1
            lines.append(f"{key} DIFFERS max |new - parent| / max |parent| = {dev:.3e} (not judged against the twin)")
        else:
            ok, dp, dn = verdict
            bad += not ok
            lines.append(f"{key} differs {dev:.3e}; |parent - twin| = {dp:.3e}, |new - twin| = {dn:.3e}: {'within' if ok else 'OUTSIDE'} the rule")
    head = f"outputs: {len(P.files)}, bit-identical (np.array_equal): {n_equal}, failing: {bad}"
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join([head] + lines) + "\n")
    print(head)
    print("\n".join(l for l in lines if not l.endswith(" equal")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
