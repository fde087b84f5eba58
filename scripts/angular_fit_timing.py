"""Per-epoch wall time of the angular (ARTS) fit at the reference's full size (1024 x 1024 CCD, 860 lineout rows, 241 angles;
the shapes of scripts/time_angular.py): the host loop over LossFunction.vg_loss with tree.Adam against loops.angular_loop
(tsff_angular_fit), for a 1-D DLM deck (nvx 256), a 2-D Arbitrary2V deck (nvx 128, table trained), a 2-D constant-table
SphericalHarmonics deck (nvx 128) and the reference's arts2v deck: a TRAINED Mora-Yahi SphericalHarmonics generator (nvx 128,
nvr 64, rmsprop; angular_loop(train_generator=True) against the host loop, whose generator gradient is by central differences),
and the reference's arts1v deck with a TRAINED free-form 1-D f_e (Arbitrary1V, nvx 256, adam; train_generator=True against the
host loop, whose generator and chain rule run in NumPy).

Both figures count epochs only.  The host loop is timed after a warm-up evaluation, over windows of 10 epochs.  Every
angular_loop call builds its own LossFunction, engine and scratch, so its per-epoch time is the difference of two calls of N1
and N2 epochs over N2 - N1.  Both are the median over --repeats repetitions (default 1), with the smallest and largest beside it.

  --deck NAME        one deck only (dlm1d, arb2d, sph2d, sphtrain, arb1v)
  --repeats R        repetitions of each timed window
  --out FILE         deck arb1v: merge the figures into FILE (default profiles/arb1v_generator_timing.json)
  --device-only      angular_loop alone (run it under rocprofv3 --kernel-trace --output-format csv)
  --kernel-sum CSV   per-epoch kernel sum of such a trace: the durations of every kernel from one epoch's k_ang_leaves up to
                     the next one's, median over the epochs of the trace; generator_ms_per_epoch: the share of the trained generator's kernels
                     in it (k_sph_table and k_sph_vjp, or k_arb1v_matvec and k_arb1v_point)
Prints one JSON line per deck."""
import copy, csv, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

SPH = {"active": False, "dim": 2, "type": "sphericalharmonic", "nvx": 128,
       "params": {"flm_type": "mora-yahi", "init_m": 2.2, "LTx": 225000.0, "LTy": 400000.0, "Nl": 1, "nvr": 128}}
SPH_TRAIN = {"active": True, "dim": 2, "type": "sphericalharmonic", "nvx": 128,
             "params": {"flm_type": "mora-yahi", "init_m": 2.2, "LTx": 225000.0, "LTy": 400000.0, "Nl": 1, "nvr": 64}}
ARB1V = {"active": True, "dim": 1, "type": "arbitrary", "nvx": 256, "params": {"init_m": 2.5}}
DECKS = (("dlm1d", 1, 256), ("arb2d", 2, 128), ("sph2d", 2, 128), ("sphtrain", 2, 128), ("arb1v", 1, 256))
ARB1V_OUT = os.path.join(ROOT, "profiles", "arb1v_generator_timing.json")
N1, N2 = 16, 48


def kernel_sum(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    epochs, gens, cur, gen = [], [], None, 0
    for r in rows:
        if r["Kernel_Name"].startswith("void tsff::k_ang_leaves"):
            if cur is not None:
                epochs.append(cur)
                gens.append(gen)
            cur, gen = 0, 0
        if cur is not None:
            dt = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            cur += dt
            if "tsff::k_sph_" in r["Kernel_Name"] or "tsff::k_arb1v_" in r["Kernel_Name"]:
                gen += dt
    # (the last epoch of the trace is cut short by what follows it: dropped with the others' tail)
    return dict(kernel_ms_per_epoch=float(np.median(epochs)) * 1e-6, generator_ms_per_epoch=float(np.median(gens)) * 1e-6,
                epochs_in_trace=len(epochs))


def merge_into(path, section, values):
    """profiles/arb1v_generator_timing.json: one section (wall, kernel_trace) replaced, the rest kept"""
    doc = json.load(open(path)) if os.path.exists(path) else {
        "what": "trained free-form 1-D f_e (Arbitrary1V) fit at the reference's ARTS size: 1024 x 1024 CCD, 860 rows, 241 angles, "
                "nvx 256, adam (scripts/angular_fit_timing.py --deck arb1v); MI355X"}
    doc[section] = values
    if "wall" in doc and "kernel_trace" in doc:
        k = doc["kernel_trace"]
        k["generator_share_of_kernel_sum"] = k["generator_ms_per_epoch"] / k["kernel_ms_per_epoch"]
        doc["device_epoch_over_kernel_sum"] = doc["wall"]["angular_loop_ms_per_epoch"] / k["kernel_ms_per_epoch"]
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)), n=len(v))


def main():
    arg = lambda k, d=None: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else d
    if "--kernel-sum" in sys.argv:
        ks = kernel_sum(arg("--kernel-sum"))
        print(json.dumps(ks))
        if arg("--deck") == "arb1v":
            merge_into(arg("--out", ARB1V_OUT), "kernel_trace", ks)
        return
    import torch
    import decks
    from tsadar_amd import ThomsonParams, calibration, loops, tree
    from tsadar_amd.loss_function import LossFunction

    device_only = "--device-only" in sys.argv
    only, repeats = arg("--deck"), int(arg("--repeats", 1))
    for name, dim, nvx in DECKS:
        if only and name != only:
            continue
        cfg = decks.deck_angular(dim, nvx)
        if name in ("sph2d", "sphtrain"):
            cfg["parameters"]["electron"]["fe"] = copy.deepcopy(SPH if name == "sph2d" else SPH_TRAIN)
        if name == "arb1v":
            cfg["parameters"]["electron"]["fe"] = copy.deepcopy(ARB1V)
        train, rms = name in ("sphtrain", "arb1v"), name == "sphtrain"
        cfg["other"]["ang_res_unit"] = 1
        cfg["optimizer"].update(method="rmsprop" if rms else "adam", learning_rate=1e-4 if rms else 1e-3, save_state=False)
        cfg["other"]["extraoptions"]["spectype"] = "angular"
        sa = calibration.get_scattering_angles(cfg)
        cfg["other"]["extraoptions"]["spectype"] = "angular_full"
        sa["angAxis"] = calibration.angular_pixel_axis()
        a, b = cfg["data"]["lineouts"]["start"], cfg["data"]["lineouts"]["end"]
        batch = dict(e_data=np.ones((b - a, 1024)), i_data=np.zeros((b - a, 1024)), e_amps=np.ones((b - a, 1)), i_amps=np.zeros(b - a),
                     noise_e=np.array([0.0]), noise_i=np.array([0.0]))
        tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
        truth = tp.copy()
        truth.X[0, 0] -= 0.3
        e_data = np.ones((1024, 1024))
        e_data[a:b] = LossFunction(copy.deepcopy(cfg), sa, batch).ts_diag(truth, batch)[0]
        all_data = dict(e_data=e_data, e_amps=np.ones((1024, 1)), i_data=np.zeros((1024, 1024)), i_amps=np.zeros(1024),
                        noiseE=np.zeros((1024, 1024)), noiseI=np.zeros((1024, 1024)))
        out = dict(deck=name, nvx=nvx)
        if not device_only:
            lf = LossFunction(copy.deepcopy(cfg), sa, batch)
            batch1 = dict(batch, e_data=e_data[a:b])
            diff, static = tree.partition(tp, tree.get_filter_spec(cfg["parameters"], tp))
            opt = tree.RMSProp(1e-4) if rms else tree.Adam(1e-3)
            st = opt.init(diff)
            lf.vg_loss(diff, static, batch1)
            host = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    (v, aux), g = lf.vg_loss(diff, static, batch1)
                    u, st = opt.update(g, st)
                    diff = tree.apply_updates(diff, u)
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) / 10 * 1e3)
            out["host_loop_ms_per_epoch"] = float(np.median(host))
            out["host_loop_spread"] = spread(host)

        def run(n):
            c = copy.deepcopy(cfg)
            c["optimizer"]["num_epochs"] = n
            info = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loops.angular_loop(c, all_data, sa, info=info, train_generator=train)
            torch.cuda.synchronize()
            assert info["stopped_after"] is None, "the timing runs must not stop early"
            return time.perf_counter() - t0

        run(2)   # (warm-up: the library, torch's allocator)
        pairs = [(run(N1), run(N2)) for _ in range(repeats)]
        per = [(t2 - t1) / (N2 - N1) * 1e3 for t1, t2 in pairs]
        out["angular_loop_ms_per_epoch"] = float(np.median(per))
        out["angular_loop_spread"] = spread(per)
        out["angular_loop_setup_ms"] = float(np.median([t1 * 1e3 - N1 * p for (t1, _), p in zip(pairs, per)]))
        print(json.dumps(out), flush=True)
        if name == "arb1v" and not device_only:
            merge_into(arg("--out", ARB1V_OUT), "wall", {k: v for k, v in out.items() if k not in ("deck", "nvx")})


if __name__ == "__main__":
    main()
