"""Per-epoch wall time of the angular (ARTS) fit at the reference's full size (1024 x 1024 CCD, 860 lineout rows, 241 angles;
the shapes of scripts/time_angular.py): the host loop over LossFunction.vg_loss with tree.Adam against loops.angular_loop
(tsff_angular_fit), for a 1-D DLM deck (nvx 256), a 2-D Arbitrary2V deck (nvx 128, table trained), a 2-D constant-table
SphericalHarmonics deck (nvx 128) and the reference's arts2v deck: a TRAINED Mora-Yahi SphericalHarmonics generator (nvx 128,
nvr 64, rmsprop; angular_loop(train_generator=True) against the host loop, whose generator gradient is by central differences).

Both figures count epochs only.  The host loop is timed after a warm-up evaluation.  Every angular_loop call builds its own
LossFunction, engine and scratch, so its per-epoch time is the difference of two calls of N1 and N2 epochs over N2 - N1.

  --deck NAME        one deck only (dlm1d, arb2d, sph2d, sphtrain)
  --device-only      angular_loop alone (run it under rocprofv3 --kernel-trace --output-format csv)
  --kernel-sum CSV   per-epoch kernel sum of such a trace: the durations of every kernel from one epoch's k_ang_leaves up to
                     the next one's, median over the epochs of the trace; generator_ms_per_epoch: the share of k_sph_table and
                     k_sph_vjp in it (the trained generator)
Prints one JSON line per deck."""
import copy, csv, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np

SPH = {"active": False, "dim": 2, "type": "sphericalharmonic", "nvx": 128,
       "params": {"flm_type": "mora-yahi", "init_m": 2.2, "LTx": 225000.0, "LTy": 400000.0, "Nl": 1, "nvr": 128}}
SPH_TRAIN = {"active": True, "dim": 2, "type": "sphericalharmonic", "nvx": 128,
             "params": {"flm_type": "mora-yahi", "init_m": 2.2, "LTx": 225000.0, "LTy": 400000.0, "Nl": 1, "nvr": 64}}
DECKS = (("dlm1d", 1, 256), ("arb2d", 2, 128), ("sph2d", 2, 128), ("sphtrain", 2, 128))
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
            if "tsff::k_sph_" in r["Kernel_Name"]:
                gen += dt
    # (the last epoch of the trace is cut short by what follows it: dropped with the others' tail)
    return dict(kernel_ms_per_epoch=float(np.median(epochs)) * 1e-6, generator_ms_per_epoch=float(np.median(gens)) * 1e-6,
                epochs_in_trace=len(epochs))


def main():
    if "--kernel-sum" in sys.argv:
        print(json.dumps(kernel_sum(sys.argv[sys.argv.index("--kernel-sum") + 1])))
        return
    import torch
    import decks
    from tsadar_amd import ThomsonParams, calibration, loops, tree
    from tsadar_amd.loss_function import LossFunction

    device_only = "--device-only" in sys.argv
    only = sys.argv[sys.argv.index("--deck") + 1] if "--deck" in sys.argv else None
    for name, dim, nvx in DECKS:
        if only and name != only:
            continue
        cfg = decks.deck_angular(dim, nvx)
        if name in ("sph2d", "sphtrain"):
            cfg["parameters"]["electron"]["fe"] = copy.deepcopy(SPH if name == "sph2d" else SPH_TRAIN)
        train = name == "sphtrain"
        cfg["other"]["ang_res_unit"] = 1
        cfg["optimizer"].update(method="rmsprop" if train else "adam", learning_rate=1e-4 if train else 1e-3, save_state=False)
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
            opt = tree.RMSProp(1e-4) if train else tree.Adam(1e-3)
            st = opt.init(diff)
            lf.vg_loss(diff, static, batch1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                (v, aux), g = lf.vg_loss(diff, static, batch1)
                u, st = opt.update(g, st)
                diff = tree.apply_updates(diff, u)
            torch.cuda.synchronize()
            out["host_loop_ms_per_epoch"] = (time.perf_counter() - t0) / 10 * 1e3

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
        t1, t2 = run(N1), run(N2)
        out["angular_loop_ms_per_epoch"] = (t2 - t1) / (N2 - N1) * 1e3
        out["angular_loop_setup_ms"] = (t1 - N1 * (t2 - t1) / (N2 - N1)) * 1e3
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
