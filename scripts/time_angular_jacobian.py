"""Time LossFunction.angular_jacobian at the reference's ARTS size -- 1024 wavelength points x 241 angles, image rows 90:950, nvx 256
-- against what it replaces, and write profiles/angular_jacobian_timing.json:

  * ``scalars``: the six scalar leaves Te, ne, m, lam, amp1, amp2 (m through a direction of f_e) against 12 forward images, the
    central differences the call replaces (Engine.form_factor + Engine.ats_spectrum each);
  * ``fval``: the 256 directions of a free-form f_e (``fe: {type: arbitrary, dim: 1, active: true}``) in chunks of 32, against 512
    forward images (measured as 12 and scaled: every image costs the same).

Per part: the wall time of the call over a window of at least half a second between two device synchronisations, behind an untimed
spin of the same call (the clock warm-up of bench.py, --spin-ms), the median of --rounds rounds that alternate with the forward
images, and its kernel sum from the handle's timing ring (tsff_kernel_times: tsff_form_factor_jvp and tsff_ats_jvp
record one event pair per call).  The ratios are reported, not asserted: the call is wanted for exact tangents without a step size
and for the directions of f_e, not for speed.

``--two-d``: the same for a 2-D f_e at the reference's ARTS size -- a 128 x 128 table, 1024 x 241 points, the Mora-Yahi deck of the
reference's arts2v -- into profiles/angular_jacobian_2d_timing.json: ``scalars`` (the generator static: Te, ne, lam, amp1, amp2; no
table direction, so one saving forward and the tails) and ``generator`` (the three generator values too: three projections of a tangent
table more), each against the 2 n forward images of central differences (Engine.form_factor_2d + Engine.ats_spectrum), with the
same windows and warm-up."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def timed(fn, steps, spin_ms, window_ms=500.0):
    """ms per call: an untimed spin of the same call (clock warm-up), then a window of at least ``window_ms`` and ``steps`` calls
    between two device synchronisations."""
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
    steps = max(steps, int(np.ceil(window_ms * 1e-3 / max(one, 1e-6))))
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def part(free_form, args):
    import decks
    import util
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L
    from tsadar_amd.loss_function import LossFunction

    cfg = decks.deck_angular(1, 256)
    for k in ("amp1", "amp2"):
        cfg["parameters"]["general"][k]["active"] = True
    if free_form:
        cfg["parameters"]["electron"]["fe"] = {"active": True, "type": "arbitrary", "dim": 1, "nvx": 256, "params": {"init_m": 2.5}}
    sa = util._angular_sa(cfg)
    rows = 950 - 90
    rng = np.random.default_rng(1)
    batch = dict(e_data=1.0 + rng.uniform(0.0, 1.0, (rows, 1024)), i_data=np.zeros((rows, 1024)), e_amps=np.ones((rows, 1)),
                 i_amps=np.zeros(rows), noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    eng = lf.ts_diag.engine(True)
    lf.ts_diag._ats_prepare(eng, batch)
    phys = eng.dev(tp.physical_matrix())
    fe = eng.dev(np.asarray(tp()["electron"]["fe"], dtype=np.float64).reshape(1, -1))
    ea = eng.dev(np.ones(rows))
    p = tp.physical_matrix()[0]

    def image():
        return eng.ats_spectrum(eng.form_factor(0, phys, fe)[0], ea, p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2])

    def central():
        for _ in range(12):
            image()

    n = lf._angular_jacobian_device(tp, batch, args.chunk)[2].shape[0]
    jac = lambda: lf._angular_jacobian_device(tp, batch, args.chunk)
    out = dict(leaves=int(n), chunk=args.chunk)
    rounds = dict(forward_images_12_ms=[], angular_jacobian_ms=[])   # the two alternating, so that a drift of the machine hits both
    for _ in range(args.rounds):
        rounds["forward_images_12_ms"].append(timed(central, args.steps, args.spin_ms))
        rounds["angular_jacobian_ms"].append(timed(jac, args.steps, args.spin_ms))
    out["rounds"] = rounds
    for k, v in rounds.items():
        out[k] = float(np.median(v))
    eng.enable_timing(4096)
    jac()
    eng.torch.cuda.synchronize()
    out["kernel_sum_ms"] = float(np.sum(eng.kernel_times_ms()))
    images = 2 * n
    out["central_images"] = images
    out["central_ms"] = out["forward_images_12_ms"] * images / 12.0
    out["ratio"] = out["angular_jacobian_ms"] / out["central_ms"]
    return out


def part_2d(with_gen, args):
    import decks
    import util
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L
    from tsadar_amd.loss_function import LossFunction

    nv = 128
    cfg = decks.deck_angular(2, nv)
    for k in ("amp1", "amp2"):
        cfg["parameters"]["general"][k]["active"] = True
    cfg["parameters"]["electron"]["fe"] = {"active": bool(with_gen), "dim": 2, "type": "sphericalharmonic", "nvx": nv,
                                           "params": {"flm_type": "mora-yahi", "init_m": 2.2, "Nl": 1, "nvr": nv, "LTx": 225000.0, "LTy": 400000.0}}
    sa = util._angular_sa(cfg)
    rows = 950 - 90
    rng = np.random.default_rng(1)
    batch = dict(e_data=1.0 + rng.uniform(0.0, 1.0, (rows, 1024)), i_data=np.zeros((rows, 1024)), e_amps=np.ones((rows, 1)),
                 i_amps=np.zeros(rows), noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    eng = lf.ts_diag.engine(True)
    lf.ts_diag._ats_prepare(eng, batch)
    phys = eng.dev(tp.physical_matrix())
    fe2 = eng.dev(np.ascontiguousarray(tp()["electron"]["fe"], dtype=np.float64))
    ea = eng.dev(np.ones(rows))
    p = tp.physical_matrix()[0]
    gen = cfg["parameters"]["general"]
    ang = (gen["ud"]["angle"], gen["Va"]["angle"])
    n = lf._angular_jacobian_device(tp, batch, args.chunk)[2].shape[0]

    def image():
        return eng.ats_spectrum(eng.form_factor_2d(0, phys, fe2, *ang)[0], ea, p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2])

    def central():
        for _ in range(2 * n):
            image()

    jac = lambda: lf._angular_jacobian_device(tp, batch, args.chunk)
    out = dict(leaves=int(n), chunk=args.chunk, central_images=2 * int(n))
    rounds = dict(central_ms=[], angular_jacobian_ms=[], forward_image_ms=[])
    for _ in range(args.rounds):
        rounds["central_ms"].append(timed(central, args.steps, args.spin_ms))
        rounds["angular_jacobian_ms"].append(timed(jac, args.steps, args.spin_ms))
        rounds["forward_image_ms"].append(timed(image, args.steps, args.spin_ms))
    out["rounds"] = rounds
    for k, v in rounds.items():
        out[k] = float(np.median(v))
    eng.enable_timing(4096)
    jac()
    eng.torch.cuda.synchronize()
    out["kernel_sum_ms"] = float(np.sum(eng.kernel_times_ms()))
    out["ratio"] = out["angular_jacobian_ms"] / out["central_ms"]
    out["jacobian_in_forward_images"] = out["angular_jacobian_ms"] / out["forward_image_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--two-d", action="store_true", help="the 2-D f_e mode (profiles/angular_jacobian_2d_timing.json)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--spin-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "angular_jacobian_2d_timing.json" if args.two_d else "angular_jacobian_timing.json")
    if args.two_d:
        res = dict(device=torch.cuda.get_device_name(0), shape="npts 1024 x 241 angles, rows 90:950, table 128 x 128 (Mora-Yahi)",
                   steps=args.steps, spin_ms=args.spin_ms, rounds=args.rounds, scalars=part_2d(False, args), generator=part_2d(True, args))
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return

    res = dict(device=torch.cuda.get_device_name(0), shape="npts 1024 x 241 angles, rows 90:950, nvx 256", steps=args.steps,
               spin_ms=args.spin_ms, rounds=args.rounds, scalars=part(False, args), fval=part(True, args))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
