"""Time LossFunction.angular_h_loss_wrt_params' device call (Engine.angular_loss_hess, tsff_angular_loss_hess) at the reference's
ARTS size -- 1024 wavelength points x 241 angles, image rows 90:950, nvx 256, leaves Te, ne, m, lam, amp1, amp2 -- and write
profiles/angular_hessian_timing.json:

  * ``angular_loss_hess_ms``: the wall time of the call over a window of at least half a second between two device synchronisations,
    behind an untimed spin of the same call (the clock warm-up of bench.py, --spin-ms);
  * ``kernel_sum_ms``: the device time of one call from the handle's timing ring (tsff_kernel_times: the call records one event pair
    around all its launches);
  * ``central_ms``: the same Hessian by 2 n central differences of the device gradient (LossFunction.vg_loss on the angular deck:
    _vg_angular_adjoint, one forward image, the ATS adjoint and the form-factor adjoint per gradient), the only route the parent commit
    has.  It is timed with the fit loss's constant denominators: the per-sample denominators |d| + 1e-10 of _loss_for_hess_fn_ change
    one element-wise factor of the seed, not a launch;
  * ``forward_image_ms``: one forward image (Engine.form_factor + Engine.ats_spectrum), the unit the pair sweeps are counted in.

The medians of --rounds rounds that alternate the three, so that a drift of the machine hits all of them.  The ratio is reported, not
asserted: the call is wanted because its Hessian is exact (a quotient of gradients crosses table cells) and shows a negative
curvature the Gauss-Newton matrix cannot."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tests"), ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from time_angular_jacobian import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--spin-ms", type=float, default=300.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "angular_hessian_timing.json"))
    args = ap.parse_args()
    import torch

    import decks
    import util
    from tsadar_amd import ThomsonParams, tree
    from tsadar_amd import _lib as L
    from tsadar_amd.loss_function import LossFunction

    cfg = decks.deck_angular(1, 256)
    for k in ("amp1", "amp2"):
        cfg["parameters"]["general"][k]["active"] = True
    sa = util._angular_sa(cfg)
    rows = 950 - 90
    rng = np.random.default_rng(1)
    batch = dict(e_data=1.0 + rng.uniform(0.0, 1.0, (rows, 1024)), i_data=np.zeros((rows, 1024)), e_amps=np.ones((rows, 1)),
                 i_amps=np.zeros(rows), noise_e=np.array([0.0]), noise_i=np.array([0.0]))
    lf = LossFunction(cfg, sa, batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    spec = tree.get_filter_spec(None, tp)
    names = [k for (_, k), _ in spec]
    act = [int(s) for _, s in spec]
    n = len(act)

    # the new call, on device-resident inputs (what LossFunction.angular_h_loss_wrt_params hands it)
    eng = lf.ts_diag.dlm_engine(True)
    lam_step = lf.ts_diag._ats_prepare(eng, batch)
    lamE = lf.ts_diag._ats_lam_axis(eng, lam_step)
    wcol = lf._angular_sum_wcol(lamE)
    x_d, d_d, ea_d, w_d = eng.dev(tp.X[0]), eng.dev(batch["e_data"]), eng.dev(np.ones(rows)), eng.dev(wcol)
    hess = lambda: eng.angular_loss_hess(x_d, act, d_d, None, ea_d, w_d, "l2")

    # the parent's route: 2 n gradients of the device adjoint
    diff, static = tree.partition(tp, spec)
    x0, lf.unravel_weights = tree.ravel_pytree(diff)
    h = 1e-6

    def central():
        for k in range(n):
            for sgn in (1.0, -1.0):
                x = x0.copy()
                x[k] += sgn * h
                lf.vg_loss(x, static, batch)

    eng1 = lf.ts_diag.engine(True)
    lf.ts_diag._ats_prepare(eng1, batch)
    phys = eng1.dev(tp.physical_matrix())
    fe = eng1.dev(np.asarray(tp()["electron"]["fe"], dtype=np.float64).reshape(1, -1))
    p = tp.physical_matrix()[0]
    image = lambda: eng1.ats_spectrum(eng1.form_factor(0, phys, fe)[0], ea_d, p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2])

    rounds = dict(angular_loss_hess_ms=[], central_ms=[], forward_image_ms=[])
    for _ in range(args.rounds):
        rounds["central_ms"].append(timed(central, args.steps, args.spin_ms))
        rounds["angular_loss_hess_ms"].append(timed(hess, args.steps, args.spin_ms))
        rounds["forward_image_ms"].append(timed(image, args.steps, args.spin_ms))
    res = dict(device=torch.cuda.get_device_name(0), shape="npts 1024 x 241 angles, rows 90:950, nvx 256", leaves=names,
               form_factor_pairs=sum(1 for a in range(n) for c in range(a, n) if all(act[i] not in (L.P_AMP1, L.P_AMP2, L.P_AMP3) for i in (a, c))),
               steps=args.steps, spin_ms=args.spin_ms, rounds=rounds)
    for k, v in rounds.items():
        res[k] = float(np.median(v))
    eng.enable_timing(64)
    hess()
    launched = eng.last_launch()   # (before the next entry point starts its own record)
    torch.cuda.synchronize()
    res["kernel_sum_ms"] = float(np.sum(eng.kernel_times_ms()))
    res["launches"] = {k: launched.count(k) for k in sorted(set(launched))}
    res["central_gradients"] = 2 * n
    res["central_note"] = ("central_ms times 2 n gradients of the fit loss (constant denominators e_norm^2): the per-sample denominators "
                           "|d| + 1e-10 of _loss_for_hess_fn_ change one element-wise factor of the seed, not a launch")
    res["ratio"] = res["angular_loss_hess_ms"] / res["central_ms"]
    res["hess_in_forward_images"] = res["angular_loss_hess_ms"] / res["forward_image_ms"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
