"""The scheduled order of the one-sweep kernel's angle loops on the GPU (r13_sweep_sched: pair_step_sched, k_pairs.inc).

k_spectrum_fused<1, 0, ., true> evaluates the two base points of a pair together, requests every table read ahead of arithmetic that
does not need it, and takes the unit's boundary point and k_s at other places than the parent did.  The order changes no arithmetic:
the same decks run through the one-sweep kernel, through the two-sweep kernel (set_launch_plan(2): k_spectrum, which the change does
not touch), through tsff_forward, and against the autodiff twin of the oracle.

Shapes, all at B = 3 -- the smallest at which the order can go wrong:
  n_angles 1, 2, 10, 16   the first and the last iteration of the angle loop, the scalar pointer's clamp at the last entry
  n_angles 17             the lane exchange off: the parent's order (the kernel without EX is not given the new one)
  line_pair0 / line_pair1 / line_none
                          EPW windows that put the laser line into a 128-sample unit of the thread's first pair (samples 0 - 511),
                          of its second pair (512 - 1023) and into neither, so that wavefronts run every (far0, far1) combination
                          of the general and the asymptotic loop; both features loaded, and each alone
  samples 511, 512, 1023  the pair boundary and the one sample without a right neighbour (has_next false only there): compared on
                          their own besides the whole spectra
  out_of_grid             T_e in [0.6, 1.0] keV and a drift: xi_e left and right of the velocity grid, the Hermite table's pad cell
  half_zp                 nvx = 256, where the planner takes the half Z' table (k_spectrum_fused<1, 0, true, true>); the others run the full one
The DLM order as a leaf and two ion species keep the parent's order (kSweepSched) and are not run here.

Bounds: spectra and the three loss sums bit for bit between the kernels, and the spectra bit for bit from tsff_forward; gradients
between the kernels at the tolerance of test_launch_plans_agree (rtol 1e-12, atol 1e-15 of the largest entry); against the twin
the suite's bounds for it (spectra 1e-8 EPW / 1e-7 IAW, loss 1e-9, gradient 1e-7 of the largest entry).  One reference per case."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

# the leaves of test_launch_plans_agree's deck (whose gradient tolerance this test takes); the drift only where the case needs it
ACTIVE = ("Te", "ne", "Ti", "Va", "lam", "amp1")
LEAVES = {"Te": "Te", "ne": "ne", "Ti": "Ti_1", "Va": "Va", "ud": "ud", "lam": "lam", "amp1": "amp1", "amp2": "amp2"}
B = 3
EDGE_SAMPLES = (511, 512, 1023)
# name -> n_angles, EPW window (nm; None: the deck's 400 - 700, laser line at sample 431), electron feature, ion feature, nvx, ranges
CASES = {
    "nang1": dict(nang=1), "nang2": dict(nang=2), "nang10": dict(nang=10), "nang16": dict(nang=16), "nang17": dict(nang=17),
    "line_pair0": dict(window=(400.0, 700.0)), "line_pair1": dict(window=(300.0, 600.0)), "line_none": dict(window=(535.0, 700.0)),
    "line_pair1_ele": dict(window=(300.0, 600.0), ion=False), "line_none_ele": dict(window=(535.0, 700.0), ion=False),
    "ion_alone": dict(ele=False),
    "out_of_grid": dict(ranges=dict(Te=(0.6, 1.0), ud=(-8.0, 8.0)), active=ACTIVE + ("ud",)),
    "half_zp": dict(nvx=256),
}


def _line_sample(cfg):
    lo, hi = cfg["other"]["lamrangE"]
    return (526.5 - lo) / (hi - lo) * (cfg["other"]["npts"] - 1)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = dict(nang=10, window=None, ele=True, ion=True, nvx=128, ranges=None, active=ACTIVE)
    c.update(CASES[name])
    cfg = decks.deck_fit(nvx=c["nvx"], active=c["active"])
    if c["window"]:
        r = cfg["data"]["fit_rng"]
        r["forward_epw_start"], r["forward_epw_end"] = c["window"]
        if c["window"][0] > 510.0:   # (the blue fit range of the deck lies left of this window: both ranges right of the line)
            r["blue_min"], r["blue_max"], r["red_min"], r["red_max"] = 540.0, 570.0, 580.0, 625.0
        decks.finish(cfg)
    sa = dict(sa=np.linspace(53.6, 66.1, c["nang"]), weights=np.ones((B, c["nang"])) / c["nang"])
    seed = 1300 + 10 * sorted(CASES).index(name)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed)
    normed = util.random_lineouts(cfg, B, seed=seed + 1, ranges=c["ranges"])
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    ext = cfg["other"]["extraoptions"]
    ext["load_ele_spec"], ext["load_ion_spec"] = c["ele"], c["ion"]
    ext["fit_EPWb"] = ext["fit_EPWr"] = c["ele"]
    ext["fit_IAW"] = c["ion"]
    return dict(c, names=[LEAVES[k] for k in c["active"]], cfg=cfg, sa=sa, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, X=util.normed_to_matrix(normed, 1))


def test_windows_put_the_line_where_the_cases_say():
    """No GPU: the laser line's sample under the three EPW windows."""
    at = {k: _line_sample(_case(k)["cfg"]) for k in ("line_pair0", "line_pair1", "line_none")}
    print(at)
    assert 0 <= at["line_pair0"] < 512 and 512 <= at["line_pair1"] < 1024 and at["line_none"] < 0


@functools.lru_cache(maxsize=None)
def _twin(name):
    from oracle import tsadar_oracle_torch as ot

    s = _case(name)
    val, named, Eo, Io = ot.value_and_grad(s["cfg"], s["sa"], s["normed"], s["batch"], s["i_norm"], s["e_norm"], s["names"])
    return dict(val=val, named=named, E=np.asarray(Eo), I=np.asarray(Io))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scheduled_sweep_against_two_sweep_forward_and_twin(name):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    s = _case(name)
    eng = Engine(s["cfg"], s["sa"])
    w = eng.loss_weights(B, s["i_norm"], s["e_norm"], s["cfg"]["data"]["ion_loss_scale"])
    gm = eng.slots.active.astype(np.uint8)
    zh = "true" if name == "half_zp" else "false"
    kernel = {0: "k_spectrum_fused<1, 0, %s, %s>" % (zh, "true" if s["nang"] <= 16 else "false"), 2: "k_spectrum<1, 1, 0, "}
    out = {}
    for plan in (0, 2):
        eng.set_launch_plan(plan)
        res = eng.loss_grad(s["X"], s["batch"], w, gm, want_spectra=True)
        torch.cuda.synchronize()
        launched = eng.last_launch()
        print(name, "plan", plan, launched)
        assert any(k.startswith(kernel[plan]) for k in launched), (plan, launched)
        out[plan] = [a.cpu().numpy() for a in res]
    eng.set_launch_plan(0)
    Ef, If = eng.forward(s["X"], s["batch"]["e_amps"], s["batch"]["i_amps"], s["batch"]["noise_e"], s["batch"]["noise_i"])
    Ef, If = Ef.cpu().numpy(), If.cpu().numpy()
    (t0, g0, E0, I0), (t2, g2, E2, I2) = out[0], out[2]
    feats = [("EPW", E0, E2, Ef, 1e-8, "E")] * s["ele"] + [("IAW", I0, I2, If, 1e-7, "I")] * s["ion"]
    for tag, a0, a2, af, _, _ in feats:
        for j in EDGE_SAMPLES:
            assert np.array_equal(a0[:, j], a2[:, j]) and np.array_equal(a0[:, j], af[:, j]), (name, tag, j, a0[:, j], a2[:, j], af[:, j])
        np.testing.assert_array_equal(a0, a2)
        np.testing.assert_array_equal(a0, af)
    np.testing.assert_array_equal(t0, t2)
    assert np.abs(g0).max() > 0.0
    print(name, "gradient, one-sweep against two-sweep: max |difference| / largest entry %.3e" % (np.abs(g0 - g2).max() / np.abs(g0).max()))
    np.testing.assert_allclose(g0, g2, rtol=1e-12, atol=1e-15 * np.abs(g0).max())
    assert np.all(g0[:, gm == 0] == 0.0)
    ref = _twin(name)
    for tag, a0, _, _, tol, key in feats:
        e = util.rel_err(a0, ref[key])
        print(name, tag, "against the twin %.3e" % e)
        assert e < tol, (name, tag, e)
    val = float(np.dot(t0, w))
    print(name, "loss", val, ref["val"])
    assert abs(val - ref["val"]) < 1e-9 * abs(ref["val"]), (name, val, ref["val"])
    G = util.matrix_to_named(g0, s["names"])
    scale = max(np.max(np.abs(v)) for v in ref["named"].values())
    for k in s["names"]:
        err = np.max(np.abs(G[k] - ref["named"][k])) / scale
        print(name, "grad", k, "%.3e" % err)
        assert err <= 1e-7, (name, k, G[k], ref["named"][k])
