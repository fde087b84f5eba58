"""The edges of the W and Z' tables on the GPU.  The pair-sweep kernels and the two-sweep kernel clamp a position into the table, take
the cell by floor and the weight by subtraction, and select the asymptote of Z' outside its table; any other form of those lookups
(fract / truncation, a pad cell for the zeros of Im Z' -- both measured and left out) has to give the same bits
exactly here.  The same decks run through the one-sweep kernel, tsff_forward and the two-sweep kernel.

Two lineouts, 10 angles, cold plasma (T_e 0.2 - 0.3 keV, T_i 20 - 50 eV), chosen with the oracle alone so that the sweeps meet

  xi_e   left of -8.2 (the clamp puts it ON node 0: t = 0 exactly), right of 8.19, in the first and in the last cell of the table
         (EPW sweep; the IAW sweep stays inside)
  xi_i   inside the Z' table, beyond both of its ends, in its last cell (IAW sweep), beyond the table with |xi_i| < 28 (general units:
         the pad cell) and with |xi_i| > 28 over whole 128-sample units (asymptotic units, EPW sweep)

(An interior node cannot be met on purpose: xi_e reaches the lookup through an activation, two square roots and a division.)
Every class is asserted non-empty, here and again in the GPU test.  nvx = 128 runs the full Z' table; the half table is not a plan bit
of the one-sweep kernel -- the planner takes it when the LDS budget asks for it -- so the second case is the same deck at nvx = 256,
where it does (tests/test_kernel_matrix.py pins k_spectrum_fused<1, 0, true, true> there).

Reference: the C++ oracle with the suite's bounds (spectra 1e-8 EPW / 1e-7 IAW, loss sums 1e-9, gradient columns 1e-6 of the column's
largest entry); spectra bit-identical across the three kernels, gradients of the two loss kernels to 1e-12; samples 0, 511, 512 and
1023 -- the ends and the pair boundary of the pair sweeps -- on their own."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

CASES = {"full_nvx128": dict(nvx=128, zh="false"), "half_nvx256": dict(nvx=256, zh="true")}
B = 2
ACTIVE = ("Te", "ne", "Ti", "Va", "ud", "lam", "amp1", "amp2")
EDGE_SAMPLES = (0, 511, 512, 1023)
XI_LO, XI_HI, XI_H = -8.2, 8.19, 0.01   # the tables' domain [-8.2, 8.19] and spacing (xi2)


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = decks.deck_fit(nvx=CASES[name]["nvx"], active=ACTIVE)
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=1500)
    normed = util.random_lineouts(cfg, B, seed=5, ranges=dict(Te=(0.2, 0.3), Ti_1=(0.02, 0.05)))
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, X=util.normed_to_matrix(normed, 1))


def _classes(name):
    s = _case(name)
    phys = orc.physical_params(s["cfg"]["parameters"], s["normed"], True)
    n = dict.fromkeys(("xe_left", "xe_right", "xe_first_cell", "xe_last_cell", "xi_inside", "xi_left", "xi_right", "xi_last_cell",
                       "xi_outside_general", "asymptotic_units", "general_units"), 0)
    cnt = lambda a, lo, hi: int(((a >= lo) & (a < hi)).sum())
    for b in range(B):
        p = orc.lineout_params(phys, b, 1)
        for f in (0, 1):
            xe, xi = util.positions(s["cfg"], s["sa"], p, f)
            assert xe.shape == (1024, 10)
            if f == 0:
                n["xe_left"] += int((xe < XI_LO).sum()); n["xe_right"] += int((xe > XI_HI).sum())
                n["xe_first_cell"] += cnt(xe, XI_LO, XI_LO + XI_H); n["xe_last_cell"] += cnt(xe, XI_HI - XI_H, XI_HI)
            else:
                n["xi_inside"] += cnt(xi, XI_LO, XI_HI); n["xi_left"] += int((xi < XI_LO).sum()); n["xi_right"] += int((xi > XI_HI).sum())
                n["xi_last_cell"] += cnt(xi, XI_HI - XI_H, XI_HI)
                n["xi_outside_general"] += int((((xi < XI_LO) | (xi > XI_HI)) & (np.abs(xi) < 28.0)).sum())
            far = (np.abs(xi) > 1.02 * 28.0).reshape(8, 128, -1).all(axis=(1, 2))   # the 128-sample units of the pair sweeps
            n["asymptotic_units"] += int(far.sum()); n["general_units"] += int((~far).sum())
    return n


@pytest.mark.parametrize("name", sorted(CASES))
def test_sweeps_reach_the_table_edges(name):
    """Oracle alone (no GPU): every class of position is met."""
    n = _classes(name)
    print(name, n)
    for k, v in n.items():
        assert v > 0, (name, k, n)


@functools.lru_cache(maxsize=None)
def _reference(name, w):
    from oracle import c_oracle as co
    from tsadar_amd.params import SlotMap

    s = _case(name)
    gm = SlotMap(s["cfg"]["parameters"], True).active.astype(np.uint8)
    sums, gref, Eo, Io = co.loss_grad(s["cfg"], s["sa"], s["X"], s["batch"], w=np.array(w), gmask=gm)
    return dict(sums=sums.sum(axis=0), grad=gref, E=Eo, I=Io, gm=gm)


def _elementwise(a, b, floor=1e-12):
    """util.rel_err's measure, per element"""
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b) / np.maximum(np.abs(b), floor * np.max(np.abs(b), axis=-1, keepdims=True))


def _check_spectra(tag, E, I, ref):
    eE, eI = _elementwise(E, ref["E"]), _elementwise(I, ref["I"])
    print(tag, "spectra: EPW %.3e IAW %.3e" % (eE.max(), eI.max()),
          "samples", {j: (float(eE[:, j].max()), float(eI[:, j].max())) for j in EDGE_SAMPLES})
    assert eE.max() < 1e-8 and eI.max() < 1e-7, (tag, eE.max(), eI.max())
    for j in EDGE_SAMPLES:
        assert np.all(ref["E"][:, j] != 0.0) and np.all(ref["I"][:, j] != 0.0)
        assert eE[:, j].max() < 1e-8, (tag, "EPW", j, eE[:, j])
        assert eI[:, j].max() < 1e-7, (tag, "IAW", j, eI[:, j])


def _check_loss_grad(tag, ref, terms, grad):
    gm = ref["gm"]
    print(tag, "loss sums", terms, ref["sums"])
    np.testing.assert_allclose(terms, ref["sums"], rtol=1e-9)
    for sl in np.nonzero(gm)[0]:
        err = np.max(np.abs(grad[:, sl] - ref["grad"][:, sl])) / np.max(np.abs(ref["grad"][:, sl]))
        print(tag, "grad column", sl, "%.3e" % err)
        assert err < 1e-6, (tag, sl, grad[:, sl], ref["grad"][:, sl])
    assert np.all(grad[:, gm == 0] == 0.0)
    assert np.all(grad[:, gm != 0] != 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_table_edges_against_oracle(name):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    n = _classes(name)
    assert min(n.values()) > 0, n
    s = _case(name)
    eng = Engine(s["cfg"], s["sa"])
    w = eng.loss_weights(B, s["i_norm"], s["e_norm"], s["cfg"]["data"]["ion_loss_scale"])
    ref = _reference(name, tuple(float(v) for v in w))
    gm = eng.slots.active.astype(np.uint8)
    assert np.array_equal(gm, ref["gm"])
    kernel = {0: "k_spectrum_fused<1, 0, %s, true>" % CASES[name]["zh"], 2: "k_spectrum<1, 1, 0, "}
    out = {}
    for plan in (0, 2):
        eng.set_launch_plan(plan)
        terms, grad, E, I = eng.loss_grad(s["X"], s["batch"], w, gm, want_spectra=True)
        torch.cuda.synchronize()
        launched = eng.last_launch()
        print(name, "plan", plan, launched)
        assert any(k.startswith(kernel[plan]) for k in launched), (plan, launched)
        out[plan] = [a.cpu().numpy() for a in (terms, grad, E, I)]
        tag = "%s plan %d" % (name, plan)
        _check_spectra(tag, out[plan][2], out[plan][3], ref)
        _check_loss_grad(tag, ref, out[plan][0], out[plan][1])
    eng.set_launch_plan(0)
    b = s["batch"]
    Ef, If = eng.forward(s["X"], b["e_amps"], b["i_amps"], b["noise_e"], b["noise_i"])
    torch.cuda.synchronize()
    launched = eng.last_launch()
    print(name, "forward", launched)
    assert any(k.startswith("k_forward_pairs<1, ") for k in launched), launched
    Ef, If = Ef.cpu().numpy(), If.cpu().numpy()
    _check_spectra(name + " forward", Ef, If, ref)
    # the three kernels: the same bits
    np.testing.assert_array_equal(out[0][2], out[2][2])
    np.testing.assert_array_equal(out[0][3], out[2][3])
    np.testing.assert_array_equal(out[0][2], Ef)
    np.testing.assert_array_equal(out[0][3], If)
    np.testing.assert_array_equal(out[0][0], out[2][0])
    np.testing.assert_allclose(out[0][1], out[2][1], rtol=1e-12, atol=1e-15 * np.abs(out[0][1]).max())
