"""The angle records of the one-sweep kernel on the GPU.

k_fused_prep writes, per (lineout, feature) item, the pairs (cos theta_a, w_a pref) of the item's angles; the angle loops of
k_spectrum_fused fetch the pair of the next iteration by one scalar load instead of reading both constants from LDS, multiplying
by pref and moving the results to SGPRs in every iteration.  The two-sweep kernel (launch plan bit 1) keeps its LDS constants
and its own product: the same deck runs through both, through tsff_loss_grad and tsff_loss_grad_packed, and against the oracle.

Shapes, the smallest at which the record can be indexed wrongly:
  B = 3 and B = 65      k_fused_prep runs 64 items per workgroup: a partial last workgroup with one and with two loaded features
  n_angles 1, 2, 10, 16 the prefetch reads entry min(a + 1, n_angles - 1): one entry, the last entry, the benchmark's ten, the
                        most the lane-exchange kernel takes
  n_angles 17           the kernel without the lane exchange reads the same record
  one feature alone     grid B, feature f0, item = lineout (electron feature, ion feature)
  two DLM column blocks set_dlm_blocks(2) at B = 4, and at B = 257: a column block holds a multiple of 256 lineouts, so only there
                        does a second launch cover lineouts [b0, b0 + B) of Btot with b0 = 256 > 0 and read the record at the
                        item of the whole batch (B = 4 stays one block).  257 lineouts are too many for the autodiff twin: that
                        case is held bit for bit against the unblocked launch, against the two-sweep kernel (spectra and loss
                        sums bit for bit, the gradient to 1e-9, see there), and against the twin on the lineouts 0, 255 (last of
                        block 0) and 256 (block 1) -- with the loss weights of a batch of three, so that their gradient rows
                        are the twin's

Bounds: spectra and the three loss sums bit-identical between the kernels, gradients to 1e-12 (as test_launch_plans_agree has
it); against the oracle the suite's bounds (tests/test_gpu_parity.py): spectra 1e-8 (EPW) / 1e-7 (IAW), loss sums 1e-9, gradient
columns 1e-6 of the column's largest entry -- the DLM case against the autodiff twin (loss 1e-9, gradient 1e-7 of the largest
entry), which differentiates the DLM order.  One reference per case."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

# name -> (n_angles, B, electron feature, ion feature, DLM column blocks)
CASES = {
    "nang10_B3": (10, 3, True, True, 0),
    "nang1_B3": (1, 3, True, True, 0),
    "nang2_B65": (2, 65, True, True, 0),
    "nang16_B3": (16, 3, True, True, 0),
    "nang17_B3": (17, 3, True, True, 0),
    "nang10_B65_ele": (10, 65, True, False, 0),
    "nang10_B3_ion": (10, 3, False, True, 0),
    "nang10_B4_dlm2": (10, 4, True, True, 2),
}
DLM_NAMES = ["Te", "ne", "m", "amp1", "amp2", "lam"]


@functools.lru_cache(maxsize=None)
def _case(name):
    nang, B, ele, ion, blocks = CASES[name]
    dlm = blocks > 0
    cfg = decks.deck_fit(active=tuple(DLM_NAMES), m=2.7) if dlm else decks.deck_fit()
    sa = dict(sa=np.linspace(53.6, 66.1, nang), weights=np.ones((B, nang)) / nang)
    seed = 1200 + 10 * sorted(CASES).index(name)
    # (data and norms of the two-feature deck, as test_rows_kernel_single_feature takes them)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed)
    normed = util.random_lineouts(cfg, B, seed=seed + 1, ranges=dict(m=(2.05, 4.4)) if dlm else None)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    ext = cfg["other"]["extraoptions"]
    ext["load_ele_spec"], ext["load_ion_spec"] = ele, ion
    ext["fit_EPWb"] = ext["fit_EPWr"] = ele
    ext["fit_IAW"] = ion
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, B=B, dlm=dlm, X=util.normed_to_matrix(normed, 1))


@functools.lru_cache(maxsize=None)
def _reference(name, w):
    s = _case(name)
    from tsadar_amd.params import SlotMap

    gm = SlotMap(s["cfg"]["parameters"], True).active.astype(np.uint8)
    if s["dlm"]:
        from oracle import tsadar_oracle_torch as ot

        val, ref, Eo, Io = ot.value_and_grad(s["cfg"], s["sa"], s["normed"], s["batch"], s["i_norm"], s["e_norm"], DLM_NAMES)
        return dict(val=val, named=ref, E=np.asarray(Eo), I=np.asarray(Io), gm=gm)
    from oracle import c_oracle as co

    sums, gref, Eo, Io = co.loss_grad(s["cfg"], s["sa"], s["X"], s["batch"], w=np.array(w), gmask=gm)
    return dict(sums=sums.sum(axis=0), grad=gref, E=Eo, I=Io, gm=gm)


def _against_oracle(tag, s, ref, w, terms, grad, E, I, ele, ion):
    if ele:
        e = util.rel_err(E, ref["E"])
        print(tag, "EPW %.3e" % e)
        assert e < 1e-8, (tag, e)
    if ion:
        e = util.rel_err(I, ref["I"])
        print(tag, "IAW %.3e" % e)
        assert e < 1e-7, (tag, e)
    gm = ref["gm"]
    if s["dlm"]:
        val = float(np.dot(terms, w))
        print(tag, "loss", val, ref["val"])
        assert abs(val - ref["val"]) < 1e-9 * abs(ref["val"]), (tag, val, ref["val"])
        G = util.matrix_to_named(grad, DLM_NAMES)
        scale = max(np.max(np.abs(v)) for v in ref["named"].values())
        for k in DLM_NAMES:
            err = np.max(np.abs(G[k] - ref["named"][k])) / scale
            print(tag, "grad", k, "%.3e" % err)
            assert err <= 1e-7, (tag, k, G[k], ref["named"][k])
    else:
        print(tag, "loss sums", terms, ref["sums"])
        np.testing.assert_allclose(terms, ref["sums"], rtol=1e-9)
        floor = 1e-12 * np.max(np.abs(ref["grad"]))
        for sl in np.nonzero(gm)[0]:
            top = np.max(np.abs(ref["grad"][:, sl]))
            if top < floor:   # (a leaf the loaded feature does not depend on to working precision -- T_i with the electron feature alone,
                #  1e-22 beside 1e-1: rounding noise in the oracle and in the kernel alike)
                assert np.max(np.abs(grad[:, sl])) < floor, (tag, sl, grad[:, sl])
                continue
            err = np.max(np.abs(grad[:, sl] - ref["grad"][:, sl])) / top
            print(tag, "grad column", sl, "%.3e" % err)
            assert err < 1e-6, (tag, sl, grad[:, sl], ref["grad"][:, sl])
    assert np.all(grad[:, gm == 0] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_angle_records_against_two_sweep_kernel_and_oracle(name):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    nang, B, ele, ion, blocks = CASES[name]
    s = _case(name)
    eng = Engine(s["cfg"], s["sa"])
    w = eng.loss_weights(B, s["i_norm"], s["e_norm"], s["cfg"]["data"]["ion_loss_scale"])
    ref = _reference(name, tuple(float(v) for v in w))
    gm = eng.slots.active.astype(np.uint8)
    assert np.array_equal(gm, ref["gm"])
    act = [int(k) for k in np.nonzero(gm)[0]]
    gmn = int(s["dlm"])
    kernel = {0: "k_spectrum_fused<1, %d, false, %s>" % (gmn, "true" if nang <= 16 else "false"), 2: "k_spectrum<1, 1, %d, " % gmn}
    out = {}
    for plan in (0, 2):
        eng.set_launch_plan(plan)
        if blocks and plan == 0:
            eng.set_dlm_blocks(blocks)
        t, g, E, I = eng.loss_grad(s["X"], s["batch"], w, gm, want_spectra=True)
        torch.cuda.synchronize()
        launched = eng.last_launch()
        print(name, "plan", plan, launched)
        assert any(k.startswith(kernel[plan]) for k in launched), (plan, launched)
        if plan == 0:   # (one k_fused_prep for the whole batch, whatever the column blocks; B = 4 is one block, see above)
            assert sum(k.startswith("k_fused_prep<") for k in launched) == 1, launched
        packed, Ep, Ip = eng.loss_grad_packed(s["X"], s["batch"], w, gm, act, want_spectra=True)
        torch.cuda.synchronize()
        assert any(k.startswith(kernel[plan]) for k in eng.last_launch()), (plan, eng.last_launch())
        eng.set_dlm_blocks(0)
        out[plan] = [a.cpu().numpy() for a in (t, g, E, I, packed, Ep, Ip)]
    eng.set_launch_plan(0)
    t0, g0, E0, I0, p0, Ep0, Ip0 = out[0]
    t2, g2, E2, I2, p2, Ep2, Ip2 = out[2]
    # the two kernels: spectra and loss sums bit for bit, gradients to 1e-12
    np.testing.assert_array_equal(E0, E2)
    np.testing.assert_array_equal(I0, I2)
    np.testing.assert_array_equal(t0, t2)
    np.testing.assert_allclose(g0, g2, rtol=1e-12, atol=1e-15 * np.abs(g0).max())
    # the packed entry point: the same spectra, sums and gradient entries from either kernel
    for p, t, g, Ep, Ip in ((p0, t0, g0, Ep0, Ip0), (p2, t2, g2, Ep2, Ip2)):
        np.testing.assert_array_equal(Ep, E0)
        np.testing.assert_array_equal(Ip, I0)
        np.testing.assert_array_equal(p[:3], t)
        np.testing.assert_array_equal(p[3:].reshape(len(act), B), g[:, act].T)
    assert np.abs(g0).max() > 0.0
    _against_oracle(name + " one-sweep", s, ref, w, t0, g0, E0, I0, ele, ion)
    _against_oracle(name + " two-sweep", s, ref, w, t2, g2, E2, I2, ele, ion)


@pytest.mark.gpu
def test_angle_records_second_column_block():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from oracle import tsadar_oracle_torch as ot
    from tsadar_amd.engine import Engine

    B, sub = 257, [0, 255, 256]
    cfg = decks.deck_fit(active=tuple(DLM_NAMES), m=2.7)
    sa = dict(sa=np.linspace(53.6, 66.1, 10), weights=np.ones((B, 10)) / 10)
    batch = util.synthetic_batch(cfg, sa, B, seed=1400)
    normed = util.random_lineouts(cfg, B, seed=1401, ranges=dict(m=(2.05, 4.4)))
    X = util.normed_to_matrix(normed, 1)
    batch3 = {k: np.asarray(v)[sub] for k, v in batch.items()}
    normed3 = {k: np.asarray(v)[sub] for k, v in normed.items()}
    sa3 = dict(sa=sa["sa"], weights=sa["weights"][sub])
    i_norm, e_norm = orc.loss_norms(cfg, batch3)
    val, named, Eo, Io = ot.value_and_grad(cfg, sa3, normed3, batch3, i_norm, e_norm, DLM_NAMES)
    eng = Engine(cfg, sa)
    w = eng.loss_weights(len(sub), i_norm, e_norm, cfg["data"]["ion_loss_scale"])   # (the twin's batch: three lineouts)
    gm = eng.slots.active.astype(np.uint8)
    out = {}
    for tag, plan, blocks in (("blocks", 0, 2), ("one launch", 0, 0), ("two-sweep", 2, 0)):
        eng.set_launch_plan(plan)
        eng.set_dlm_blocks(blocks)
        res = eng.loss_grad(X, batch, w, gm, want_spectra=True)
        torch.cuda.synchronize()
        launched = eng.last_launch()
        print(tag, launched)
        n_fused = sum(k.startswith("k_spectrum_fused<1, 1, false, true>") for k in launched)
        assert n_fused == {"blocks": 2, "one launch": 1, "two-sweep": 0}[tag], launched
        out[tag] = [a.cpu().numpy() for a in res]
    eng.set_dlm_blocks(0)
    eng.set_launch_plan(0)
    for a, b in zip(out["blocks"], out["one launch"]):
        np.testing.assert_array_equal(a, b)
    t, g, E, I = out["blocks"]
    t2, g2, E2, I2 = out["two-sweep"]
    np.testing.assert_array_equal(E, E2)
    np.testing.assert_array_equal(I, I2)
    np.testing.assert_array_equal(t, t2)
    # The gradient against the two-sweep kernel.  The cases above hold it to 1e-12 at the batch sizes the issue names.  An entry is a sum
    # over 2 x 10 240 points that the two kernels add in different orders: N eps = 20 480 x 1.1e-16 = 2.3e-12 of the sum of the terms'
    # magnitudes, which cancellation among the terms -- 257 random DLM lineouts meet more of it than three do -- can leave two to three
    # decades above the entry itself.  Bound: 1e-9 of the entry, or 1e-12 of the gradient's largest entry for entries that nearly cancel.
    dg = np.abs(g - g2)
    print("gradient, one-sweep against two-sweep: max relative %.3e, max absolute / largest entry %.3e" %
          (np.max(dg / np.maximum(np.abs(g2), 1e-300)), dg.max() / np.abs(g2).max()))
    np.testing.assert_allclose(g, g2, rtol=1e-9, atol=1e-12 * np.abs(g2).max())
    eE, eI = util.rel_err(E[sub], Eo), util.rel_err(I[sub], Io)
    print("spectra of lineouts", sub, "EPW %.3e IAW %.3e" % (eE, eI))
    assert eE < 1e-8 and eI < 1e-7, (eE, eI)
    G = util.matrix_to_named(g[sub], DLM_NAMES)
    scale = max(np.max(np.abs(v)) for v in named.values())
    for k in DLM_NAMES:
        err = np.max(np.abs(G[k] - named[k])) / scale
        print("grad", k, "%.3e" % err)
        assert err <= 1e-7, (k, G[k], named[k])
