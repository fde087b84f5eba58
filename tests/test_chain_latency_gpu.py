"""The one-sweep kernel's grouped wavefront sums on the GPU.

k_spectrum_fused sums its five mid-chain values and its 9 + 3 n_ion lineout-scalar adjoints over a wavefront by reduce-scatter
(wave_sums_scatter, tsff_device.h; the schedule: wave_scatter.h, modelled in tests/test_reduce_scatter_model.py): sum k ends in one
group of four lanes, whose first lane stores it.  No bit may move: the additions are the butterfly's.  (The issue's third item, the ion
feature's workgroups dispatched first behind a launch-plan bit, measured nothing and was taken out again, DESIGN.md section 4.1b: there
is one order of dispatch, and no second one to compare with.)

Shapes, the smallest at which this can go wrong:
  B = 1, 3, 65, 257     one item per feature (one workgroup per half of the grid), a partial k_fused_prep workgroup with one and with two
                        features, and more than 256 lineouts (a second k_fused_finish workgroup)
  both features         the interleaved grid 2B; each feature alone: grid B, item = lineout
  n_angles 1, 10, 16    the kernel with the lane exchange; 17: the one without it (the same chain)

Per case, from one engine: tsff_loss_grad and tsff_loss_grad_packed twice.  The two runs of each are equal bit for bit (loss sums,
gradient, spectra, packed buffer), the packed buffer -- called with
B_global = B + 5 and b_off = 2 -- holds the gradient in its columns [2, 2 + B) and zeros in the others, and the result meets the
C++ oracle at the bounds of tests/test_angle_records_gpu.py (spectra 1e-8 / 1e-7, loss sums 1e-9, gradient columns 1e-6 of the
column's largest entry: its _against_oracle, imported).  One reference per case."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc
from test_angle_records_gpu import _against_oracle

B_OFF, B_EXTRA = 2, 5

# name -> (n_angles, B, electron feature, ion feature)
CASES = {
    "B1_nang10": (10, 1, True, True),
    "B3_nang1": (1, 3, True, True),
    "B3_nang17": (17, 3, True, True),
    "B65_nang16": (16, 65, True, True),
    "B257_nang10": (10, 257, True, True),
    "B1_nang16_ion": (16, 1, False, True),
    "B3_nang10_ele": (10, 3, True, False),
    "B65_nang1_ion": (1, 65, False, True),
    "B65_nang17_ele": (17, 65, True, False),
    "B257_nang16_ele": (16, 257, True, False),
    "B257_nang1_ion": (1, 257, False, True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    nang, B, ele, ion = CASES[name]
    cfg = decks.deck_fit()
    sa = dict(sa=np.linspace(53.6, 66.1, nang), weights=np.ones((B, nang)) / nang)
    seed = 2300 + 10 * sorted(CASES).index(name)
    batch = util.synthetic_batch(cfg, sa, B, seed=seed)
    normed = util.random_lineouts(cfg, B, seed=seed + 1)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    ext = cfg["other"]["extraoptions"]
    ext["load_ele_spec"], ext["load_ion_spec"] = ele, ion
    ext["fit_EPWb"] = ext["fit_EPWr"] = ele
    ext["fit_IAW"] = ion
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, B=B, dlm=False, X=util.normed_to_matrix(normed, 1))


@functools.lru_cache(maxsize=None)
def _reference(name, w):
    from oracle import c_oracle as co
    from tsadar_amd.params import SlotMap

    s = _case(name)
    gm = SlotMap(s["cfg"]["parameters"], True).active.astype(np.uint8)
    sums, gref, Eo, Io = co.loss_grad(s["cfg"], s["sa"], s["X"], s["batch"], w=np.array(w), gmask=gm)
    return dict(sums=sums.sum(axis=0), grad=gref, E=Eo, I=Io, gm=gm)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_grouped_sums(name):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    nang, B, ele, ion = CASES[name]
    s = _case(name)
    eng = Engine(s["cfg"], s["sa"])
    w = eng.loss_weights(B, s["i_norm"], s["e_norm"], s["cfg"]["data"]["ion_loss_scale"])
    ref = _reference(name, tuple(float(v) for v in w))
    gm = eng.slots.active.astype(np.uint8)
    assert np.array_equal(gm, ref["gm"])
    act = [int(k) for k in np.nonzero(gm)[0]]
    kernel = "k_spectrum_fused<1, 0, false, %s>" % ("true" if nang <= 16 else "false")
    runs = {}
    for rep in (0, 1):
        res = eng.loss_grad(s["X"], s["batch"], w, gm, want_spectra=True)
        torch.cuda.synchronize()
        assert any(k.startswith(kernel) for k in eng.last_launch()), eng.last_launch()
        runs["grad", rep] = [a.cpu().numpy() for a in res]
        res = eng.loss_grad_packed(s["X"], s["batch"], w, gm, act, B_global=B + B_EXTRA, b_offset=B_OFF, want_spectra=True)
        torch.cuda.synchronize()
        assert any(k.startswith(kernel) for k in eng.last_launch()), eng.last_launch()
        runs["packed", rep] = [a.cpu().numpy() for a in res]   # (copies: the packed buffer is persistent)
    # two runs of each: every array bit for bit
    for what in ("grad", "packed"):
        for a, b in zip(runs[what, 0], runs[what, 1]):
            np.testing.assert_array_equal(a, b, err_msg=what)
    t, g, E, I = runs["grad", 0]
    packed, Ep, Ip = runs["packed", 0]
    np.testing.assert_array_equal(Ep, E)
    np.testing.assert_array_equal(Ip, I)
    # the packed buffer: the loss sums, this call's columns, zeros in the columns of the other ranks
    Bg = B + B_EXTRA
    assert packed.shape == (3 + len(act) * Bg,)
    np.testing.assert_array_equal(packed[:3], t)
    cols = packed[3:].reshape(len(act), Bg)
    np.testing.assert_array_equal(cols[:, B_OFF:B_OFF + B], g[:, act].T)
    assert np.all(cols[:, :B_OFF] == 0.0) and np.all(cols[:, B_OFF + B:] == 0.0)
    assert np.abs(g).max() > 0.0
    _against_oracle(name, s, ref, w, t, g, E, I, ele, ion)
