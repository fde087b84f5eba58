"""The software-pipelined IRF convolutions (conv4_phase) at every tap-group count at which the loop takes another path.

conv4_phase walks the taps in groups of four, two groups per request and four per loop body, and finishes with a tail of 0 .. 3
groups; it requests two groups beyond the last one it uses, in the forward direction upwards and in the adjoint downwards.  The
two-sweep kernel k_spectrum (launch plan 2) computes the same sums with a loop of its own and is the bit-for-bit reference: for
every IRF setting below, the default plan (k_spectrum_fused) must give the spectra and the three loss sums of plan 2 and the
spectra of tsff_forward (k_forward_pairs) exactly, and its gradient to 1e-12 relative (test_launch_plans_agree's tolerance).

Group counts.  The taps of a feature are the Gaussian on the feature's own wavelength axis within `irf_cutoff_sigmas` standard
deviations of the axis' centre, which lies half-way between two samples: n taps (n even), first tap at offset -n / 2.  The host
(tsff_create) walks them in na_f = (pre + n + 3) / 4 groups forward and na_a = (prea + n + 3) / 4 groups in the adjoint, where
pre / prea align the first tap to a multiple of four.  With an even n and the offset -n / 2 the forward count is always even
(n = 2 .. 8 -> 2, 10 .. 16 -> 4, ...) -- except for the identity tap of spect_stddev_ion = 0 (n = 1, one group) -- while the adjoint
count takes every value (n = 2 -> 1, 4 / 6 -> 2, 8 / 10 -> 3, 12 / 14 -> 4, 16 / 18 -> 5, 32 -> 9).  The settings are chosen so that the
counts of the two directions together cover 1 (Gaussian and identity), 2, 3, 4, 5, 9 (one more than a multiple of the body of
four groups) and the widest response there is: every sample of the axis a tap, 256 / 257 groups (the LDS admits it at one point
per pixel; would the engine have to cut the taps to fit, the cut response is the widest by construction).  The counts are computed
here as the host computes them and the cover is asserted.

B = 3 lineouts (two with noise, one without), 1024 samples; one case with two ion species.
"""
import warnings

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

B = 3
BODY = 4   # tap groups per loop body of conv4_phase

# name -> (spect_stddev_ele and spect_stddev_ion in samples of the feature's axis (None: the deck's own; 0: no response), cutoff, ions)
CASES = {
    "n2_identity": (0.08, 0.0, 12.0, 1),
    "n8_n4": (1.0, 0.5, 4.0, 1),           # (cut at 4 sigma: four samples on either side, two on either side)
    "n16_n12": (0.667, 0.5, 12.0, 1),
    "n32_widest": (1.333, 400.0, 12.0, 1),
    "deck_two_ions": (None, None, 12.0, 2),
}
WANTED = {1, 2, 3, 4, 5, 9}


def group_counts(n, toff):
    """(forward, adjoint) tap groups of n taps with first offset toff, as tsff_create computes them"""
    pre = toff - 4 * (toff // 4)
    ua = -toff - n + 1
    prea = ua - 4 * (ua // 4)
    return (pre + n + 3) // 4, (prea + n + 3) // 4


def case_cfg(name):
    from tsadar_amd.engine import wavelength_axis_nm

    sd_e, sd_i, cutoff, n_ion = CASES[name]
    cfg = decks.deck_fit(n_ion=n_ion)
    o = cfg["other"]
    wid = o["PhysParams"]["widIRF"]
    for key, rng, sd in (("spect_stddev_ele", "lamrangE", sd_e), ("spect_stddev_ion", "lamrangI", sd_i)):
        if sd is not None:
            lam = wavelength_axis_nm(o[rng], 1024)
            wid[key] = sd * float(lam[1] - lam[0])
    return cfg, cutoff, n_ion


def case_counts(cfg, cutoff):
    """{feature: (n, forward groups, adjoint groups)} of a deck at a cut-off, on the host as the engine does it"""
    from tsadar_amd.engine import binned_taps, gaussian_taps, wavelength_axis_nm

    o = cfg["other"]
    out = {}
    for f, key, rng in (("ele", "spect_stddev_ele", "lamrangE"), ("ion", "spect_stddev_ion", "lamrangI")):
        sd = float(o["PhysParams"]["widIRF"][key])
        if not sd:
            out[f] = (1, *group_counts(1, 0))   # the identity tap
            continue
        t, d0 = gaussian_taps(wavelength_axis_nm(o[rng], 1024), sd, cutoff)
        t, off = binned_taps(t, d0, 1)
        out[f] = (t.size, *group_counts(t.size, off))
    return out


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def measured():
    """one 'measured' batch for every case (the deck's own IRF): two lineouts with noise, one without"""
    cfg = decks.deck_fit()
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=91)
    batch["noise_e"][2] = 0.0
    batch["noise_i"][2] = 0.0
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    return sa, batch, i_norm, e_norm


def test_settings_cover_the_group_counts():
    """(no GPU needed; the GPU cases below are only as good as this cover)"""
    seen, widest = set(), 0
    identity = False
    for name in CASES:
        cfg, cutoff, _ = case_cfg(name)
        for f, (n, na_f, na_a) in case_counts(cfg, cutoff).items():
            print(f"{name} {f}: {n} taps, {na_f} groups forward, {na_a} adjoint")
            seen |= {na_f, na_a}
            widest = max(widest, n)
            identity |= n == 1
    assert WANTED <= seen, (sorted(WANTED - seen), sorted(seen))
    assert identity
    assert any(na > BODY + 1 and na % BODY == 1 for na in seen)
    assert any(na % BODY == r for na in seen for r in (2, 3)) and any(na % BODY == 0 for na in seen)
    assert widest == 1024   # every sample of the axis a tap: there is no wider response


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_pipelined_convolutions_keep_their_bits(torch_mod, measured, name):
    from tsadar_amd.engine import Engine

    sa, batch, i_norm, e_norm = measured
    cfg, cutoff, n_ion = case_cfg(name)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng = Engine(cfg, sa, irf_cutoff_sigmas=cutoff)
    if name == "n32_widest":   # all of the axis, or what the engine had to cut it to
        n_ion_taps = case_counts(cfg, eng.irf_cutoff_sigmas)["ion"][0]
        assert n_ion_taps == 1024 or eng.irf_cutoff_sigmas < cutoff, (n_ion_taps, eng.irf_cutoff_sigmas, [str(w.message) for w in caught])
    else:
        assert eng.irf_cutoff_sigmas == cutoff
    normed = util.random_lineouts(cfg, B, seed=141)
    X = util.normed_to_matrix(normed, n_ion)
    w = eng.loss_weights(B, i_norm, e_norm, cfg["data"]["ion_loss_scale"])
    gm = eng.slots.active.astype(np.uint8)
    out = {}
    for plan in (0, 2):   # bit 1: the two-sweep kernel (its own convolution loops) instead of the one-sweep one
        eng.set_launch_plan(plan)
        t, g, E, I = eng.loss_grad(X, batch, w, gm, want_spectra=True)
        out[plan] = [a.cpu().numpy().copy() for a in (t, g, E, I)]
    eng.set_launch_plan(0)
    Ef, If = eng.forward(X, batch["e_amps"], batch["i_amps"], batch["noise_e"], batch["noise_i"])
    t0, g0, E0, I0 = out[0]
    t2, g2, E2, I2 = out[2]
    assert np.all(np.isfinite(E0)) and np.all(np.isfinite(I0)) and np.all(np.isfinite(g0))
    assert np.array_equal(E0, E2) and np.array_equal(I0, I2), name
    assert np.array_equal(t0, t2), (name, t0, t2)
    np.testing.assert_allclose(g0, g2, rtol=1e-12, atol=1e-15 * np.abs(g2).max())
    assert np.array_equal(E0, Ef.cpu().numpy()) and np.array_equal(I0, If.cpu().numpy()), name
