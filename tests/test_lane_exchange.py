"""The base-point exchange between neighbouring lanes (EX), with and without it, bit for bit.

A pair of samples takes its third base point -- the right neighbour of its second sample -- from the next lane's registers
(next_lane_f64, tsff_device.h: the whole-wavefront DPP shift); lane 63 takes the point right of its 128-sample unit, evaluated
once per (unit, angle) before the sweep.  Launch plan bit 8 switches the exchange off: every lane evaluates that point itself.
The exchanged doubles are the ones the lane would have computed, so spectra, loss terms and gradient of plan 0 and plan 8 are
equal under np.array_equal.  A shift in the wrong direction hands every lane its LEFT neighbour's point, a wrong lane 63 spoils
two samples per unit (the last of a unit and, through the finite difference along lambda, nothing else): either shows here at
once.

Cases: 1, 10 and 16 scattering angles (the exchange needs n_angles <= 16; the boundary points of a unit are evaluated by
lane = 16 P + a), one and two ion species, with and without the DLM order as a leaf (GM = 1: the tangent lookups read the
exchanged xi_e), one and two points per pixel (k_spectrum_fused / k_spectrum_rows, which still exchanges through LDS: the same
contract) and the forward-only kernel (k_forward_pairs) in its two workgroup sizes.  The lineouts' probe wavelengths put the
laser line into different 128-sample units of the ion feature (1.5 nm over 1024 samples: 0.1875 nm per unit), so that both the
asymptotic and the general sweep run with the exchange in first, inner and last units, lane 63 of the last unit included (its
right neighbour is the clamped last sample).
"""
import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

pytestmark = pytest.mark.gpu

# probe wavelengths (nm) of the lineouts: units 0, 1, 4, 6 and 7 of the ion feature's axis 525.75 .. 527.25 nm
LAMS = (525.80, 526.00, 526.52, 527.00, 527.20)


def _setup(nang, n_ion, dlm, ppp):
    active = ("Te", "ne", "Ti", "Va", "lam", "amp1") + (("m",) if dlm else ())
    cfg = decks.deck_fit(points_per_pixel=ppp, active=active, n_ion=n_ion, m=2.6 if dlm else 2.0)
    B = len(LAMS)
    wts = np.linspace(1.0, 2.0, nang)
    sa = dict(sa=np.linspace(53.6, 66.1, nang) if nang > 1 else np.array([60.0]), weights=(wts / wts.sum()) * np.ones([B, nang]))
    batch = util.synthetic_batch(cfg, sa, B, seed=900 + nang)
    normed = util.random_lineouts(cfg, B, seed=950 + nang)
    for i, lam in enumerate(LAMS):   # (through the inverse of the activation: the physical value is the one asked for)
        normed["lam"][i] = util.random_lineouts(cfg, B, seed=1, ranges=dict(lam=(lam, lam)))["lam"][i]
    if dlm:
        normed["m"] = util.random_lineouts(cfg, B, seed=970 + nang, ranges=dict(m=(2.1, 4.3)))["m"]
    rng = np.random.default_rng(980 + nang)
    batch["noise_e"] = 0.02 * rng.random((B, 1024))
    batch["noise_i"] = 0.02 * rng.random((B, 1024))
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    return cfg, sa, batch, normed, i_norm, e_norm


@pytest.mark.parametrize("ppp", [1, 2])
@pytest.mark.parametrize("dlm", [False, True], ids=["plasma", "dlm"])
@pytest.mark.parametrize("n_ion", [1, 2])
@pytest.mark.parametrize("nang", [1, 10, 16])
def test_exchange_changes_no_bit(nang, n_ion, dlm, ppp):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    cfg, sa, batch, normed, i_norm, e_norm = _setup(nang, n_ion, dlm, ppp)
    B = len(LAMS)
    eng = Engine(cfg, sa)
    w = eng.loss_weights(B, i_norm, e_norm, cfg["data"]["ion_loss_scale"])
    X = util.normed_to_matrix(normed, n_ion)
    gm = eng.slots.active.astype(np.uint8)
    sweep = "k_spectrum_fused<" if ppp == 1 else "k_spectrum_rows<"
    out, fwd, names = {}, {}, {}
    # 0: exchange; 8: none; 1 / 9: the same for the large-batch forms (256-thread forward workgroups, one rows workgroup for all rounds)
    for plan in (0, 8, 1, 9):
        eng.set_launch_plan(plan)
        out[plan] = [a.cpu().numpy() for a in eng.loss_grad(X, batch, w, gm, want_spectra=True)]
        names[plan] = [k for k in eng.last_launch() if k.startswith(sweep)] if plan in (0, 8) else None
        Ef, If = eng.forward(X, batch["e_amps"], batch["i_amps"], noise_e=batch["noise_e"], noise_i=batch["noise_i"], fe=None)
        fwd[plan] = (Ef.cpu().numpy(), If.cpu().numpy(), list(eng.last_launch()))
    eng.set_launch_plan(0)
    # the two plans did run the two forms: the sweep kernel's EX argument (the fourth) is true under plan 0 and false under plan 8
    assert names[0] and all(k.split(",")[3].strip(" >") == "true" for k in names[0]), names[0]
    assert names[8] and all(k.split(",")[3].strip(" >") == "false" for k in names[8]), names[8]
    terms, grad, E, I = out[0]
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0.0 and np.isfinite(E).all() and np.isfinite(I).all()
    for a, b in ((0, 8), (1, 9)):
        for k, what in enumerate(("loss terms", "gradient", "ThryE", "ThryI")):
            np.testing.assert_array_equal(out[a][k], out[b][k], err_msg=f"{what}, plan {a} against {b}")
        for k, what in enumerate(("ThryE", "ThryI")):
            np.testing.assert_array_equal(fwd[a][k], fwd[b][k], err_msg=f"forward {what}, plan {a} against {b}: {fwd[a][2]} / {fwd[b][2]}")
    # and the forward-only kernels give the bits of the loss kernels' spectra
    np.testing.assert_array_equal(fwd[0][0], E)
    np.testing.assert_array_equal(fwd[0][1], I)
