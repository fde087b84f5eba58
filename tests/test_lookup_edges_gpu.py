"""The edges of the sweep's lookups on the GPU: xi_e left of, right of and just inside the velocity grid, the pair boundary of
the pair-sweep kernels and the one sample without a right neighbour.

The single-species pair-sweep kernels (k_spectrum_fused, k_forward_pairs) send every position outside the vx grid to the
out-of-grid cell of the Hermite coefficient table (cell nvx - 1: ln f_e = -50, slope 0; hermite_lookup_c<true>, hermite_pad_cell)
instead of selecting on a comparison, and know at compile time that every sample but the second one of a thread's last pair has a
right neighbour (pair_has_next).  The two-sweep kernel keeps the selects: the same decks run through both, and through tsff_forward.
A few lineouts per case, 10 angles, chosen with the oracle alone so that the EPW sweep meets every class of position:

  below    xi_e <  vx[0]                         (out-of-grid cell through floor = -1)
  above    xi_e >  vx[-1]                        (out-of-grid cell through the upper clamp)
  inside   vx[0] <= xi_e <= vx[-1]
  edge     xi_e inside the first or the last interval of the grid

and each class holds at least 1 % of the case's (lambda, theta) points.  The two edge intervals count as ONE class: an interval
is 1 / (nvx - 1) of the grid, 0.79 % at nvx = 128, and a lineout whose 1024 evenly spaced samples reach an end of the grid
spends at most about that share of them in the interval there (measured with the oracle: 0.5 - 0.8 % each, whatever the window
and the temperature); both intervals are asserted non-empty on their own.  T_e in [0.6, 1.0] keV pushes both EPW wings out of
the grid (a drift u_d moves them against each other); the IAW sweep lies inside the grid throughout.

Grids: nvx = 128 (the benchmark's) and nvx = 33, where nvx - 1 is a power of two (the spacing of the doubles changes right at
the upper clamp).  The third case makes the DLM order a leaf (GM = 1): the tangent table's all-zero out-of-grid cell is read.

Reference: the C++ oracle (forward-mode dual numbers), with the tolerances tests/test_gpu_parity.py uses for it -- spectra 1e-8
(EPW) / 1e-7 (IAW), loss sums 1e-9, gradient columns 1e-6 of the column's largest entry.  The C++ oracle does not differentiate
the DLM order: that case takes the autodiff twin, as test_gpu_parity does for such decks (spectra 1e-8 / 1e-7, loss 1e-9,
gradient 1e-7 of the largest entry).  One reference per case, shared by its tests."""
import functools

import numpy as np
import pytest

import decks
import util
from oracle import tsadar_oracle as orc

CASES = {
    "nvx128": dict(nvx=128, B=5, seed=901, active=("Te", "ne", "Ti", "Va", "ud", "lam", "amp1", "amp2")),
    "nvx33": dict(nvx=33, B=4, seed=911, active=("Te", "ne", "Ti", "Va", "ud", "lam", "amp1", "amp2")),
    "nvx128_dlm": dict(nvx=128, B=3, seed=921, active=("Te", "ne", "m", "amp1", "amp2", "lam")),
}
EDGE_SAMPLES = (511, 512, 1023)   # the pair boundary of the pair-sweep kernels and the only sample without a right neighbour


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]
    dlm = "m" in c["active"]
    cfg = decks.deck_fit(nvx=c["nvx"], active=c["active"], m=2.7 if dlm else 2.0)
    B = c["B"]
    sa = util.sa_fit(B)
    batch = util.synthetic_batch(cfg, sa, B, seed=c["seed"])
    ranges = dict(Te=(0.6, 1.0), ud=(-8.0, 8.0))
    if dlm:
        ranges["m"] = (2.05, 4.4)
    normed = util.random_lineouts(cfg, B, seed=c["seed"] + 1, ranges=ranges)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, i_norm=i_norm, e_norm=e_norm, B=B, dlm=dlm, X=util.normed_to_matrix(normed, 1))


def _xi_e(cfg, sa, p):
    """xi_e [npts, n_angles] of one lineout's EPW sweep: form_factor.py:215-253 as the oracle's form_factor() writes them (G = 1)."""
    lam_axis = np.linspace(cfg["other"]["lamrangE"][0], cfg["other"]["lamrangE"][1], cfg["other"]["npts"])
    omgs = (2e7 * np.pi * orc.C / lam_axis)[:, None]
    omgL = 2 * np.pi * 1e7 * orc.C / (p["lam"] + cfg["data"].get("ele_lam_shift", 0.0))
    omgpe = orc.C0 * np.sqrt(1.0e20 * p["ne"])
    ks = np.sqrt(omgs**2 - omgpe**2) / orc.C
    kL = np.sqrt(omgL**2 - omgpe**2) / orc.C
    k = np.sqrt(ks**2 + kL**2 - 2 * ks * kL * np.cos(np.asarray(sa["sa"]) * np.pi / 180)[None, :])
    vTe = np.sqrt(p["Te"] / orc.ME)
    return ((omgs - omgL) - k * p["Va"] * 1e6) / (k * vTe) - p["ud"] * 1e6 / vTe


def _classes(name):
    s = _case(name)
    vx = orc.velocity_grid(CASES[name]["nvx"])
    phys = orc.physical_params(s["cfg"]["parameters"], s["normed"], True)
    x = np.stack([_xi_e(s["cfg"], s["sa"], orc.lineout_params(phys, b, 1)) for b in range(s["B"])])
    assert x.shape == (s["B"], 1024, 10)
    first, last = (x >= vx[0]) & (x < vx[1]), (x > vx[-2]) & (x <= vx[-1])
    frac = dict(below=np.mean(x < vx[0]), above=np.mean(x > vx[-1]), inside=np.mean((x >= vx[0]) & (x <= vx[-1])),
                edge=np.mean(first | last))
    return frac, int(first.sum()), int(last.sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_lineouts_cover_every_class_of_position(name):
    """Oracle alone (no GPU): every class of xi_e holds at least 1 % of the case's points, both edge intervals are met."""
    frac, n_first, n_last = _classes(name)
    print(name, {k: round(float(v), 4) for k, v in frac.items()}, "first", n_first, "last", n_last)
    for k, v in frac.items():
        assert v >= 0.01, (name, k, v)
    assert n_first > 0 and n_last > 0, (name, n_first, n_last)


@functools.lru_cache(maxsize=None)
def _reference(name, w):
    """Loss (sums or value), gradient and spectra of the case with the loss weights w (a tuple), computed once."""
    s = _case(name)
    from tsadar_amd.params import SlotMap

    gm = SlotMap(s["cfg"]["parameters"], True).active.astype(np.uint8)
    if s["dlm"]:
        from oracle import tsadar_oracle_torch as ot

        names = ["Te", "ne", "m", "amp1", "amp2", "lam"]
        val, ref, Eo, Io = ot.value_and_grad(s["cfg"], s["sa"], s["normed"], s["batch"], s["i_norm"], s["e_norm"], names)
        return dict(val=val, named=ref, names=names, E=np.asarray(Eo), I=np.asarray(Io), gm=gm)
    from oracle import c_oracle as co

    sums, gref, Eo, Io = co.loss_grad(s["cfg"], s["sa"], s["X"], s["batch"], w=np.array(w), gmask=gm)
    return dict(sums=sums.sum(axis=0), grad=gref, E=Eo, I=Io, gm=gm)


def _elementwise(a, b, floor=1e-12):
    """util.rel_err's measure, per element: |a - b| / max(|b|, floor * max|b| of the row)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b) / np.maximum(np.abs(b), floor * np.max(np.abs(b), axis=-1, keepdims=True))


def _check_spectra(tag, E, I, ref):
    eE, eI = _elementwise(E, ref["E"]), _elementwise(I, ref["I"])
    print(tag, "spectra: EPW %.3e IAW %.3e" % (eE.max(), eI.max()),
          "samples", {j: (float(eE[:, j].max()), float(eI[:, j].max())) for j in EDGE_SAMPLES})
    assert eE.max() < 1e-8 and eI.max() < 1e-7, (tag, eE.max(), eI.max())
    for j in EDGE_SAMPLES:   # separately: the pair boundary and the sample without a right neighbour, both features
        assert np.all(ref["E"][:, j] != 0.0) and np.all(ref["I"][:, j] != 0.0)
        assert eE[:, j].max() < 1e-8, (tag, "EPW", j, eE[:, j])
        assert eI[:, j].max() < 1e-7, (tag, "IAW", j, eI[:, j])


def _check_loss_grad(tag, s, ref, w, terms, grad):
    gm = ref["gm"]
    if s["dlm"]:
        val = float(np.dot(terms, w))
        print(tag, "loss", val, ref["val"])
        assert abs(val - ref["val"]) < 1e-9 * abs(ref["val"]), (tag, val, ref["val"])
        G = util.matrix_to_named(grad, ref["names"])
        scale = max(np.max(np.abs(v)) for v in ref["named"].values())
        for k in ref["names"]:
            err = np.max(np.abs(G[k] - ref["named"][k])) / scale
            print(tag, "grad", k, "%.3e" % err)
            assert err <= 1e-7, (tag, k, G[k], ref["named"][k])
    else:
        print(tag, "loss sums", terms, ref["sums"])
        np.testing.assert_allclose(terms, ref["sums"], rtol=1e-9)
        for sl in np.nonzero(gm)[0]:
            err = np.max(np.abs(grad[:, sl] - ref["grad"][:, sl])) / np.max(np.abs(ref["grad"][:, sl]))
            print(tag, "grad column", sl, "%.3e" % err)
            assert err < 1e-6, (tag, sl, grad[:, sl], ref["grad"][:, sl])
    assert np.all(grad[:, gm == 0] == 0.0)
    assert np.all(grad[:, gm != 0] != 0.0)   # every trainable leaf of every lineout is reached


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_lookup_edges_against_oracle(name):
    """tsff_loss_grad by the one-sweep kernel (plan 0) and by the two-sweep kernel (plan bit 1) and tsff_forward against the oracle:
    spectra, loss terms, gradient; samples 511, 512 and 1023 of both features on their own."""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from tsadar_amd.engine import Engine

    frac, n_first, n_last = _classes(name)
    assert min(frac.values()) >= 0.01 and n_first > 0 and n_last > 0, (frac, n_first, n_last)
    s = _case(name)
    eng = Engine(s["cfg"], s["sa"])
    w = eng.loss_weights(s["B"], s["i_norm"], s["e_norm"], s["cfg"]["data"]["ion_loss_scale"])
    ref = _reference(name, tuple(float(v) for v in w))
    gm = eng.slots.active.astype(np.uint8)
    assert np.array_equal(gm, ref["gm"])
    kernel = {0: "k_spectrum_fused<1, %d, " % int(s["dlm"]), 2: "k_spectrum<1, 1, %d, " % int(s["dlm"])}   # (k_spectrum<NI, MODE, GM, ...>)
    for plan in (0, 2):
        eng.set_launch_plan(plan)
        terms, grad, E, I = eng.loss_grad(s["X"], s["batch"], w, gm, want_spectra=True)
        torch.cuda.synchronize()
        launched = eng.last_launch()
        print(name, "plan", plan, launched)
        assert any(k.startswith(kernel[plan]) for k in launched), (plan, launched)
        tag = "%s plan %d" % (name, plan)
        _check_spectra(tag, E.cpu().numpy(), I.cpu().numpy(), ref)
        _check_loss_grad(tag, s, ref, w, terms.cpu().numpy(), grad.cpu().numpy())
    eng.set_launch_plan(0)
    b = s["batch"]
    Ef, If = eng.forward(s["X"], b["e_amps"], b["i_amps"], b["noise_e"], b["noise_i"])
    torch.cuda.synchronize()
    launched = eng.last_launch()
    print(name, "forward", launched)
    assert any(k.startswith("k_forward_pairs<") for k in launched), launched
    _check_spectra(name + " forward", Ef.cpu().numpy(), If.cpu().numpy(), ref)
