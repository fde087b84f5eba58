"""The oracle against every fixture the reference's own tests hold for this path:
the golden vector of tests/test_forward/test_1d.py and the two dispersion-relation known-answer
tests.  CPU only."""
import os

import numpy as np
from scipy.signal import find_peaks

import decks
import util
from oracle import tsadar_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_golden_vector():
    """tests/test_forward/test_1d.py:17-84: assert_allclose(ThryE, ThryE-1d.npy, rtol=1e-4), atol 0.
    The restatement reproduces it to < 1e-9 (measured 6e-13)."""
    cfg = decks.deck_1d()
    batch = dict(i_data=np.array([1]), e_data=np.array([1]), noise_e=np.array([0]), noise_i=np.array([0]),
                 e_amps=np.array([1]), i_amps=np.array([1]))
    normed = orc.init_normed_params(cfg["parameters"], 1, activate=True)
    E, I, lE, lI = orc.ts_diag(cfg, util.P9, normed, batch)
    golden = np.load(os.path.join(GOLDEN, "ref_ThryE-1d.npy"))
    np.testing.assert_allclose(E, golden, rtol=1e-4, atol=0)  # the reference's own criterion
    assert np.max(np.abs(E - golden) / np.abs(golden)) < 1e-9
    assert E.max() == golden.max() == 1.0104138361652801  # amp 1 -> 1.010414 through the "logit"


def test_activation_round_trip_quirk():
    """SURVEY.md Q6 (ts_params.py:344): Te .5 -> .50175, lam 524 -> 524.022, amp 1 -> 1.010414, m 2.5 -> 2.5158."""
    cfg = decks.deck_1d()
    p = orc.physical_params(cfg["parameters"], orc.init_normed_params(cfg["parameters"], 1, True), True)
    assert abs(p["Te"][0] - 0.50175174) < 1e-8
    assert abs(p["lam"][0] - 524.02200177) < 1e-8
    assert abs(p["amp1"][0] - 1.01041384) < 1e-8
    assert abs(p["m"][0] - 2.51579223) < 1e-8


def _kat_params(cfg):
    P = cfg["parameters"]
    return dict(Te=P["electron"]["Te"]["val"], ne=P["electron"]["ne"]["val"], lam=P["general"]["lam"]["val"],
                Va=0.0, ud=0.0, ne_gradient=0.0, Te_gradient=0.0,
                Ti=[P["ion-1"]["Ti"]["val"]], Z=[P["ion-1"]["Z"]["val"]], A=[P["ion-1"]["A"]["val"]], fract=[1.0])


def test_epw_bohm_gross_kat():
    """tests/test_form_factor/test_epw.py:33-74: EPW peaks vs omega^2 = wpe^2 + 3 k^2 vTe^2, rtol 1e-2."""
    cfg = decks.deck_kat("epw")
    p = _kat_params(cfg)
    vx, fe = orc.velocity_grid(128), orc.dlm_fe(2.0, 128)
    P, lam_cm = orc.form_factor([400, 700], 8192, 0.0, np.array([60.0]), 1, p, vx, fe)
    spec = np.squeeze(P)
    peaks, props = find_peaks(spec, height=(0.01, 0.5), prominence=0.02)
    hi = peaks[np.argmax(props["peak_heights"])]
    lo = peaks[np.argsort(props["peak_heights"])[0]]
    lams = lam_cm[[hi, lo]]
    model = 2 * np.pi * orc.C / lams
    omgpe = orc.C0 * np.sqrt(0.2 * 1e20)
    omgL = 2 * np.pi * 1e7 * orc.C / p["lam"]
    ks = np.sqrt(model**2 - omgpe**2) / orc.C
    kL = np.sqrt(omgL**2 - omgpe**2) / orc.C
    k = np.sqrt(ks**2 + kL**2 - 2 * ks * kL * np.cos(60 * np.pi / 180))
    omg = np.sqrt(omgpe**2 + 3 * k**2 * (0.5 / orc.ME))
    np.testing.assert_allclose(model, [omgL + omg[0], omgL - omg[1]], rtol=1e-2)


def test_iaw_dispersion_kat():
    """tests/test_form_factor/test_iaw.py:40-71: IAW peaks vs omega = 2 kL sqrt((Z Te + 3 Ti)/Mi), rtol 1e-2."""
    cfg = decks.deck_kat("iaw")
    p = _kat_params(cfg)
    vx, fe = orc.velocity_grid(128), orc.dlm_fe(2.0, 128)
    P, lam_cm = orc.form_factor([525, 528], 8192, 0.0, np.array([60.0]), 1, p, vx, fe)
    spec = np.squeeze(np.mean(P, axis=0))
    peaks, props = find_peaks(spec, height=0.1, prominence=0.2)
    hi = peaks[np.argmax(props["peak_heights"])]
    second = peaks[np.argpartition(props["peak_heights"], -2)[-2]]
    lams = lam_cm[[hi, second]]
    omgpe = orc.C0 * np.sqrt(0.2 * 1e20)
    omgL = 2 * np.pi * 1e7 * orc.C / p["lam"]
    kL = np.sqrt(omgL**2 - omgpe**2) / orc.C
    model = 2 * np.pi * orc.C / lams
    omg = 2 * kL * np.sqrt((0.5 + 3 * 0.2) / orc.MP)
    np.testing.assert_allclose(sorted([omgL + omg, omgL - omg]), sorted(model), rtol=1e-2)
    # sharper than the reference's criterion (which is dominated by omgL): the peak SEPARATION is twice the
    # ion-acoustic frequency k*cs with k = 2 kL sin(theta/2) = kL at 60 degrees and the deck's Te = 0.6, Ti = 0.2
    cs = np.sqrt((p["Z"][0] * p["Te"] + 3 * p["Ti"][0]) / (p["A"][0] * orc.MP))
    assert abs(abs(model[0] - model[1]) / (2 * kL * cs) - 1) < 0.1


def test_zprime_table_is_not_analytic():
    """the shipped Re Z' table deviates from -2(1 + xi Z(xi)) by up to ~1.6e-3 -> use the table."""
    from scipy.special import wofz

    _, xi2 = orc.xi_grids()
    zr, zi = orc.zprime_tables()
    Z = 1j * np.sqrt(np.pi) * wofz(xi2)
    ana = -2 * (1 + xi2 * Z)
    assert 1e-4 < np.max(np.abs(zr - ana.real)) < 5e-3
    assert np.max(np.abs(zi - ana.imag)) < 1e-4
    assert xi2.size == 1640 and orc.xi_grids()[0].size == 1024


def test_ratintn_drops_last_interval_and_matches_quadrature():
    """SURVEY.md Q3 + a sanity check of W against the principal-value integral for a Maxwellian:
    W(x) = PV int f'(v)/(v - x) dv = -sqrt? -> compare with the analytic Re Z' relation within 1e-3."""
    vx, fe = orc.velocity_grid(128), orc.dlm_fe(2.0, 128)
    W, ratmod = orc.chi_table(vx, fe)
    xi1, xi2 = orc.xi_grids()
    assert W.shape == (1640,) and ratmod.shape == (1024,)
    # for f = exp(-v^2/2)/sqrt(2 pi):  PV int f'/(v-x) dv = -(1 + (x/sqrt2) Re Z(x/sqrt2)) = Re Z'(x/sqrt 2)/2
    from scipy.special import wofz

    x = xi2[np.abs(xi2) < 4]
    Zp = -2 * (1 + (x / np.sqrt(2)) * (1j * np.sqrt(np.pi) * wofz(x / np.sqrt(2))))
    assert np.max(np.abs(W[np.abs(xi2) < 4] - 0.5 * Zp.real)) < 2e-3
