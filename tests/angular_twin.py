"""The torch twin as the yardstick of the forward-mode calls of the angular path (tests/test_form_factor_jvp.py,
tests/test_angular_postfit.py): ``ot.form_factor`` with ``ot.chi_table`` and ``ot.ats_spectrum`` as they stand, one
``torch.autograd.functional.jvp`` per direction."""
import numpy as np

import util
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L

ROW_TOL = 1e-7   # every row within ROW_TOL of its own largest entry in the twin: the bound tests/test_jacobian.py holds the chain to


def row_ratios(Jd, Jt):
    """max |Jd - Jt| / max |Jt| per row (the last axis); a row that is identically zero in the twin must be exactly zero."""
    Jd, Jt = np.asarray(Jd), np.asarray(Jt)
    scale = np.max(np.abs(Jt), axis=-1)
    err = np.max(np.abs(Jd - Jt), axis=-1)
    zero = scale == 0.0
    assert not np.any(Jd[zero]), "a row that is zero in the twin is not exactly zero on the device"
    return np.where(zero, 0.0, err / np.where(zero, 1.0, scale))


def twin_p(px, n_ion, ti_same, A):
    """The twin's parameter dict of one lineout from the physical parameters px [NP] (a tensor), a tied Ti taken from ion 1."""
    p = {k: px[util.slot_of(k)] for k in ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]}
    o = lambda s, k: L.P_ION0 + 4 * s + k
    p["Ti"] = [px[o(0 if (s > 0 and ti_same[s]) else s, L.ION_TI)] for s in range(n_ion)]
    p["Z"] = [px[o(s, L.ION_Z)] for s in range(n_ion)]
    p["fract"] = [px[o(s, L.ION_FRACT)] for s in range(n_ion)]
    p["A"] = [float(a) for a in A]
    return p


def form_factor_fn(cfg, sa_deg, n_ion, ti_same, A, feature=0):
    """-> f(px [NP], fe [nvx]) = P [G, npts, n_angles] of the twin, differentiable in both (W from ot.chi_table of the same fe)."""
    from oracle import tsadar_oracle_torch as ot

    other = cfg["other"]
    G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
    vx = ot._t(orc.velocity_grid(cfg["parameters"]["electron"]["fe"]["nvx"]))
    rng, shift = (other["lamrangE"], cfg["data"]["ele_lam_shift"]) if feature == 0 else (other["lamrangI"], 0.0)

    def f(px, fe):
        P, _ = ot.form_factor(rng, other["npts"], shift, sa_deg, G, twin_p(px, n_ion, ti_same, A), vx, fe, ot.chi_table(vx, fe))
        return P

    return f


def form_factor_jvp(cfg, sa_deg, n_ion, ti_same, x, fe, phys_dot, fe_dot, feature=0):
    """The twin's (P, P_dot [n_dir]) of one lineout: x [NP] physical, fe [nvx], phys_dot [n_dir, NP], fe_dot [n_dir, nvx] or None."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    A = [x[L.P_ION0 + 4 * s + L.ION_A] for s in range(n_ion)]
    f = form_factor_fn(cfg, sa_deg, n_ion, ti_same, A, feature)
    x0, f0 = ot._t(x), ot._t(fe)
    P, out = None, []
    for k in range(phys_dot.shape[0]):
        vf = ot._t(fe_dot[k]) if fe_dot is not None else torch.zeros_like(f0)
        P, Pd = torch.autograd.functional.jvp(f, (x0, f0), (ot._t(phys_dot[k]), vf))
        out.append(Pd.detach().numpy())
    return P.detach().numpy(), np.array(out)


def ats_fn(cfg, sa, n_lam, e_amps, lam):
    """-> g(P [G, npts, n_angles], amp [2]) = the twin's ARTS image [rows, n_lam], differentiable in both."""
    from oracle import tsadar_oracle_torch as ot

    lam_nm = np.linspace(*cfg["other"]["lamrangE"], cfg["other"]["npts"])

    def g(P, amp):
        y, _ = ot.ats_spectrum(cfg, sa["weights"], sa["angAxis"], P, lam_nm, n_lam, e_amps, dict(lam=float(lam), amp1=amp[0], amp2=amp[1]))
        return y

    return g
