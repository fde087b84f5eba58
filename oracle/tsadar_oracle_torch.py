"""Gradient oracle: the same restatement as ``tsadar_oracle.py`` written with torch float64 CPU
tensors so that ``torch.autograd`` plays the role JAX autodiff plays in the reference
(``eqx.filter_value_and_grad(__loss__)``, tsadar/inverse/loss_function.py:108).

TEST INFRASTRUCTURE ONLY (see the header of tsadar_oracle.py).  The forward values of this twin are
checked against the NumPy oracle (tests/test_oracle_torch.py), which is itself pinned to the
reference's golden vector; its gradients are checked against finite differences of the NumPy
oracle.  Sub-gradient conventions are those of JAX: ``max`` -> one-hot at the arg-max (torch.amax
splits ties evenly; ties have measure zero), linear interpolation -> slope of the active segment,
``where`` masks -> pass-through.

The second half restates the oracle's 2-D form factor (rotate_df, calc_chi_vals_2d, form_factor_2d) and its ARTS instrument chain
(ats_spectrum); ``ff2d_adjoint`` / ``ats_adjoint`` are the references of tests/test_ff2d_adjoint_twin.py, ``loss_adjoint`` of
tests/test_loss_grad_entries.py and ``ff1d_adjoint`` of tests/test_form_factor_adjoint_twin.py.
"""
from __future__ import annotations

import numpy as np
import torch

from . import tsadar_oracle as orc

DT = torch.float64


def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=DT)


def interp_linear(x, xp, fp, left=None, right=None):
    """jnp.interp (see tsadar_oracle.interp_linear)."""
    xp, fp = _t(xp), _t(fp)
    i = torch.clamp(torch.searchsorted(xp, x.detach().contiguous(), right=True), 1, xp.numel() - 1)
    dx = xp[i] - xp[i - 1]
    df = fp[i] - fp[i - 1]
    f = fp[i - 1] + ((x - xp[i - 1]) / dx) * df
    lo = fp[0] if left is None else left
    hi = fp[-1] if right is None else right
    f = torch.where(x < xp[0], lo, f)
    f = torch.where(x > xp[-1], hi, f)
    return f


def hermite_slopes(x, f):
    d = (f[1:] - f[:-1]) / (x[1:] - x[:-1])
    return torch.cat([d[:1], 0.5 * (d[:-1] + d[1:]), d[-1:]])


def interp_hermite(xq, x, f, lo, hi):
    x = _t(x)
    fx = hermite_slopes(x, f)
    i = torch.clamp(torch.searchsorted(x, xq.detach().contiguous(), right=True), 1, x.numel() - 1)
    dx = x[i] - x[i - 1]
    t = (xq - x[i - 1]) / dx
    f0, f1 = f[i - 1], f[i]
    m0, m1 = fx[i - 1] * dx, fx[i] * dx
    c2 = -3 * f0 + 3 * f1 - 2 * m0 - m1
    c3 = 2 * f0 - 2 * f1 + m0 + m1
    fq = f0 + t * (m0 + t * (c2 + t * c3))
    fq = torch.where(xq < x[0], torch.full_like(fq, lo), fq)
    fq = torch.where(xq > x[-1], torch.full_like(fq, hi), fq)
    return fq


def gradient_uniform(f, h):
    return torch.cat([((f[1] - f[0]) / h)[None], (f[2:] - f[:-2]) / (2 * h), ((f[-1] - f[-2]) / h)[None]])


def ratcen(f, g):
    """ratintn.py:26-52 (see tsadar_oracle.ratcen).  ``f``: [N], ``g``: [..., N]; the branch is chosen from detached values, and
    the branch not taken is evaluated at a harmless argument so that it cannot leak a NaN into the gradient."""
    fdif = f[1:-1] - f[0:-2]
    gdif = g[..., 1:-1] - g[..., 0:-2]
    fav = 0.5 * (f[1:-1] + f[0:-2])
    gav = 0.5 * (g[..., 1:-1] + g[..., 0:-2])
    small = (torch.abs(gdif) < 1.0e-4 * torch.abs(gav)).detach()
    tmp = fav * gdif - gav * fdif
    gav_s = torch.where(small, gav, torch.ones_like(gav))
    rf = fav / gav_s + tmp * gdif / (12.0 * gav_s**3)
    rfn = fdif / gdif + tmp * torch.log(torch.abs((gav + 0.5 * gdif) / (gav - 0.5 * gdif))) / gdif**2
    return torch.where(small, rf, rfn)


def ratintn(f, g, z):
    """ratintn.py:4-23 (see tsadar_oracle.ratintn): sum(ratcen(f, g) * (z[1:-1] - z[0:-2]))."""
    zdif = z[1:-1] - z[0:-2]
    return torch.sum(ratcen(f, g) * zdif, dim=-1)


def chi_table(vx, fe):
    """form_factor.py:263-268 (see tsadar_oracle.chi_table; differentiable in fe)."""
    xi1, xi2 = (_t(a) for a in orc.xi_grids())
    ratmod = torch.exp(interp_hermite(xi1, vx, torch.log(fe), -50.0, -50.0))
    ratdf = gradient_uniform(ratmod, xi1[1] - xi1[0])
    return ratintn(ratdf, xi1[None, :] - xi2[:, None], xi1)


def dlm_fe(m, nvx):
    """DLM1V.__call__ (base.py:277-294), differentiable in m."""
    vx = orc.velocity_grid(nvx)
    tab = _t(orc.dlm_table(nvx))
    max_ = _t(orc.DLM_M_AXIS)
    k = int(np.clip(np.searchsorted(orc.DLM_M_AXIS, float(m.detach()), side="right"), 1, 30))
    t = (m - max_[k - 1]) / (max_[k] - max_[k - 1])
    f = tab[:, k - 1] + t * (tab[:, k] - tab[:, k - 1])
    if float(m.detach()) < 2.0:
        f = tab[:, 0] + 0.0 * m
    if float(m.detach()) > 5.0:
        f = tab[:, -1] + 0.0 * m
    return f / torch.sum(f) / (vx[1] - vx[0])


def physical_params(cfg_params, normed, activate=True):
    """ts_params.py:583-603 for tensors ``normed[name]`` of shape [B]."""
    def act(active, x):
        return torch.sigmoid(x) if (activate and active) else x

    el = cfg_params["electron"]
    phys = {}
    for k in ["Te", "ne"]:
        phys[k] = act(el[k]["active"], normed[k]) * (el[k]["ub"] - el[k]["lb"]) + el[k]["lb"]
    if "m" in normed:
        phys["m"] = act(el["fe"].get("active", False), normed["m"]) * 3.0 + 2.0
    species = orc.ion_species(cfg_params)
    fsum = 0.0
    for s, sp in enumerate(species):
        ic = cfg_params[sp]
        for k in ["Ti", "Z"]:
            phys[f"{k}_{s+1}"] = act(ic[k]["active"], normed[f"{k}_{s+1}"]) * (ic[k]["ub"] - ic[k]["lb"]) + ic[k]["lb"]
        phys[f"A_{s+1}"] = normed[f"A_{s+1}"]
        phys[f"fract_{s+1}"] = act(ic["fract"]["active"], normed[f"fract_{s+1}"])
        if s > 0 and ic["Ti"].get("same", False):
            phys[f"Ti_{s+1}"] = phys["Ti_1"]
        fsum = fsum + phys[f"fract_{s+1}"]
    for s in range(len(species)):
        phys[f"fract_{s+1}"] = phys[f"fract_{s+1}"] / fsum
    g = cfg_params["general"]
    for k in orc.GENERAL_KEYS:
        phys[k] = act(g[k]["active"], normed[k]) * (g[k]["ub"] - g[k]["lb"]) + g[k]["lb"]
    return phys


def form_factor(lam_range, npts, lam_shift, sa_deg, G, p, vx, fe, W):
    """form_factor.py:163-298 for one lineout (tensors; see tsadar_oracle.form_factor)."""
    xi1, xi2 = orc.xi_grids()
    zr_tab, zi_tab = orc.zprime_tables()
    lam_axis = np.linspace(lam_range[0], lam_range[1], npts)
    omgL_num = 2 * np.pi * 1e7 * orc.C
    omgs = _t(2e7 * np.pi * orc.C / lam_axis)[None, :, None]
    lin = lambda v: (1 - v / 200) + (torch.arange(G, dtype=DT) * ((v / 100) / (G - 1)) if G > 1 else torch.zeros(1, dtype=DT))
    ne = 1.0e20 * p["ne"] * lin(p["ne_gradient"])
    Te = p["Te"] * lin(p["Te_gradient"])
    lam = p["lam"] + lam_shift
    A = torch.stack([_t(a) for a in p["A"]])
    Z = torch.stack(list(p["Z"])).reshape(1, 1, 1, -1)
    Ti = torch.stack(list(p["Ti"]))
    fract = torch.stack(list(p["fract"])).reshape(1, 1, 1, -1)
    Va = p["Va"] * 1e6
    ud = p["ud"] * 1e6
    Mi = (A * orc.MP).reshape(1, 1, 1, -1)
    sarad = _t(np.asarray(sa_deg) * np.pi / 180).reshape(1, 1, -1)
    omgL = omgL_num / lam
    omgpe = orc.C0 * torch.sqrt(ne[:, None, None])
    omg = omgs - omgL
    ks = torch.sqrt(omgs**2 - omgpe**2) / orc.C
    kL = torch.sqrt(omgL**2 - omgpe**2) / orc.C
    k = torch.sqrt(ks**2 + kL**2 - 2 * ks * kL * torch.cos(sarad))
    omgdop = omg - k * Va
    vTe = torch.sqrt(Te[:, None, None] / orc.ME)
    klde = (vTe / omgpe) * k
    Zbar = torch.sum(Z * fract)
    ni = fract * ne[:, None, None, None] / Zbar
    omgpi = orc.C0 * Z * torch.sqrt(ni * orc.ME / Mi)
    vTi = torch.sqrt(Ti.reshape(1, 1, 1, -1) / Mi)
    kldi = (vTi / omgpi) * k[..., None]
    xii = (1.0 / (np.sqrt(2.0) * vTi)) * (omgdop / k)[..., None]
    ZpiR = interp_linear(xii, xi2, zr_tab, left=xii**-2, right=xii**-2)
    ZpiI = interp_linear(xii, xi2, zi_tab, left=torch.zeros_like(xii), right=torch.zeros_like(xii))
    chiIr = torch.sum(-0.5 / kldi**2 * ZpiR, dim=3)
    chiIi = torch.sum(-0.5 / kldi**2 * ZpiI, dim=3)
    xie = omgdop / (k * vTe) - ud / vTe
    fe_vphi = torch.exp(interp_hermite(xie, vx, torch.log(fe), -50.0, -50.0))
    df = (fe_vphi[:, 1:, :] - fe_vphi[:, :-1, :]) / (xie[:, 1:, :] - xie[:, :-1, :])
    df = torch.cat([df, torch.zeros((G, 1, df.shape[2]), dtype=DT)], dim=1)
    chiEi = np.pi / klde**2 * df
    chiEr = -1.0 / klde**2 * interp_linear(xie, xi2, W)
    epsr = 1.0 + chiEr + chiIr
    epsi = chiEi + chiIi
    eps2 = epsr**2 + epsi**2
    ion_fact = fract * Z**2 / Zbar / vTi
    ion_comp = ion_fact * ((chiEr**2 + chiEi**2)[..., None] * torch.exp(-(xii**2)) / np.sqrt(2 * np.pi))
    ele_comp = ((1.0 + chiIr) ** 2 + chiIi**2) * fe_vphi / vTe
    S_ion = torch.sum(1.0 / k[..., None] * ion_comp / eps2[..., None], dim=3)
    S_ele = 1.0 / k * ele_comp / eps2
    PsOmg = (S_ion + S_ele) * (1 + 2 * omgdop / omgL) * orc.RE**2 * ne[:, None, None]
    lams = 2 * np.pi * orc.C / omgs
    return PsOmg * 2 * np.pi * orc.C / lams**2, lams[0, :, 0]


def _conv_same(x, g):
    n = x.numel()
    full = torch.nn.functional.conv1d(x.reshape(1, 1, -1), g.flip(0).reshape(1, 1, -1), padding=n - 1).reshape(-1)
    c = (n - 1) // 2
    return full[c : c + n]


def _conv_same_matrix(g):
    """The matrix T with T @ x = _conv_same(x, g) for len(x) = len(g) = n: T[i, j] = g[i + (n - 1) // 2 - j] inside the kernel,
    zero outside.  One product convolves every column of an image."""
    n = g.numel()
    k = torch.arange(n)[:, None] + (n - 1) // 2 - torch.arange(n)[None, :]
    return torch.where((k >= 0) & (k < n), g[k.clamp(0, n - 1)], torch.zeros((), dtype=DT))


def _irf(lam, modl, stddev):
    origin = (lam.max() + lam.min()) / 2.0
    g = (1.0 / (stddev * np.sqrt(2.0 * np.pi))) * torch.exp(-((lam - origin) ** 2.0) / (2.0 * stddev**2.0))
    y = _conv_same(modl, g)
    return (torch.amax(modl) / torch.amax(y)) * y


def ts_diag(cfg, sa, normed, batch, activate=True, fe_batch=None, tap=None):
    """thomson_diagnostic.py:109-142 with tensors; returns (ThryE, ThryI, lamE, lamI) [B, 1024].  ``tap``: a callable
    (b, feature, P) -> P called right after form_factor; what it returns goes on in P's place (loss_adjoint splits the chain there).
    Where f_e is differentiated it is also called as (b, "tables", (fe, W)) -> (fe, W) before the form factors of lineout b."""
    cfgp = cfg["parameters"]
    other = cfg["other"]
    ext = other["extraoptions"]
    phys = physical_params(cfgp, normed, activate)
    n_ion = len(orc.ion_species(cfgp))
    B = normed["Te"].numel()
    G = cfgp["general"]["Te_gradient"]["num_grad_points"]
    nvx = cfgp["electron"]["fe"]["nvx"]
    vx = orc.velocity_grid(nvx)
    w_ang = _t(np.asarray(sa["weights"])[0])
    outE, outI, lamE, lamI = [], [], [], []

    def col(name, b):
        v = _t(batch[name])
        if v.ndim == 0:
            return v
        v = v[b] if v.shape[0] == B else v
        return v.reshape(()) if v.ndim == 1 and v.shape[0] == 1 else v

    for b in range(B):
        p = {k: phys[k][b] for k in ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]}
        for k in ["Ti", "Z", "A", "fract"]:
            p[k] = [phys[f"{k}_{s+1}"][b] for s in range(n_ion)]
        if fe_batch is not None:
            fe = _t(fe_batch)
            fe = fe[b] if fe.ndim == 2 else fe
        else:
            fe = dlm_fe(phys["m"][b], nvx)
        W = chi_table(vx, fe) if fe.requires_grad else _t(orc.chi_table_cached(vx, fe.detach().numpy()))
        if tap is not None and fe.requires_grad:
            fe, W = tap(b, "tables", (fe, W))
        for feature in ("ion", "ele"):
            if not ext["load_ion_spec" if feature == "ion" else "load_ele_spec"]:
                continue
            rng, shift = (other["lamrangI"], 0.0) if feature == "ion" else (other["lamrangE"], cfg["data"]["ele_lam_shift"])
            P, lam_cm = form_factor(rng, other["npts"], shift, sa["sa"], G, p, vx, fe, W)
            if tap is not None:
                P = tap(b, feature, P)
            lam = lam_cm * 1e7
            modl = torch.sum(torch.mean(P, dim=0) * w_ang, dim=1)
            if feature == "ele":
                filt = other["iawfilter"]
                if filt[0]:
                    fb, fr = filt[3] - filt[2] / 2, filt[3] + filt[2] / 2
                    if other["lamrangE"][0] < fr and other["lamrangE"][1] > fb:
                        modl = torch.where((fb < lam) & (fr > lam), modl * 10.0 ** (-filt[1]), modl)
                y = _irf(lam, modl, other["PhysParams"]["widIRF"]["spect_stddev_ele"])
                y = y.reshape(1024, -1).mean(dim=1)
                lamb = lam.reshape(1024, -1).mean(dim=1)
                y = col("e_amps", b) * y / torch.amax(y)
                y = torch.where(lamb < p["lam"], p["amp1"] * y, p["amp2"] * y)
                outE.append(y + col("noise_e", b))
                lamE.append(lamb)
            else:
                if other["PhysParams"]["widIRF"]["spect_stddev_ion"]:
                    y = _irf(lam, modl, other["PhysParams"]["widIRF"]["spect_stddev_ion"])
                    y = y.reshape(1024, -1).mean(dim=1)
                    lamb = lam.reshape(1024, -1).mean(dim=1)
                    y = p["amp3"] * col("i_amps", b) * y / torch.amax(y)
                else:   # irf.py:82-86: no ion IRF -> ThryI = modlI (un-normalised, un-binned)
                    y, lamb = modl, lam
                outI.append(y + col("noise_i", b))
                lamI.append(lamb)
    z = torch.zeros((B, 1024), dtype=DT)
    st = lambda l: torch.stack(l) if l else z
    return st(outE), st(outI), st(lamE), st(lamI)


def masked_sums(cfg, sa, normed, batch, activate=True, fe_batch=None):
    """Un-normalised masked sums [S_iaw, S_blue, S_red] of the loss functional over the given lineouts,
    the number of fitted entries of each, and the spectra (loss_function.py:190-267 before the mean)."""
    ThryE, ThryI, lamE, lamI = ts_diag(cfg, sa, normed, batch, activate, fe_batch)
    S, N = _sums_of_spectra(cfg, batch, ThryE, ThryI, lamE, lamI)
    return S, N, ThryE, ThryI


def _sums_of_spectra(cfg, batch, ThryE, ThryI, lamE, lamI):
    """masked_sums from the spectra on: (S [3], N [3])."""
    ext = cfg["other"]["extraoptions"]
    method = cfg["optimizer"]["loss_method"]
    iaw, blue, red = orc.fit_masks(cfg, lamE.detach().numpy(), lamI.detach().numpy())

    def fun(d, t):
        d = _t(d)
        if method == "l1":
            return torch.abs(d - t)
        if method == "l2":
            return torch.square(d - t)
        if method == "log-cosh":
            return torch.log(torch.cosh(d - t))
        return t - d * torch.log(t)

    z = torch.zeros((), dtype=DT)
    S = [z, z, z]
    N = [0, 0, 0]
    if ext["fit_IAW"]:
        S[0], N[0] = fun(batch["i_data"], ThryI)[torch.as_tensor(iaw)].sum(), int(iaw.sum())
    if ext["fit_EPWb"]:
        S[1], N[1] = fun(batch["e_data"], ThryE)[torch.as_tensor(blue)].sum(), int(blue.sum())
    if ext["fit_EPWr"]:
        S[2], N[2] = fun(batch["e_data"], ThryE)[torch.as_tensor(red)].sum(), int(red.sum())
    return torch.stack(S), N


def loss(cfg, sa, normed, batch, i_norm, e_norm, activate=True, fe_batch=None):
    """loss_function.py:364-373 (nanmean over the masked entries of the whole batch)."""
    S, N, ThryE, ThryI = masked_sums(cfg, sa, normed, batch, activate, fe_batch)
    return _loss_of_sums(cfg, S, N, i_norm, e_norm), ThryE, ThryI


def _loss_of_sums(cfg, S, N, i_norm, e_norm):
    """loss from the masked sums on: the means, the halving, ion_loss_scale."""
    ext = cfg["other"]["extraoptions"]
    dep = cfg["optimizer"]["loss_method"] in ("l1", "l2")  # the other functionals ignore the denominator
    ui, ue = (i_norm**2, e_norm**2) if dep else (1.0, 1.0)
    i_err = S[0] / (N[0] * ui) if ext["fit_IAW"] else torch.zeros((), dtype=DT)
    e_err = torch.zeros((), dtype=DT)
    if ext["fit_EPWb"]:
        e_err = e_err + S[1] / (N[1] * ue)
    if ext["fit_EPWr"]:
        e_err = e_err + S[2] / (N[2] * ue)
        if ext["fit_EPWb"]:
            e_err = e_err * 0.5
    return cfg["data"]["ion_loss_scale"] * i_err + e_err


def hessian_loss(cfg, sa, normed, batch, activate=True):
    """``LossFunction._loss_for_hess_fn_`` (loss_function.py:173-188): denominators |data| + 1e-10, sum reduce,
    i_error + e_error (e_error halved when both EPW ranges are fitted, :262-264)."""
    ThryE, ThryI, lamE, lamI = ts_diag(cfg, sa, normed, batch, activate)
    ext = cfg["other"]["extraoptions"]
    iaw, blue, red = orc.fit_masks(cfg, lamE.detach().numpy(), lamI.detach().numpy())
    ed, idt = _t(batch["e_data"]), _t(batch["i_data"])
    fe = torch.square(ed - ThryE) / (torch.abs(ed) + 1e-10)
    fi = torch.square(idt - ThryI) / (torch.abs(idt) + 1e-10)
    i_err = fi[torch.as_tensor(iaw)].sum() if ext["fit_IAW"] else torch.zeros((), dtype=DT)
    e_err = torch.zeros((), dtype=DT)
    if ext["fit_EPWb"]:
        e_err = e_err + fe[torch.as_tensor(blue)].sum()
    if ext["fit_EPWr"]:
        e_err = e_err + fe[torch.as_tensor(red)].sum()
        if ext["fit_EPWb"]:
            e_err = e_err * 0.5
    return i_err + e_err


def hessian(cfg, sa, normed_np, batch, names, activate=True):
    """Dense Hessian [P, P] of hessian_loss w.r.t. the leaves ``names`` of a ONE-lineout batch (double backward)."""
    base = {k: _t(v).clone() for k, v in normed_np.items()}

    def f(vec):
        nm = dict(base)
        for i, k in enumerate(names):
            nm[k] = vec[i:i + 1]
        return hessian_loss(cfg, sa, nm, batch, activate)

    x0 = torch.cat([base[k].reshape(1) for k in names])
    return torch.autograd.functional.hessian(f, x0).numpy()


def value_and_grad(cfg, sa, normed_np, batch, i_norm, e_norm, names, activate=True, fe_batch=None):
    """(loss, {name: dloss/d normed[name]  [B]}, ThryE, ThryI) by reverse-mode autodiff."""
    normed = {k: _t(v).clone() for k, v in normed_np.items()}
    for k in names:
        normed[k].requires_grad_(True)
    val, E, I = loss(cfg, sa, normed, batch, i_norm, e_norm, activate, fe_batch)
    grads = torch.autograd.grad(val, [normed[k] for k in names], allow_unused=True)
    out = {k: (g.numpy() if g is not None else np.zeros_like(normed_np[k])) for k, g in zip(names, grads)}
    return float(val.detach()), out, E.detach().numpy(), I.detach().numpy()


def ff1d_adjoint(f, x, fe, Pbar, slots, want_fe=True, chunk=16):
    """The adjoint of the 1-D form factor of ONE lineout as the sum of its terms, and the sum of their absolute values:

      g[k] = sum_(g,i,a) Pbar[g,i,a] dP[g,i,a]/dx_k,   A[k]: |.| of every term

    ``f``: (px [NP], fe [nvx]) -> P [G, npts, n_angles], differentiable in both (tests/angular_twin.form_factor_fn: form_factor
    with chi_table of the same fe; every species its own leaf, ti_same all zero); ``x`` [NP] physical, ``fe`` [nvx], ``Pbar`` the
    seed, ``slots``: the entries of px to differentiate.  d P / d x is taken by forward mode, ``chunk`` unit directions at a time:
    the terms are per point, the chain is not cut further (the path of an f_e node through W and its direct path arrive summed).
    A is the scale at which two float64 summations of these terms may differ, entry by entry (as in ff2d_adjoint, loss_adjoint).
    Returns (g_phys [len(slots)], A_phys, g_fe [nvx], A_fe); the last two None without ``want_fe``."""
    x0, f0, Pb = _t(x), _t(fe), _t(np.asarray(Pbar, dtype=np.float64))
    ns, nvx = len(slots), f0.numel()
    n = ns + (nvx if want_fe else 0)
    TX, TF = torch.zeros((n, x0.numel()), dtype=DT), torch.zeros((n, nvx), dtype=DT)
    TX[torch.arange(ns), torch.as_tensor(list(slots))] = 1.0
    if want_fe:
        TF[ns + torch.arange(nvx), torch.arange(nvx)] = 1.0
    one = lambda tx, tf: torch.func.jvp(f, (x0, f0), (tx, tf))[1]
    g, A = [], []
    for lo in range(0, n, chunk):
        t = Pb[None] * torch.func.vmap(one)(TX[lo:lo + chunk], TF[lo:lo + chunk])   # [chunk, G, npts, n_angles]
        g.append(t.sum(dim=(1, 2, 3)))
        A.append(t.abs().sum(dim=(1, 2, 3)))
    g, A = torch.cat(g).numpy(), torch.cat(A).numpy()
    return (g[:ns], A[:ns], g[ns:], A[ns:]) if want_fe else (g, A, None, None)


def ff1d_reverse(f, x, fe, Pbar):
    """One backward of <Pbar, P>: (d / d px [NP], d / d fe [nvx]) -- what ff1d_adjoint's terms must sum to."""
    x0, f0 = _t(x).clone().requires_grad_(True), _t(fe).clone().requires_grad_(True)
    gx, gf = torch.autograd.grad((_t(np.asarray(Pbar, dtype=np.float64)) * f(x0, f0)).sum(), [x0, f0])
    return gx.numpy(), gf.numpy()


def value_and_grad_fe(cfg, sa, normed_np, batch, i_norm, e_norm, names, fe_batch, activate=True):
    """As value_and_grad plus d loss / d fe_batch [B, nvx]: what equinox.filter_value_and_grad yields for the
    leaves of a free-form distribution function before the generator's own chain rule (base.py:157-204)."""
    normed = {k: _t(v).clone() for k, v in normed_np.items()}
    for k in names:
        normed[k].requires_grad_(True)
    fe = _t(np.asarray(fe_batch)).clone().requires_grad_(True)
    val, E, I = loss(cfg, sa, normed, batch, i_norm, e_norm, activate, fe)
    grads = torch.autograd.grad(val, [normed[k] for k in names] + [fe], allow_unused=True)
    out = {k: (g.numpy() if g is not None else np.zeros_like(normed_np[k])) for k, g in zip(names, grads[:-1])}
    return float(val.detach()), out, grads[-1].numpy(), E.detach().numpy(), I.detach().numpy()


def _jacobian_rows(T, leaves, rows):
    """d T / d leaf[rows[r]] for every leaf: a tensor [len(leaves), len(rows)] + T.shape by the double-backward trick --
    h = grad(<T, v>, leaf) with the graph kept is linear in v, and grad(h[b], v) is d T / d leaf[b].  A leaf T does not depend on
    gives zeros."""
    J = torch.zeros((len(leaves), len(rows)) + tuple(T.shape), dtype=DT)
    if not T.requires_grad:
        return J
    v = torch.ones_like(T, requires_grad=True)
    h = torch.autograd.grad((T * v).sum(), leaves, create_graph=True, allow_unused=True)
    for k, hk in enumerate(h):
        if hk is None or not hk.requires_grad:
            continue
        for r, b in enumerate(rows):
            J[k, r] = torch.autograd.grad(hk[b], v, retain_graph=True)[0]
    return J


def _sparse_jacobian(P, x, chunk=256):
    """d P / d x for a table x [n] that every point of P reads a few nodes of: (node index, flat point index, value) of the
    non-zero entries, by the double-backward trick of _jacobian_rows, a chunk of nodes per backward."""
    v = torch.ones_like(P, requires_grad=True)
    h, = torch.autograd.grad((P * v).sum(), x, create_graph=True)
    n = x.numel()
    ii, pp, vv = [], [], []
    # the nodes some point reads, from random positive weights: a node that no point reads has an exactly zero row
    hr, = torch.autograd.grad((P * (1.0 + torch.rand_like(P))).sum(), x, retain_graph=True)
    nodes = torch.nonzero(hr, as_tuple=True)[0]
    for lo in range(0, nodes.numel(), chunk):
        sel = nodes[lo:lo + chunk]
        eye = torch.zeros((sel.numel(), n), dtype=DT)
        eye[torch.arange(sel.numel()), sel] = 1.0
        J, = torch.autograd.grad(h, v, grad_outputs=eye, retain_graph=True, is_grads_batched=True)
        J = J.reshape(sel.numel(), -1)
        i, q = torch.nonzero(J, as_tuple=True)
        ii.append(sel[i]); pp.append(q); vv.append(J[i, q])
    return torch.cat(ii), torch.cat(pp), torch.cat(vv)


def _adjoint_graph(cfg, sa, normed_np, batch, names, fe_batch, activate):
    """What loss_adjoint needs that no seed changes: the chain cut at P -- leaves -> P (stage 1; kept as its Jacobian, the graph of
    each form-factor call is dropped at once) and (P_leaf, leaves) -> T (stage 2; graph kept) -- and d T / d leaves at fixed P.
    Where the DLM order is a leaf the chain is cut once more, at the tables m -> (f_e, W) -> P: d P / d m of one point is a sum over
    the table nodes the point reads, whose terms cancel, and the terms of g[b, m] are then those of every (point, node)."""
    normed = {k: _t(v).clone() for k, v in normed_np.items()}
    leaves = [normed[k].requires_grad_(True) for k in names]
    B = normed["Te"].numel()
    P_leaf, JP, tables, JX = {}, {}, {}, {}

    def tap(b, feature, P):
        if feature == "tables":   # P = (fe, W): held as leaves; their own derivatives along m
            d = [_jacobian_rows(x, [normed["m"]], [b])[0, 0] for x in P]
            tables[b] = [x.detach().clone().requires_grad_(True) for x in P]
            JX[b] = dict(d=d, J={})
            return tuple(tables[b])
        JP[(b, feature)] = _jacobian_rows(P, leaves, [b])[:, 0]          # [K, G, npts, n_angles]
        if b in tables:
            JX[b]["J"][feature] = [_sparse_jacobian(P, x) for x in tables[b]]
        P_leaf[(b, feature)] = P.detach().clone().requires_grad_(True)
        return P_leaf[(b, feature)]

    E, I, lamE, lamI = ts_diag(cfg, sa, normed, batch, activate, fe_batch, tap=tap)
    JT = []
    for T in (E, I):   # [K, B, 1024]: lineout b's row of d T / d leaf[b] (the amplitudes; every other path runs through P)
        J = _jacobian_rows(T, leaves, list(range(B)))
        JT.append(torch.stack([J[:, b, b] for b in range(B)], dim=1))
    return dict(E=E, I=I, lamE=lamE.detach(), lamI=lamI.detach(), P_leaf=P_leaf, JP=JP, JE=JT[0], JI=JT[1], JX=JX)


def loss_adjoint(cfg, sa, normed_np, batch, i_norm, e_norm, names, seed_from=None, fe_batch=None, activate=True, cache=None):
    """The loss gradient as the sum of its terms, and the sum of their absolute values:

      g[b, k] = sum_(f,g,i,a) Pbar[f,g,i,a] dP[f,g,i,a]/dx_k + sum_(f,j) Tbar[f,j] (dT[f,j]/dx_k at fixed P),   A[b, k]: |.| of every term

    P: what form_factor returns (feature f, gradient point g, wavelength sample i, angle a), T: ThryE / ThryI, Tbar = d loss / d T,
    Pbar = d loss / d P.  A is the scale at which two float64 summations of these terms may differ, entry by entry (as in ff2d_adjoint).
    ``seed_from`` = (E, I): Tbar is the derivative of the loss functional (loss()'s own weights, masks and halving) at those spectra
    instead of the twin's own -- the adjoint of a device whose forward is pinned separately.  ``names``: the trainable leaves
    (a tied Ti is not one; its adjoint arrives in ion-1's; for ``m`` the terms are those of every (point, table node), see
    _adjoint_graph); ``cache``: a dict that keeps what does not depend on the seed.
    Returns (g [B, K], A [B, K], ThryE, ThryI)."""
    c = cache if cache is not None else {}
    if "E" not in c:
        c.update(_adjoint_graph(cfg, sa, normed_np, batch, names, fe_batch, activate))
    E, I = c["E"], c["I"]
    Es, Is = (E, I) if seed_from is None else (_t(np.asarray(seed_from[0])), _t(np.asarray(seed_from[1])))
    Es, Is = Es.detach().clone().requires_grad_(True), Is.detach().clone().requires_grad_(True)
    S, N = _sums_of_spectra(cfg, batch, Es, Is, c["lamE"], c["lamI"])
    Eb, Ib = torch.autograd.grad(_loss_of_sums(cfg, S, N, i_norm, e_norm), [Es, Is], allow_unused=True)
    Eb = torch.zeros_like(Es) if Eb is None else Eb
    Ib = torch.zeros_like(Is) if Ib is None else Ib
    keys = list(c["P_leaf"])
    Pbar = torch.autograd.grad((Eb * E).sum() + (Ib * I).sum(), [c["P_leaf"][k] for k in keys], retain_graph=True)
    B, K = E.shape[0], len(names)
    g, A = torch.zeros((B, K), dtype=DT), torch.zeros((B, K), dtype=DT)
    for (b, f), pb in zip(keys, Pbar):
        t = pb[None] * c["JP"][(b, f)]
        g[b] += t.sum(dim=(1, 2, 3))
        A[b] += t.abs().sum(dim=(1, 2, 3))
        if b in c["JX"]:   # the DLM order: Pbar[point] dP[point]/dx[node] dx[node]/dm over the nodes of f_e and of W
            for (i, q, v), d in zip(c["JX"][b]["J"][f], c["JX"][b]["d"]):
                t = pb.reshape(-1)[q] * v * d[i]
                g[b, names.index("m")] += t.sum()
                A[b, names.index("m")] += t.abs().sum()
    for Tb, J in ((Eb, c["JE"]), (Ib, c["JI"])):
        t = Tb[None] * J
        g += t.sum(dim=2).T
        A += t.abs().sum(dim=2).T
    return g.numpy(), A.numpy(), E.detach().numpy(), I.detach().numpy()


# ---------------------------------------------------------------------------------------------
# 2-D distribution functions: the twin of tsadar_oracle's restatement of FormFactor.calc_in_2D.  Every function below
# restates the NumPy oracle's function of the same name (tsadar_oracle.py), which cites the reference lines it follows.
# Cell indices and branches are taken from detached values; the query positions themselves stay differentiable.
# ---------------------------------------------------------------------------------------------
def approx_df_axis(x, f, axis):
    """tsadar_oracle.approx_df_axis: mean of the two adjacent secants, one-sided at the ends."""
    f = torch.movedim(f, axis, 0)
    d = (f[1:] - f[:-1]) / (x[1:] - x[:-1]).reshape((-1,) + (1,) * (f.ndim - 1))
    out = torch.cat([d[:1], 0.5 * (d[:-1] + d[1:]), d[-1:]], dim=0)
    return torch.movedim(out, 0, axis)


def interp2d_cubic_extrap(xq, yq, x, y, f):
    """tsadar_oracle.interp2d_cubic_extrap: bicubic Hermite patch, the boundary patch outside the grid."""
    x, y = _t(x), _t(y)
    fx = approx_df_axis(x, f, 0)
    fy = approx_df_axis(y, f, 1)
    fxy = approx_df_axis(y, fx, 1)
    i = torch.clamp(torch.searchsorted(x, xq.detach().contiguous(), right=True), 1, x.numel() - 1)
    j = torch.clamp(torch.searchsorted(y, yq.detach().contiguous(), right=True), 1, y.numel() - 1)
    dx = x[i] - x[i - 1]
    dy = y[j] - y[j - 1]
    tx = (xq - x[i - 1]) / dx
    ty = (yq - y[j - 1]) / dy

    def basis(t):
        t2, t3 = t * t, t * t * t
        return (2 * t3 - 3 * t2 + 1, -2 * t3 + 3 * t2), (t3 - 2 * t2 + t, t3 - t2)

    (hx0, hx1), (gx0, gx1) = basis(tx)
    (hy0, hy1), (gy0, gy1) = basis(ty)
    out = 0.0
    for a, (hxa, gxa) in enumerate(((hx0, gx0), (hx1, gx1))):
        for b, (hyb, gyb) in enumerate(((hy0, gy0), (hy1, gy1))):
            ii, jj = i - 1 + a, j - 1 + b
            out = out + f[ii, jj] * hxa * hyb + fx[ii, jj] * dx * gxa * hyb + fy[ii, jj] * dy * hxa * gyb \
                + fxy[ii, jj] * dx * dy * gxa * gyb
    return out


def rotate_df(vx, df, angle_deg):
    """tsadar_oracle.rotate_df; ``angle_deg`` may be a tensor (differentiable)."""
    vx = _t(vx)
    rad = -_t(angle_deg) * (np.pi / 180)
    c, s = torch.cos(rad), torch.sin(rad)
    X, Y = torch.meshgrid(vx, vx, indexing="ij")
    xq = c * X + s * Y
    yq = -s * X + c * Y
    return interp2d_cubic_extrap(xq.reshape(-1), yq.reshape(-1), vx, vx, df).reshape(vx.numel(), vx.numel())


def calc_chi_vals_2d(vx, DF, beta, xie_mag, klde_mag):
    """tsadar_oracle.calc_chi_vals_2d for one (lambda, theta) point (0-dim tensors)."""
    vx = _t(vx)
    dvx = vx[1] - vx[0]
    fe_2D_k = rotate_df(vx, DF, beta * (180 / np.pi))
    fe_1D_k = torch.sum(fe_2D_k, dim=0) * dvx
    df = gradient_uniform(fe_1D_k, dvx)
    xq = xie_mag.reshape(1)
    fe_vphi = interp_linear(xq, vx, fe_1D_k)[0]
    dfe = interp_linear(xq, vx, df)[0]
    chiEI = np.pi / klde_mag**2 * dfe
    chiERrat = -1.0 / klde_mag**2 * ratintn(df, vx - xie_mag, vx)
    return fe_vphi, chiEI, chiERrat


def form_factor_2d(lam_range, npts, lam_shift, sa_deg, num_grad_points, p, vx, fe2d, ud_angle, va_angle, lam_index=None,
                   grad_index=None, debug=None, beta_of=None):
    """tsadar_oracle.form_factor_2d for one lineout: ``p`` holds tensors Te, ne, lam, Va, ud, ne_gradient, Te_gradient, lists
    of tensors Ti, Z, fract and plain numbers A; ``fe2d`` a tensor [nv, nv].  Returns (P[G, npts, ntheta], lam_cm), differentiable
    in all of them.  The points are walked one at a time, O(nv^2) each.  ``grad_index`` restricts the gradient points the
    way ``lam_index`` restricts the wavelengths (no coupling along either).  ``beta_of``: a map applied to the rotation angle
    before the table is rotated (only to restate the problem on a mirrored table, see ff2d_adjoint)."""
    _, xi2 = orc.xi_grids()
    zr_tab, zi_tab = orc.zprime_tables()
    G = num_grad_points
    lam_axis = np.linspace(lam_range[0], lam_range[1], npts)
    if lam_index is not None:
        lam_axis = lam_axis[np.asarray(lam_index)]
    omgL_num = 2 * np.pi * 1e7 * orc.C
    omgs = _t(2e7 * np.pi * orc.C / lam_axis)[None, :, None]
    # linspace(1 - v/200, 1 + v/200, G) = 1 + v * cg
    cg = _t(np.linspace(-1.0 / 200, 1.0 / 200, G))
    if grad_index is not None:
        cg = cg[np.asarray(grad_index)]
    ne = 1.0e20 * p["ne"] * (1 + p["ne_gradient"] * cg)
    Te = p["Te"] * (1 + p["Te_gradient"] * cg)
    lam = p["lam"] + lam_shift
    A = _t(np.asarray(p["A"], dtype=np.float64))
    Z = torch.stack(list(p["Z"])).reshape(1, 1, 1, -1)
    Ti = torch.stack(list(p["Ti"]))
    fract = torch.stack(list(p["fract"])).reshape(1, 1, 1, -1)
    Va0, ud0 = p["Va"] * 1e6, p["ud"] * 1e6
    Mi = (A * orc.MP).reshape(1, 1, 1, -1)
    sarad = _t(np.asarray(sa_deg, dtype=np.float64) * np.pi / 180).reshape(1, 1, -1)
    Va = (Va0 * np.cos(va_angle * np.pi / 180), Va0 * np.sin(va_angle * np.pi / 180))
    ud = (ud0 * np.cos(ud_angle * np.pi / 180), ud0 * np.sin(ud_angle * np.pi / 180))
    omgL = omgL_num / lam
    omgpe = orc.C0 * torch.sqrt(ne[:, None, None])
    omg = omgs - omgL
    kLx = torch.sqrt(omgL**2 - omgpe**2) / orc.C
    ks_mag = torch.sqrt(omgs**2 - omgpe**2) / orc.C
    kx, ky = torch.cos(sarad) * ks_mag - kLx, torch.sin(sarad) * ks_mag - 0.0
    k_mag = torch.sqrt(kx * kx + ky * ky)
    omgdop = omg - (kx * Va[0] + ky * Va[1])
    vTe = torch.sqrt(Te[:, None, None] / orc.ME)
    klde_mag = (vTe / omgpe) * k_mag
    Zbar = torch.sum(Z * fract)
    ni = fract * ne[:, None, None, None] / Zbar
    omgpi = orc.C0 * Z * torch.sqrt(ni * orc.ME / Mi)
    vTi = torch.sqrt(Ti.reshape(1, 1, 1, -1) / Mi)
    kldi = (vTi / omgpi) * k_mag[..., None]
    xii = (1.0 / (np.sqrt(2.0) * vTi)) * (omgdop / k_mag)[..., None]
    ZpiR = interp_linear(xii, xi2, zr_tab, left=xii**-2, right=xii**-2)
    ZpiI = interp_linear(xii, xi2, zi_tab, left=torch.zeros_like(xii), right=torch.zeros_like(xii))
    chiIr = torch.sum(-0.5 / kldi**2 * ZpiR, dim=3)
    chiIi = torch.sum(-0.5 / kldi**2 * ZpiI, dim=3)
    a = omgdop / k_mag**2
    xie = ((a * kx - ud[0]) / vTe, (a * ky - ud[1]) / vTe)
    xie_mag = torch.sqrt(xie[0] ** 2 + xie[1] ** 2)
    # np.heaviside(x, 1) = 1 for x >= 0: the half plane is chosen from the detached value
    beta = torch.atan(xie[1] / xie[0]) + np.pi * (xie[0].detach() < 0).to(DT)
    if debug is not None:
        debug.update(beta=beta.detach().numpy(), xie_mag=xie_mag.detach().numpy(), xii=xii.detach().numpy())
    if beta_of is not None:
        beta = beta_of(beta)
    shp = tuple(beta.shape)
    vals = [calc_chi_vals_2d(vx, fe2d, beta[idx], xie_mag[idx], klde_mag[idx]) for idx in np.ndindex(*shp)]
    fe_vphi, chiEi, chiEr = (torch.stack([v[c] for v in vals]).reshape(shp) for c in range(3))
    epsr = 1.0 + chiEr + chiIr
    epsi = chiEi + chiIi
    eps2 = epsr**2 + epsi**2
    ion_fact = fract * Z**2 / Zbar / vTi
    ion_comp = ion_fact * ((chiEr**2 + chiEi**2)[..., None] * torch.exp(-(xii**2)) / np.sqrt(2 * np.pi))
    ele_comp = ((1.0 + chiIr) ** 2 + chiIi**2) * fe_vphi / vTe
    S_ion = torch.sum(1.0 / k_mag[..., None] * ion_comp / eps2[..., None], dim=3)
    S_ele = 1.0 / k_mag * ele_comp / eps2
    PsOmg = (S_ion + S_ele) * (1 + 2 * omgdop / omgL) * orc.RE**2 * ne[:, None, None]
    lams = 2 * np.pi * orc.C / omgs
    return PsOmg * 2 * np.pi * orc.C / lams**2, lams[0, :, 0]


def phys_names_2d(n_ion):
    """The physical parameters of one lineout that the 2-D form factor depends on (A is a constant)."""
    return ["Te", "ne", "lam", "ud", "Va", "Te_gradient", "ne_gradient"] + [f"{k}_{s+1}" for s in range(n_ion) for k in ("Ti", "Z", "fract")]


def _leaf_params(p_np, names):
    """Oracle lineout dict (tsadar_oracle.lineout_params) -> the same dict of 0-dim tensors, and the leaves named ``names``."""
    p = {k: _t(p_np[k]).clone() for k in ["Te", "ne", "lam", "ud", "Va", "Te_gradient", "ne_gradient"]}
    for k in ["Ti", "Z", "fract"]:
        p[k] = [_t(v).clone() for v in p_np[k]]
    p["A"] = list(p_np["A"])
    leaves = []
    for nm in names:
        if "_" in nm and nm.rsplit("_", 1)[1].isdigit():
            k, s = nm.rsplit("_", 1)
            leaves.append(p[k][int(s) - 1].requires_grad_(True))
        else:
            leaves.append(p[nm].requires_grad_(True))
    return p, leaves


def ff2d_adjoint(lam_range, npts, lam_shift, sa_deg, num_grad_points, lineouts, vx, fe2d, ud_angle, va_angle, lam_index, Pbar,
                 names, points=None, mirrored=False):
    """Reverse mode of J = sum Pbar * P over the seeded points of form_factor_2d, one backward per point.

    ``lineouts``: one oracle parameter dict per lineout (tsadar_oracle.lineout_params); ``Pbar`` [B, G, len(lam_index), ntheta]
    (a point whose seed is exactly zero is not visited); ``names``: the parameters to differentiate (phys_names_2d).
    ``points``: optional list of (b, g, l, t) -- the contribution of those points only (l indexes ``lam_index``).
    ``mirrored``: the same mathematics in another summation order -- the transposed table rotated by the reflected angle
    -pi/2 - beta gives every projection with its summed axis reversed; the table gradient is transposed back.

    Returns (g_phys [B, len(names)], g_table [nv, nv], A_phys, A_table): the per-point gradients summed, and their absolute
    values summed.  ``A`` is the scale at which two float64 summations of the same terms may legitimately differ, entry by entry;
    max |g| is not (a handful of rim entries of the table carry weights orders of magnitude above the rest)."""
    Pbar = np.asarray(Pbar, dtype=np.float64)
    sa_deg = np.asarray(sa_deg, dtype=np.float64)
    lam_index = np.asarray(lam_index)
    B, nv = len(lineouts), len(vx)
    assert Pbar.shape == (B, num_grad_points, lam_index.size, sa_deg.size), Pbar.shape
    fe = _t(fe2d).clone()
    fe = (fe.T.contiguous() if mirrored else fe).requires_grad_(True)
    beta_of = (lambda beta: -np.pi / 2 - beta) if mirrored else None
    g_phys, A_phys = np.zeros((B, len(names))), np.zeros((B, len(names)))
    g_tab, A_tab = torch.zeros((nv, nv), dtype=DT), torch.zeros((nv, nv), dtype=DT)
    todo = points if points is not None else [idx for idx in np.ndindex(*Pbar.shape)]
    per_b = {}
    for (b, g, l, t) in todo:
        if Pbar[b, g, l, t] == 0.0:
            continue
        if b not in per_b:
            per_b[b] = _leaf_params(lineouts[b], names)
        p, leaves = per_b[b]
        P, _ = form_factor_2d(lam_range, npts, lam_shift, sa_deg[t : t + 1], num_grad_points, p, vx, fe, ud_angle, va_angle,
                              lam_index=lam_index[l : l + 1], grad_index=[g], beta_of=beta_of)
        grads = torch.autograd.grad(P.reshape(()), leaves + [fe], allow_unused=True)
        w = float(Pbar[b, g, l, t])
        for c, gr in enumerate(grads[:-1]):
            if gr is not None:
                g_phys[b, c] += w * float(gr)
                A_phys[b, c] += abs(w * float(gr))
        g_tab += w * grads[-1]
        A_tab += (w * grads[-1]).abs()
    if mirrored:
        g_tab, A_tab = g_tab.T.contiguous(), A_tab.T.contiguous()
    return g_phys, g_tab.numpy(), A_phys, A_tab.numpy()


# ---------------------------------------------------------------------------------------------
# Angular (ARTS) instrument chain: the twin of tsadar_oracle.ats_model / add_ats_irf / reduce_ats_to_resunit / ats_spectrum,
# differentiable in P, amp1 and amp2.  ``lam`` only selects between the two amplitudes (detached).
# ---------------------------------------------------------------------------------------------
def ats_model(cfg, weights, P, lam_nm):
    """tsadar_oracle.ats_model: P [G, npts, n_angles] -> modlE [n_px, npts]."""
    lam_nm = _t(lam_nm)
    modl = _t(weights) @ torch.mean(P, dim=0).T
    filt = cfg["other"]["iawfilter"]
    if filt[0]:
        fb, fr = filt[3] - filt[2] / 2, filt[3] + filt[2] / 2
        if cfg["other"]["lamrangE"][0] < fr and cfg["other"]["lamrangE"][1] > fb:
            modl = torch.where((fb < lam_nm) & (fr > lam_nm), modl * 10.0 ** (-filt[1]), modl)
    return modl


def add_ats_irf(cfg, ang_axis, lam_nm, modl):
    """tsadar_oracle.add_ats_irf: "same" convolutions along the angular-pixel axis, then the wavelength axis."""
    ang_axis, lam_nm = _t(ang_axis), _t(lam_nm)
    wid = cfg["other"]["PhysParams"]["widIRF"]
    s_lam, s_ang = wid["spect_FWHM_ele"] / 2.3548, wid["ang_FWHM_ele"] / 2.3548
    o_lam = (lam_nm.max() + lam_nm.min()) / 2.0
    o_ang = (ang_axis.max() + ang_axis.min()) / 2.0
    g_lam = (1.0 / (s_lam * np.sqrt(2.0 * np.pi))) * torch.exp(-((lam_nm - o_lam) ** 2.0) / (2.0 * s_lam**2.0))
    g_ang = (1.0 / (s_ang * np.sqrt(2.0 * np.pi))) * torch.exp(-((ang_axis - o_ang) ** 2.0) / (2.0 * s_ang**2.0))
    y = (_conv_same_matrix(g_ang) @ modl).T      # [npts, n_px]: every wavelength column along the pixel axis
    y = (_conv_same_matrix(g_lam) @ y).T        # [n_px, npts]: every pixel row along the wavelength axis
    return torch.amax(modl, dim=1, keepdim=True) / torch.amax(y, dim=1, keepdim=True) * y


def _block_means(y, step):
    """[average(y[:, i : i + step], axis=1) for i in range(0, y.shape[1], step)] as one array [blocks, rows]."""
    n = y.shape[1]
    if n % step == 0:
        return y.reshape(y.shape[0], n // step, step).mean(dim=2).T
    return torch.stack([torch.mean(y[:, i : i + step], dim=1) for i in range(0, n, step)])


def reduce_ats_to_resunit(cfg, y, lam_nm, n_lam_out, e_amps, p):
    """tsadar_oracle.reduce_ats_to_resunit; ``p``: lam (number), amp1, amp2 (tensors)."""
    lam_nm = _t(lam_nm)
    lam_step = round(y.shape[1] / n_lam_out)
    ang_step = round(y.shape[0] / cfg["other"]["CCDsize"][0])
    y = _block_means(y, lam_step)
    y = _block_means(y, ang_step)
    lam = _block_means(lam_nm[None, :], lam_step)[:, 0]
    y = y[cfg["data"]["lineouts"]["start"] : cfg["data"]["lineouts"]["end"], :]
    y = _t(e_amps) * y / torch.amax(y, dim=1, keepdim=True)
    y = torch.where(lam < float(p["lam"]), p["amp1"] * y, p["amp2"] * y)
    return y, lam


def ats_spectrum(cfg, weights, ang_axis, P, lam_nm, n_lam_out, e_amps, p):
    """tsadar_oracle.ats_spectrum."""
    modl = ats_model(cfg, weights, P, lam_nm)
    y = add_ats_irf(cfg, ang_axis, lam_nm, modl)
    return reduce_ats_to_resunit(cfg, y, lam_nm, n_lam_out, e_amps, p)


def ats_adjoint(cfg, weights, ang_axis, P, lam_nm, n_lam_out, e_amps, p, Ebar):
    """One backward of <Ebar, ats_spectrum(P, amp1, amp2)>: (Pbar [G, npts, n_angles], amp1_bar, amp2_bar)."""
    Pt = _t(np.asarray(P, dtype=np.float64)).clone().requires_grad_(True)
    a1 = _t(p["amp1"]).clone().requires_grad_(True)
    a2 = _t(p["amp2"]).clone().requires_grad_(True)
    y, _ = ats_spectrum(cfg, weights, ang_axis, Pt, lam_nm, n_lam_out, e_amps, dict(lam=p["lam"], amp1=a1, amp2=a2))
    gP, g1, g2 = torch.autograd.grad(torch.sum(_t(Ebar) * y), [Pt, a1, a2])
    return gP.numpy(), float(g1), float(g2)
