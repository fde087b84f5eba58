"""Shared helpers of the test-suite: synthetic lineouts, oracle <-> engine parameter layouts, the angular (ARTS) fit's host loop."""
from __future__ import annotations

import copy

import numpy as np

from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L
from tsadar_amd.params import SlotMap

P9 = dict(
    sa=np.linspace(53.637560, 66.1191, 10),
    weights=np.array([0.00702671050853565, 0.0391423809738300, 0.0917976667717670, 0.150308544660150,
                      0.189541011666141, 0.195351560740507, 0.164271879645061, 0.106526733030044,
                      0.0474753389486960, 0.00855817305526778]),
)


def sa_fit(B):
    """Scattering-angle dict as the fitting path builds it (lineouts.py:103): weights [B, ntheta]."""
    return dict(sa=P9["sa"], weights=P9["weights"] * np.ones([B, 10]))


_GENERAL_SLOT = {"lam": L.P_LAM, "amp1": L.P_AMP1, "amp2": L.P_AMP2, "amp3": L.P_AMP3,
                 "ne_gradient": L.P_NE_GRADIENT, "Te_gradient": L.P_TE_GRADIENT, "ud": L.P_UD, "Va": L.P_VA}


def slot_of(name: str) -> int:
    if name == "Te":
        return L.P_TE
    if name == "ne":
        return L.P_NE
    if name == "m":
        return L.P_M
    if name in _GENERAL_SLOT:
        return _GENERAL_SLOT[name]
    k, s = name.rsplit("_", 1)
    return L.P_ION0 + 4 * (int(s) - 1) + {"Ti": L.ION_TI, "Z": L.ION_Z, "A": L.ION_A, "fract": L.ION_FRACT}[k]


def normed_to_matrix(normed: dict, n_ion: int) -> np.ndarray:
    B = len(normed["Te"])
    X = np.zeros((B, L.n_params(n_ion)))
    X[:, L.P_M] = 2.0
    for k, v in normed.items():
        X[:, slot_of(k)] = v
    return X


def matrix_to_named(G: np.ndarray, names) -> dict:
    return {k: G[:, slot_of(k)] for k in names}


def random_lineouts(cfg, B, seed=20251004, activate=True, ranges=None):
    """Normalised leaves (oracle dict) of B lineouts with physical values drawn uniformly from
    the ranges of SURVEY.md section 8d (those of the reference's tests/test_inverse/test_1d_random.py:33-39
    and decks).  The draw is mapped through the exact inverse of the activation so that the
    physical value is the drawn one."""
    rng = np.random.default_rng(seed)
    cfgp = cfg["parameters"]
    sm = SlotMap(cfgp, activate)
    rg = dict(Te=(0.3, 1.5), ne=(0.1, 0.7), Ti_1=(0.05, 0.5), lam=(525.5, 527.5), amp1=(0.5, 2.5),
              amp2=(0.5, 2.5), amp3=(0.5, 2.5), Va=(-2.0, 2.0))
    if ranges:
        rg.update(ranges)
    normed = orc.init_normed_params(cfgp, B, activate)
    for name, (lo, hi) in rg.items():
        if name not in normed:
            continue
        s = slot_of(name)
        val = rng.uniform(lo, hi, B)
        u = (val - sm.shift[s]) / sm.scale[s]
        normed[name] = np.log(u / (1 - u)) if sm.sigmoid[s] else u
    return normed


def synthetic_batch(cfg, sa, B, seed=7, noise_level=0.01, activate=True):
    """'Measured' data for a fit test: the oracle forward model at independently drawn truth
    parameters plus 1 % Gaussian noise; amplitudes = row max inside the fit ranges
    (lineouts.py:127-150)."""
    truth = random_lineouts(cfg, B, seed=seed + 1000, activate=activate)
    unit = dict(e_amps=np.ones(B), i_amps=np.ones(B), noise_e=np.zeros((B, 1024)), noise_i=np.zeros((B, 1024)),
                e_data=np.ones((B, 1024)), i_data=np.ones((B, 1024)))
    E, I, lE, lI = orc.ts_diag(cfg, sa, truth, unit, activate)
    rng = np.random.default_rng(seed)
    E = E * (1 + noise_level * rng.standard_normal(E.shape))
    I = I * (1 + noise_level * rng.standard_normal(I.shape))
    iaw, blue, red = orc.fit_masks(cfg, lE, lI)
    e_amps = np.array([np.amax(E[b][blue[b] | red[b]]) for b in range(B)])
    i_amps = np.array([np.amax(I[b][iaw[b]]) if iaw[b].any() else 1.0 for b in range(B)])
    return dict(e_data=E, i_data=I, e_amps=e_amps, i_amps=i_amps,
                noise_e=0.01 * np.abs(rng.standard_normal((B, 1024))), noise_i=0.01 * np.abs(rng.standard_normal((B, 1024))))


def rel_err(a, b, floor=1e-12):
    """max |a-b| / max(|b|, floor * max|b| per row)."""
    a, b = np.asarray(a), np.asarray(b)
    scale = np.maximum(np.abs(b), floor * np.max(np.abs(b), axis=-1, keepdims=True))
    return float(np.max(np.abs(a - b) / scale))


def _twin_weighted_grad(cfg, sa, normed, batch, w, names, fe_batch=None):
    """d (sum_k w[k] S_k) / d leaves of the given lineouts by reverse-mode autodiff of the torch twin: the per-lineout gradient
    of the library's loss (weights fixed by the whole batch), whatever subset of lineouts is evaluated.
    -> (S [3], {leaf: gradient [n]}, d / d fe_batch [n, nvx] or None, ThryE, ThryI): tests/test_concurrency.py,
    test_per_lineout_tables_gpu.py"""
    import torch
    from oracle import tsadar_oracle_torch as ot

    nt = {k: ot._t(v).clone() for k, v in normed.items()}
    for k in names:
        nt[k].requires_grad_(True)
    fb = None if fe_batch is None else torch.tensor(fe_batch, dtype=torch.float64, requires_grad=True)
    S, _, E, I = ot.masked_sums(cfg, sa, nt, batch, True, fb)
    val = (torch.as_tensor(np.asarray(w, dtype=np.float64)) * S).sum()
    leaves = [nt[k] for k in names] + ([fb] if fb is not None else [])
    grads = torch.autograd.grad(val, leaves, allow_unused=True)
    out = {k: g.numpy() for k, g in zip(names, grads)}
    return S.detach().numpy(), out, (grads[-1].numpy() if fb is not None else None), E.detach().numpy(), I.detach().numpy()


def positions(cfg, sa, p, feature, ion=0, grad_point=None):
    """(xi_e, xi_i) [npts, n_angles] of one lineout's sweep over a feature: form_factor.py:215-253 as the oracle's form_factor().
    ``ion``: the species xi_i is of; ``grad_point``: the gradient point whose T_e and n_e the sweep runs at (None: the lineout's own,
    G = 1).  tests/test_table_edges_gpu.py, test_loss_grad_entries.py"""
    o = cfg["other"]
    rng = o["lamrangE"] if feature == 0 else o["lamrangI"]
    shift = cfg["data"].get("ele_lam_shift", 0.0) if feature == 0 else 0.0
    Te, ne = p["Te"], p["ne"]
    if grad_point is not None:   # linspace(1 - v / 200, 1 + v / 200, G)[grad_point]
        G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
        at = lambda v: np.linspace(1 - v / 200, 1 + v / 200, G)[grad_point]
        Te, ne = Te * at(p["Te_gradient"]), ne * at(p["ne_gradient"])
    omgs = (2e7 * np.pi * orc.C / np.linspace(rng[0], rng[1], o["npts"]))[:, None]
    omgL = 2 * np.pi * 1e7 * orc.C / (p["lam"] + shift)
    omgpe = orc.C0 * np.sqrt(1.0e20 * ne)
    ks = np.sqrt(omgs**2 - omgpe**2) / orc.C
    kL = np.sqrt(omgL**2 - omgpe**2) / orc.C
    k = np.sqrt(ks**2 + kL**2 - 2 * ks * kL * np.cos(np.asarray(sa["sa"]) * np.pi / 180)[None, :])
    omgdop = (omgs - omgL) - k * p["Va"] * 1e6
    vTe = np.sqrt(Te / orc.ME)
    vTi = np.sqrt(np.asarray(p["Ti"])[ion] / (np.asarray(p["A"])[ion] * orc.MP))
    return omgdop / (k * vTe) - p["ud"] * 1e6 / vTe, (1.0 / (np.sqrt(2.0) * vTi)) * (omgdop / k)


def node_distance(x, nodes):
    """distance of every x to the nearest node of a uniform grid, in cells (beyond the grid: to its end node)"""
    t = (np.asarray(x) - nodes[0]) / (nodes[1] - nodes[0])
    return np.abs(t - np.clip(np.round(t), 0, len(nodes) - 1))


# ---- the angular (ARTS) fit: tests/test_angular_loop_device.py, test_sph_generator_device.py, test_arb1v_generator_device.py
def _angular_sa(cfg):
    from tsadar_amd import calibration

    cfg["other"]["extraoptions"]["spectype"] = "angular"
    sa = calibration.get_scattering_angles(cfg)
    cfg["other"]["extraoptions"]["spectype"] = "angular_full"
    sa["angAxis"] = calibration.angular_pixel_axis()
    return sa


def _host_loop(config, all_data, sa):
    """The reference's loop body (loops.py:197-270) over LossFunction.vg_loss with tree.Adam / tree.RMSProp.  A saved state of a
    trained SphericalHarmonics also carries the generator's radial functions, as the reference's."""
    from tsadar_amd import ThomsonParams, tree
    from tsadar_amd.loss_function import LossFunction

    config = copy.deepcopy(config)
    config["optimizer"]["batch_size"] = 1
    lo = config["data"]["lineouts"]
    lo["start"] = int(lo["start"] / config["other"]["ang_res_unit"])
    lo["end"] = int(lo["end"] / config["other"]["ang_res_unit"])
    a, b = lo["start"], lo["end"]
    batch1 = {"e_data": all_data["e_data"][a:b, :], "e_amps": all_data["e_amps"][a:b, :], "i_data": all_data["i_data"],
              "i_amps": all_data["i_amps"], "noise_e": all_data["noiseE"][a:b, :], "noise_i": all_data["noiseI"][a:b, :]}
    loss_fn = LossFunction(config, sa, batch1)
    opt = config["optimizer"]
    solver = (tree.Adam if opt["method"] == "adam" else tree.RMSProp)(opt["learning_rate"])
    ts_params = ThomsonParams(config["parameters"], num_params=1, batch=False, activate=True)
    diff_params, static_params = tree.partition(ts_params, tree.get_filter_spec(config["parameters"], ts_params))
    opt_state = solver.init(diff_params)
    best_weights, epoch_loss, best_loss, num_g_wait, num_b_wait = {}, 0.0, 100.0, 0, 0
    losses, states, stopped = [], {}, None
    for i_epoch in range(opt["num_epochs"]):
        (val, aux), grad = loss_fn.vg_loss(diff_params, static_params, batch1)
        updates, opt_state = solver.update(grad, opt_state)
        diff_params = tree.apply_updates(diff_params, updates)
        epoch_loss = val
        losses.append(val)
        if epoch_loss < best_loss:
            if best_loss - epoch_loss < 0.000001:
                best_loss = epoch_loss
                best_weights = tree.combine(diff_params, static_params)
                num_g_wait += 1
                if num_g_wait > 5:
                    stopped = i_epoch
                    break
            elif epoch_loss > best_loss:
                num_b_wait += 1
                if num_b_wait > 5:
                    break
            else:
                best_loss = epoch_loss
                best_weights = tree.combine(diff_params, static_params)
                num_b_wait = 0
                num_g_wait = 0
        if opt["save_state"] and i_epoch % opt["save_state_freq"] == 0 and best_weights != {}:
            states[i_epoch] = best_weights.get_unnormed_params()
            if best_weights.slots.gen2d_active:
                states[i_epoch]["electron"]["flm"] = best_weights.sph.get_unnormed_params()["flm"]
    final = tree.combine(diff_params, static_params)
    return dict(best=best_weights, epoch_loss=epoch_loss, losses=np.array(losses), states=states, stopped=stopped, final=final)


def _rel(a, b, floor=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), max(floor, 1e-300)))) if a.size else 0.0


def _device(cfg, all_data, sa, **kw):
    from tsadar_amd import loops

    info = {}
    best, epoch_loss, loss_fn = loops.angular_loop(copy.deepcopy(cfg), all_data, sa, info=info, **kw)
    return best, epoch_loss, loss_fn, info


def _stage_records(eng, cfg, two_d, want_gfe=True):
    """The launch records of the entry points an epoch is made of, called one by one at the fit's shapes (one lineout, all its
    points; want_gfe: with the table adjoint / the f_e adjoint, as the fit of a deck asks for them)."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd import _lib as L

    torch = eng.torch
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    phys = tp.physical_matrix()
    p, gen, rows = phys[0], cfg["parameters"]["general"], eng._ats_shape[0]
    fe = np.ascontiguousarray(tp()["electron"]["fe"], dtype=np.float64)
    if two_d:
        fe = eng.dev(fe)
        P = eng.form_factor_2d(0, phys, fe, gen["ud"]["angle"], gen["Va"]["angle"], save=True)
    else:
        fe = fe.reshape(1, -1)
        P = eng.form_factor(0, phys, fe)
    rec = [eng.last_launch()]
    E = eng.ats_spectrum(P[0], np.ones(rows), p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2])
    rec.append(eng.last_launch())
    Pbar, _ = eng.ats_adjoint(P[0], np.ones(rows), p[L.P_LAM], p[L.P_AMP1], p[L.P_AMP2], torch.ones_like(E))
    rec.append(eng.last_launch())
    if two_d:
        eng.form_factor_2d_grad(0, phys, fe, Pbar.reshape(P.shape), gen["ud"]["angle"], gen["Va"]["angle"], want_table=want_gfe, use_saved=True)
    else:
        eng.form_factor_grad(0, phys, fe, Pbar.reshape(P.shape), want_fe=want_gfe)
    rec.append(eng.last_launch())
    torch.cuda.synchronize()
    return rec


# ---- the 2-D form factor's adjoint against the oracle's autodiff twin: tests/test_ff2d_adjoint_twin.py, test_oracle_torch.py
def fe2d(nv, kind="anisotropic"):
    """A normalised 2-D f_e on the velocity grid.  "anisotropic": super-Gaussian with a drifting bump, no symmetry left for a
    transposed or mirrored index to hide behind."""
    vx = orc.velocity_grid(nv)
    X, Y = np.meshgrid(vx, vx, indexing="ij")
    if kind == "maxwellian":
        f = np.exp(-(X**2 + Y**2) / 2)
    else:
        f = np.exp(-((X / 1.3) ** 2 + (Y / 0.8) ** 2) ** 1.4 / 2) + 0.05 * np.exp(-((X - 2.0) ** 2 + (Y + 1.0) ** 2))
    return vx, f / (f.sum() * (vx[1] - vx[0]) ** 2)


# Cases by table size.  lam: the seeded wavelength samples per feature (0: electron window, 1: ion window); drifts: (ud or None = the
# lineouts' own, ud_angle, va_angle).  In the electron window |xi_e| stays on the velocity grid for samples ~260 .. 620 only, and one
# sample of every list lies beside the laser line (sample 431 there): away from it every xi_i is beyond the Z' table, chi_i no longer
# depends on T_i, and d P / d T_i would be a rounding residue with no scale of its own.
_SA3 = [35.0, 60.0, 110.0]
_DRIFT1 = [(None, 25.0, -40.0)]
FF2D_TWIN_CASES = {
    48: dict(n_ion=2, G=3, sa=_SA3, lam={0: [262, 333, 431, 610], 1: [0, 100, 511, 700]}, drifts=_DRIFT1),
    129: dict(n_ion=1, G=1, sa=_SA3, lam={0: [300, 432], 1: [511]}, drifts=_DRIFT1),
    # the angles and drift settings of test_rolling_sampler_every_walk_direction; the laser line lies at sample 234.7 of the ion window
    132: dict(n_ion=1, G=1, sa=[25.0, 40.0, 62.0, 88.0, 115.0, 150.0], lam={1: [3, 231, 234, 235, 236, 239]},
              drifts=[(1.4, 25.0, -40.0), (1.4, 115.0, 200.0), (-1.2, 60.0, 10.0), (0.9, 290.0, 135.0)]),
    133: dict(n_ion=1, G=1, sa=_SA3, lam={0: [280, 430], 1: [236]}, drifts=_DRIFT1),
    257: dict(n_ion=1, G=1, sa=_SA3, lam={0: [300, 431], 1: [511, 1023]}, drifts=_DRIFT1),
    258: dict(n_ion=1, G=1, sa=_SA3, lam={0: [432, 600], 1: [100]}, drifts=_DRIFT1),
}


def ff2d_twin_case(nv):
    """CPU-side set-up of one case of FF2D_TWIN_CASES: deck, angles, two lineouts, table."""
    import decks

    c = FF2D_TWIN_CASES[nv]
    cfg = decks.deck_fit(n_ion=c["n_ion"])
    if c["G"] > 1:
        g = cfg["parameters"]["general"]
        g["Te_gradient"].update(val=6.0, num_grad_points=c["G"])
        g["ne_gradient"].update(val=9.0, num_grad_points=c["G"])
    B = 2
    sa = dict(sa=np.array(c["sa"]), weights=np.ones((B, len(c["sa"]))) / len(c["sa"]))
    normed = random_lineouts(cfg, B, seed=67, ranges=dict(ud=(-1.5, 1.5)))
    phys = orc.physical_params(cfg["parameters"], normed, True)
    phys["ud"] = np.array([0.8, -1.1])
    vx, fe2 = fe2d(nv)
    return dict(cfg=cfg, sa=sa, B=B, G=c["G"], n_ion=c["n_ion"], phys=phys, vx=vx, fe2=fe2, lam=c["lam"], drifts=c["drifts"], nv=nv)


def ff2d_with_drift(case, ud):
    """The physical parameters of a case at one drift setting: (dict, matrix [B, NP], one oracle dict per lineout)."""
    phys = dict(case["phys"])
    if ud is not None:
        phys["ud"] = np.array([ud, -0.7 * ud])
    X = normed_to_matrix(phys, case["n_ion"])
    return phys, X, [orc.lineout_params(phys, b, case["n_ion"]) for b in range(case["B"])]


def ff2d_lam_range(case, feature):
    return case["cfg"]["other"]["lamrangE" if feature == 0 else "lamrangI"]


def ff2d_kink_distances(case, feature, lineouts, ud_angle, va_angle):
    """How far the seeded points of one feature lie from the kinks of the forward, from the NumPy oracle's own intermediates:
    (beta [B, G, nl, ntheta], distance of |xi_e| to the nearest vx node in cells -- negative outside the grid --, distance of
    every xi_i inside the Z' table to its nearest node in cells).  Runs no rotation: the table is 4 x 4."""
    vx = case["vx"]
    dv = vx[1] - vx[0]
    _, xi2 = orc.xi_grids()
    beta, de, di = [], [], []
    vx4, f4 = fe2d(4, "maxwellian")
    for p in lineouts:
        dbg = {}
        orc.form_factor_2d(ff2d_lam_range(case, feature), 1024, 0.0, case["sa"]["sa"], case["G"], p, vx4, f4, ud_angle, va_angle,
                           lam_index=np.array(case["lam"][feature]), debug=dbg)
        beta.append(dbg["beta"])
        t = (dbg["xie_mag"] - vx[0]) / dv
        de.append(np.where((t < 0) | (t > len(vx) - 1), -1.0, np.abs(t - np.round(t))))
        u = (dbg["xii"] - xi2[0]) / (xi2[1] - xi2[0])
        di.append(np.where((u < 0) | (u > len(xi2) - 1), np.inf, np.abs(u - np.round(u))))
    return np.array(beta), np.array(de), np.array(di)


def smooth_positive_image(shape, seed):
    """A random, positive, smooth image P [G, npts, n_angles] for the ARTS chain: a few low-frequency waves on a constant
    (generic: no ties among the row maxima the chain normalises by)."""
    rng = np.random.default_rng(seed)
    G, n, m = shape
    x, y = np.linspace(0, 1, n)[None, :, None], np.linspace(0, 1, m)[None, None, :]
    P = np.full(shape, 1.5)
    for _ in range(6):
        fx, fy = rng.uniform(0.3, 3.0, 2)
        P = P + rng.uniform(0.05, 0.2) * np.cos(2 * np.pi * (fx * x + fy * y) + rng.uniform(0, 2 * np.pi, (G, 1, 1)))
    return P
