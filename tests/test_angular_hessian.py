"""tsff_angular_loss_hess / Engine.angular_loss_hess / LossFunction.angular_h_loss_wrt_params: the exact Hessian of the reference's
``_loss_for_hess_fn_`` on an angular (ARTS) deck with a 1-D f_e, in one device call.

The yardstick is the torch twin as it stands: ``_image_fn`` / ``_setup`` of tests/test_angular_postfit.py (``at.form_factor_fn``,
``ot.chi_table``, ``ot.ats_spectrum``) for the small six-leaf deck, and the same composition written for any ion count for the other
decks.  The loss Hessian is ``torch.autograd.functional.hessian``, the second derivative of the image for a pair of leaves a nested
``functional.jvp``; every twin quantity is computed once per module and never modified.  Difference quotients are no yardstick here:
a quotient of the twin's own Jacobian is off by up to 1e-3 on (lam, Te), because samples cross table cells inside the step.

Every entry of H is held to HESS_TOL of sqrt(|H_aa H_cc|) of the twin -- the bar of tests/test_hessian_exact.py on the scale of
test_angular_gauss_newton_matches_twin (absolute values: an l1 Hessian has no positive diagonal); every image row of a derivative image
to at.ROW_TOL of that row's largest entry in the twin.

The model image E is compared bit for bit with tsff_ats_spectrum of tsff_form_factor where both calls exist on one handle (an explicit
f_e table: test_pairs_without_form_factor_launch_nothing, test_ion_counts_and_ties); on a DLM handle tsff_form_factor does not exist
(it takes explicit tables), and E is held to the twin's image at the bound test_angular_jacobian_matches_twin uses."""
import copy
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import angular_twin as at
import decks
import util
import test_angular_postfit as ap
from oracle import tsadar_oracle as orc
from tsadar_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsadar_amd", "csrc")
RECORD = os.path.join(ROOT, "profiles", "angular_hessian_pytest.txt")
HESS_TOL = 1e-7   # tests/test_hessian_exact.py
LEAVES = ["Te", "ne", "m", "lam", "amp1", "amp2"]
METHODS = ["l2", "l1", "log-cosh", "poisson"]
PAIRS = [("Te", "Te"), ("Te", "ne"), ("m", "m"), ("m", "Te"), ("lam", "lam"), ("lam", "amp1"), ("amp1", "amp1"), ("Te", "amp2")]

# The sigmas of the l2 Hessian (condition ~1e7).  MEASURED_ENTRY_ERR: the largest |H - H_twin| / sqrt(|H_aa H_cc|) the four cases of
# test_hessian_matches_twin measured on an MI355X (profiles/angular_hessian_pytest.txt).  SIGMA_BOUND: the largest relative change of
# a sigma of the TWIN's l2 Hessian under symmetric noise of ten times that size on the same scale, 100 draws, seed 0 (_sigma_bound
# below; test_sigma_bound_is_reproducible recomputes it on the CPU).
MEASURED_ENTRY_ERR = 8.8e-10
SIGMA_BOUND = 1.4e-4   # (_sigma_bound gave 1.379e-4; the sigmas of the l2 case moved by 8.1e-10)

# the launch plan of k_ffhess (tsff_api.inc): grid (pairs, angle chunks), chunks = min(n_angles, kFfhessWGPerCU * CUs / pairs)
FFHESS_WG_PER_CU = 4
N_ANGLES = 241    # the ARTS calibration (util._angular_sa)
CUS = 256         # MI355X

# every kernel the call adds and the GPU case that launches it
KERNELS = {
    "k_ffhess<1>": "test_hessian_matches_twin[l2]",
    "k_ffhess<2>": "test_ion_counts_and_ties[2]",
    "k_ffhess<3>": "test_ion_counts_and_ties[3]",
    "k_ffhess<4>": "test_ion_counts_and_ties[4]",
    "k_ats_rownorm_jvp2": "test_second_order_image_rows",
    "k_ats_resunit_jvp2": "test_second_order_image_rows",
    "k_ats_hess_reduce": "test_hessian_matches_twin[l2]",
}


def record(key, text):
    """One line per case in profiles/angular_hessian_pytest.txt: the case's previous line is replaced."""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    lines = {}
    if os.path.exists(RECORD):
        lines = {l.split(" ", 1)[0]: l.rstrip("\n") for l in open(RECORD) if l.strip()}
    lines[key] = f"{key} {text}"
    with open(RECORD, "w") as f:
        f.write("".join(v + "\n" for _, v in sorted(lines.items())))


def pair_index(a, c, n):
    """(a <= c) row-major over the upper triangle: hess_pair's order"""
    return a * n - a * (a - 1) // 2 + (c - a)


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _functional(method, d, t):
    """the functional of _loss_for_hess_fn_ (loss_function.py:170-188): |d| + 1e-10 under l2 and l1"""
    import torch

    if method == "l1":
        return torch.abs(d - t) / (torch.abs(d) + 1e-10)
    if method == "l2":
        return torch.square(d - t) / (torch.abs(d) + 1e-10)
    if method == "log-cosh":
        return torch.log(torch.cosh(d - t))
    return t - d * torch.log(t)


def _wcol(cfg, lam):
    """sum reduce over the blue and red masks of the resolution-unit axis, halved when both are fitted"""
    r, ext = cfg["data"]["fit_rng"], cfg["other"]["extraoptions"]
    c = 0.5 if (ext["fit_EPWb"] and ext["fit_EPWr"]) else 1.0
    w = np.zeros(lam.size)
    if ext["fit_EPWb"]:
        w += c * ((lam > r["blue_min"]) & (lam < r["blue_max"]))
    if ext["fit_EPWr"]:
        w += c * ((lam > r["red_min"]) & (lam < r["red_max"]))
    return w


def _twin_of_image(F, x0, w, d, noise, method):
    """-> (loss, grad [n], H [n, n]) of sum_j w_j l(d_j, F(x)_j + noise_j) at x0 by torch autograd"""
    import torch
    from oracle import tsadar_oracle_torch as ot

    wt, dt, nt = ot._t(w)[None, :], ot._t(d), ot._t(noise)
    sel = wt[0] > 0

    def loss(x):
        t = F(x) + nt
        return torch.sum((wt * _functional(method, dt, t))[:, sel])   # (poisson's log of a column outside the fit ranges is not asked for)

    H = torch.autograd.functional.hessian(loss, x0)
    x = x0.clone().requires_grad_(True)
    val = loss(x)
    g, = torch.autograd.grad(val, x)
    return float(val.detach()), g.numpy(), H.numpy()


@functools.lru_cache(maxsize=None)
def _twin_small(method):
    """The six-leaf deck of tests/test_angular_postfit.py: the twin's loss, gradient and Hessian for one loss method."""
    lf, tp, batch = ap._loss_fn(False)
    names, x0, F = ap._image_fn(False, tp)
    assert names == LEAVES
    cfg, _, _, lam = ap._setup(False)
    return _twin_of_image(F, x0, _wcol(cfg, lam), batch["e_data"], batch["noise_e"], method)


@functools.lru_cache(maxsize=None)
def _twin_second(a, c):
    """The twin's second derivative of the image w.r.t. the leaves a and c of the six-leaf deck: a nested jvp."""
    import torch

    _, tp, _ = ap._loss_fn(False)
    _, x0, F = ap._image_fn(False, tp)
    va, vc = torch.zeros_like(x0), torch.zeros_like(x0)
    va[a] = 1.0
    vc[c] = 1.0
    inner = lambda x: torch.autograd.functional.jvp(F, x, va, create_graph=True)[1]
    return torch.autograd.functional.jvp(inner, x0, vc)[1].detach().numpy()


def _gauss_newton(Jt, w, d, t, method):
    """sum_j w_j l''(d_j, t_j) J_a J_c of the twin's Jacobian"""
    res = d - t
    if method == "l2":
        e2 = 2.0 / (np.abs(d) + 1e-10)
    elif method == "l1":
        e2 = np.zeros_like(d)
    elif method == "log-cosh":
        e2 = 1.0 - np.tanh(res) ** 2
    else:
        e2 = d / (t * t)
    return np.einsum("arc,rc,brc->ab", Jt, w[None, :] * e2, Jt)


def _first_derivative(d, t, method):
    res = d - t
    if method == "l2":
        return -2.0 * res / (np.abs(d) + 1e-10)
    if method == "l1":
        return -np.sign(res) / (np.abs(d) + 1e-10)
    if method == "log-cosh":
        return -np.tanh(res)
    return 1.0 - d / t


def _sigmas(H):
    inv = np.linalg.inv(H)
    return np.sign(np.diag(inv)) * np.sqrt(np.abs(np.diag(inv)))


def _sigma_bound(Ht, entry_err, draws=100, seed=0):
    """The largest relative change of a sigma of Ht under symmetric noise of 10 x entry_err x sqrt(|H_aa H_cc|)."""
    rng = np.random.default_rng(seed)
    sc = np.sqrt(np.abs(np.outer(np.diag(Ht), np.diag(Ht))))
    s0 = _sigmas(Ht)
    worst = 0.0
    for _ in range(draws):
        N = rng.standard_normal(Ht.shape)
        N = 0.5 * (N + N.T)
        worst = max(worst, float(np.max(np.abs(_sigmas(Ht + 10.0 * entry_err * sc * N) - s0) / np.abs(s0))))
    return worst


# ---- decks with more ion species, ties, gradient points: the same composition for any ion count ----
def _ions(cfg, n_ion, tie=None, fract_active=False):
    P = cfg["parameters"]
    species = [(8.0, 14.0, 0.2, 0.4), (1.0, 1.0, 0.3, 0.3), (6.0, 12.0, 0.25, 0.2), (2.0, 4.0, 0.35, 0.1)][:n_ion]
    tot = sum(s[3] for s in species)
    for s, (Z, A, Ti, fr) in enumerate(species):
        P[f"ion-{s + 1}"] = {"Ti": decks._p(Ti, True, 0.01, 1.0, same=(tie == s)), "Z": decks._p(Z, True, 0.5, 25.0),
                             "A": {"val": A, "active": False}, "fract": {"val": fr / tot, "active": bool(fract_active)}}


def _grad3(cfg):
    g = cfg["parameters"]["general"]
    g["Te_gradient"].update(val=6.0, num_grad_points=3, active=True)
    g["ne_gradient"].update(val=9.0, num_grad_points=3)


# n_ion -> (deck modifiers, the leaves by their oracle names, fe_mode)
ION_CASES = {
    # Ti of ion 2 tied to ion 1's, Z and a fraction (sigmoid, then the renormalisation) among the leaves: tie_and_renorm at second
    # order; four leaves reach the form factor -> 10 pairs, 102 angle chunks.  (No Ti among the leaves of these cases: the electron
    # feature does not feel an ion temperature -- the twin's own second derivative w.r.t. one is rounding noise, 1e-13 against 1e8
    # for Te -- so there is no scale to hold such an entry to.)
    2: (lambda cfg: _ions(cfg, 2, tie=1, fract_active=True), ["Te", "m", "Z_2", "fract_1"], "dlm"),
    # three gradient points with Te_gradient a leaf; an explicit table (fe_mode PER_LINEOUT): 3 pairs, one angle per workgroup
    3: (lambda cfg: (_ions(cfg, 3), _grad3(cfg)), ["Te_gradient", "Z_3"], "table"),
    # no m, on a shared table (fe_mode SHARED)
    4: (lambda cfg: (_ions(cfg, 4, tie=2), cfg["parameters"]["electron"]["fe"].update(active=False)), ["ne", "Z_4"], "shared"),
}


# the six-leaf deck without m among the leaves (f_e not fitted): LossFunction runs it on the deck's own engine, the table explicit
NO_M_CASE = (lambda cfg: cfg["parameters"]["electron"]["fe"].update(active=False), ["Te", "ne", "lam", "amp1", "amp2"], "table")


@functools.lru_cache(maxsize=None)
def _ion_case(n_ion):
    """-> dict(cfg, sa, keys, mode, X [NP] the normalised leaf row, e_data, noise, e_amps, lam, x0, F, twin (loss, grad, H))"""
    import torch
    from oracle import tsadar_oracle_torch as ot

    mods, keys, mode = NO_M_CASE if n_ion == "no_m" else ION_CASES[n_ion]
    cfg = decks.deck_angular(1, ap.NVX, ap.CCD, ap.START, ap.END)
    mods(cfg)
    n_ion = len(orc.ion_species(cfg["parameters"]))
    sa = util._angular_sa(cfg)
    normed = orc.init_normed_params(cfg["parameters"], 1, True)
    base = {k: ot._t(v) for k, v in normed.items()}
    other = cfg["other"]
    G = cfg["parameters"]["general"]["Te_gradient"]["num_grad_points"]
    vx = ot._t(orc.velocity_grid(ap.NVX))
    lam_nm = np.linspace(*other["lamrangE"], 1024)
    e_amps = np.random.default_rng(3).uniform(0.5, 2.0, (ap.ROWS, 1))

    def image(nm):
        phys = ot.physical_params(cfg["parameters"], nm, True)
        p = {k: phys[k][0] for k in ["Te", "ne", "lam", "amp1", "amp2", "amp3", "ne_gradient", "Te_gradient", "ud", "Va"]}
        for k in ["Ti", "Z", "A", "fract"]:
            p[k] = [phys[f"{k}_{s + 1}"][0] for s in range(n_ion)]
        fe = ot.dlm_fe(phys["m"][0], ap.NVX)
        P, _ = ot.form_factor(other["lamrangE"], other["npts"], cfg["data"]["ele_lam_shift"], sa["sa"], G, p, vx, fe, ot.chi_table(vx, fe))
        return ot.ats_spectrum(cfg, sa["weights"], sa["angAxis"], P, lam_nm, ap.N_LAM, e_amps,
                               dict(lam=float(p["lam"].detach()), amp1=p["amp1"], amp2=p["amp2"]))

    def F(x):
        nm = dict(base)
        for i, k in enumerate(keys):
            nm[k] = x[i:i + 1]
        return image(nm)[0]

    # the data: the twin's image at Te - 0.2, ne + 0.12 (normalised), as _setup builds its own: the large residual is the point
    truth = dict(base)
    truth["Te"] = truth["Te"] - 0.2
    truth["ne"] = truth["ne"] + 0.12
    with torch.no_grad():
        data, lam = image(truth)
    data, lam = data.numpy(), lam.numpy()
    noise = 0.01 * np.abs(np.random.default_rng(4).standard_normal((ap.ROWS, ap.N_LAM)))
    x0 = torch.cat([base[k] for k in keys])
    twin = _twin_of_image(F, x0, _wcol(cfg, lam), data, noise, "l2")
    X = util.normed_to_matrix(normed, n_ion)[0]
    m_phys = float(orc.physical_params(cfg["parameters"], normed, True)["m"][0])
    return dict(cfg=cfg, sa=sa, keys=keys, mode=mode, X=X, e_data=data, noise=noise, e_amps=e_amps, lam=lam, twin=twin, m=m_phys)


def _hess_ok(H, Ht):
    sc = np.sqrt(np.abs(np.outer(np.diag(Ht), np.diag(Ht))))
    ratio = np.abs(H - Ht) / sc
    return ratio, bool(np.all(np.abs(H - Ht) <= HESS_TOL * sc))


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_fire_before_an_engine_exists():
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    def check(lf, tp, batch, match):
        before = copy.deepcopy(lf.cfg)
        with pytest.raises(NotImplementedError, match=match):
            lf.angular_h_loss_wrt_params(tp, batch)
        assert lf.ts_diag._engines == {} and lf.cfg == before

    lf, tp, batch = ap._loss_fn(False)
    # the three 1-D calls keep refusing angular decks by name
    for call in (lambda: lf.jacobian(tp, batch), lambda: lf.gn_loss_wrt_params(tp, batch),
                 lambda: lf.h_loss_wrt_params(tp, batch, method="exact")):
        with pytest.raises(NotImplementedError, match="angular"):
            call()
    assert lf.ts_diag._engines == {}
    lf.distributed = True
    check(lf, tp, batch, "distributed")
    lf.distributed = False
    lf.multiplex_ang = True
    check(lf, tp, batch, "multiplexed")
    lf.multiplex_ang = False
    # a 2-D f_e deck
    cfg2 = decks.deck_angular(2, 32, ap.CCD, ap.START, ap.END)
    sa = ap._setup(False)[1]
    check(LossFunction(cfg2, sa, batch), ThomsonParams(cfg2["parameters"], 1, batch=False, activate=True), batch, "2-D")
    # a fitted Arbitrary1V.fval
    lff, tpf, bf = ap._loss_fn(True)
    check(lff, tpf, bf, "fval")
    # a 1-D deck
    cfg1 = decks.deck_fit()
    b1 = util.synthetic_batch(cfg1, util.sa_fit(2), 2, seed=1)
    check(LossFunction(cfg1, util.sa_fit(2), b1), ThomsonParams(cfg1["parameters"], 2, batch=True, activate=True), b1, "angular_full")


def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "tsff.h")).read()
    assert int(re.search(r"#define TSFF_ABI_VERSION (\d+)", header).group(1)) == L.ABI_VERSION >= 19
    decl = re.search(r"int tsff_angular_loss_hess\((.*?)\);", header, re.S).group(1)
    assert "tsff_angular_loss_hess" in L.EXPORTS
    assert len(L._SIGNATURES["tsff_angular_loss_hess"][1]) == len(decl.split(",")) == 18
    assert "loss_function.py:170-188" in header[header.index("Exact Hessian of the angular"):header.index("int tsff_angular_loss_hess")]
    from tsadar_amd import build

    build.build()
    lib = L.load()
    assert lib.tsff_abi_version() == L.ABI_VERSION and hasattr(lib, "tsff_angular_loss_hess")


def _library_kernels(path):
    data = open(path, "rb").read()
    found = re.findall(rb"_ZN4tsff\d+(?:k_ffhess|k_ats_hess|k_ats_\w+?_jvp2)\w*", data)
    mangled = sorted({m.decode()[:-3] if m.endswith(b".kd") else m.decode() for m in found})
    out = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^(void )?tsff::", "", s).split("(")[0] for s in out if s.strip()}


def test_every_new_kernel_has_a_case():
    from tsadar_amd import build

    have = _library_kernels(build.build())
    assert have == set(KERNELS), (sorted(have), sorted(KERNELS))
    tests = {k: v.split("[")[0] for k, v in KERNELS.items()}
    for k, name in tests.items():
        assert callable(globals().get(name)), (k, name)
    assert set(ION_CASES) == {2, 3, 4}


def test_second_order_normalisation_formulas_on_the_host():
    """A NumPy transcription of k_ats_rownorm_jvp2 and k_ats_resunit_jvp2 against the second derivative of the twin's add_ats_irf +
    reduce_ats_to_resunit (a nested jvp): a 16 x 64 image that depends on three parameters, linearly and quadratically, the third of
    which also drives amp1 through a sigmoid."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    npx, npts, n_lam, ccd0 = 16, 64, 32, 8
    cfg = decks.deck_angular(1, 64, (ccd0, n_lam), 1, 7)
    lam_step, ang_step, r0, r1 = npts // n_lam, npx // ccd0, 1, 7
    rng = np.random.default_rng(21)
    lam_nm = np.linspace(*cfg["other"]["lamrangE"], npts)
    ang = np.linspace(-6.0, 7.0, npx) + 0.1 * rng.standard_normal(npx)
    ang.sort()
    M0 = rng.uniform(0.5, 2.0, (npx, npts))
    D = rng.standard_normal((3, npx, npts)) * 0.3
    Q = rng.standard_normal((3, 3, npx, npts)) * 0.2
    Q = 0.5 * (Q + Q.transpose(1, 0, 2, 3))
    e_amps = rng.uniform(0.5, 2.0, (r1 - r0, 1))
    lam_split, a2 = float(lam_nm[npts // 2 + 1]) + 1e-3, 0.8
    x0 = ot._t(np.array([0.1, -0.2, 0.3]))

    def model(x):
        return ot._t(M0) + torch.einsum("i,irc->rc", x, ot._t(D)) + 0.5 * torch.einsum("i,j,ijrc->rc", x, x, ot._t(Q))

    def amp1(x):
        return 0.5 + 2.0 * torch.sigmoid(x[2])

    def F(x):
        y = ot.add_ats_irf(cfg, ang, lam_nm, model(x))
        return ot.reduce_ats_to_resunit(cfg, y, lam_nm, n_lam, e_amps, dict(lam=lam_split, amp1=amp1(x), amp2=ot._t(a2)))[0]

    def second(a, c):
        va, vc = torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        va[a] = 1.0
        vc[c] = 1.0
        inner = lambda x: torch.autograd.functional.jvp(F, x, va, create_graph=True)[1]
        return torch.autograd.functional.jvp(inner, x0, vc)[1].detach().numpy()

    # ---- the transcription ----
    wid = cfg["other"]["PhysParams"]["widIRF"]
    s_lam, s_ang = wid["spect_FWHM_ele"] / 2.3548, wid["ang_FWHM_ele"] / 2.3548
    g_lam = np.exp(-((lam_nm - (lam_nm.max() + lam_nm.min()) / 2.0) ** 2) / (2 * s_lam**2)) / (s_lam * np.sqrt(2 * np.pi))
    g_ang = np.exp(-((ang - (ang.max() + ang.min()) / 2.0) ** 2) / (2 * s_ang**2)) / (s_ang * np.sqrt(2 * np.pi))
    Ca, Cl = ot._conv_same_matrix(ot._t(g_ang)).numpy(), ot._conv_same_matrix(ot._t(g_lam)).numpy()
    conv = lambda X: (Cl @ (Ca @ X).T).T
    x = x0.numpy()
    Mv = M0 + np.einsum("i,irc->rc", x, D) + 0.5 * np.einsum("i,j,ijrc->rc", x, x, Q)
    M1 = [D[i] + np.einsum("j,jrc->rc", x, Q[i]) for i in range(3)]
    Bv, B1 = conv(Mv), [conv(m) for m in M1]
    rr = np.arange(npx)
    jM, jB = np.argmax(Mv, axis=1), np.argmax(Bv, axis=1)
    mM, mB = Mv[rr, jM], Bv[rr, jB]
    s = mM / mB
    rho = [M1[i][rr, jM] / mM - B1[i][rr, jB] / mB for i in range(3)]
    Yv = Bv * s[:, None]
    Y1 = [B1[i] * s[:, None] + Bv * (s * rho[i])[:, None] for i in range(3)]
    sg = 1.0 / (1.0 + np.exp(-x[2]))
    dsg = sg * (1 - sg)
    av, ad, add = 0.5 + 2.0 * sg, 2.0 * dsg, 2.0 * dsg * (1 - 2 * sg)
    blocks = lambda Y: Y.reshape(ccd0, ang_step, n_lam, lam_step).mean(axis=(1, 3))[r0:r1]
    lamb = lam_nm.reshape(n_lam, lam_step).mean(axis=1)
    blue = lamb < lam_split
    assert blue.any() and (~blue).any()
    for a in range(3):
        for c in range(a, 3):
            M2, B2 = Q[a, c], conv(Q[a, c])
            rho_ac = M2[rr, jM] / mM - M1[a][rr, jM] * M1[c][rr, jM] / mM**2 - B2[rr, jB] / mB + B1[a][rr, jB] * B1[c][rr, jB] / mB**2
            Y2 = (B2 * s[:, None] + B1[a] * (s * rho[c])[:, None] + B1[c] * (s * rho[a])[:, None]
                  + Bv * (s * (rho[a] * rho[c] + rho_ac))[:, None])
            Dv, Da, Dc, Dac = blocks(Yv), blocks(Y1[a]), blocks(Y1[c]), blocks(Y2)
            R = np.arange(Dv.shape[0])
            js = np.argmax(Dv, axis=1)
            mx, mxa, mxc, mxac = (Z[R, js][:, None] for Z in (Dv, Da, Dc, Dac))
            u = Dv / mx
            ua, uc = (Da - u * mxa) / mx, (Dc - u * mxc) / mx
            uac = (Dac - ua * mxc - uc * mxa - u * mxac) / mx
            amp = np.where(blue, av, a2)[None, :]
            amp_a = np.where(blue, ad if a == 2 else 0.0, 0.0)[None, :]
            amp_c = np.where(blue, ad if c == 2 else 0.0, 0.0)[None, :]
            amp_ac = np.where(blue, add if a == c == 2 else 0.0, 0.0)[None, :]
            got = e_amps * (uac * amp + ua * amp_c + uc * amp_a + u * amp_ac)
            want = second(a, c)
            ratio = np.max(np.abs(got - want)) / np.max(np.abs(want))
            assert ratio <= 1e-11, (a, c, ratio)   # (both sides are the same formula up to the order of a few hundred operations)


def test_sizes_cross_the_cuts():
    """k_ffhess's launch plan has one cut: whether a workgroup walks one angle or several (angle chunks = min(n_angles,
    kFfhessWGPerCU * CUs / pairs)).  The cases sit on both sides of it."""
    api = open(os.path.join(CSRC, "tsff_api.inc")).read()
    assert int(re.search(r"constexpr int kFfhessWGPerCU = (\d+);", api).group(1)) == FFHESS_WG_PER_CU, "move FFHESS_WG_PER_CU"
    assert "const int want = kFfhessWGPerCU * h->ncu2d();" in api
    assert "p.grid = dim3(std::max(A.npair, 1), (unsigned)std::max(1, std::min(h->S.n_angles, want / std::max(A.npair, 1))));" in api
    assert "for (int a = blockIdx.y; a < NA; a += gridDim.y) {" in open(os.path.join(CSRC, "k_ffhess.inc")).read()
    chunks = lambda nf: min(N_ANGLES, FFHESS_WG_PER_CU * CUS // (nf * (nf + 1) // 2))
    amp = ("amp1", "amp2", "amp3")
    nf = {n: sum(k not in amp for k in ION_CASES[n][1]) for n in ION_CASES}
    assert chunks(sum(k not in amp for k in LEAVES)) == 102      # six leaves, ten pairs: two or three angles per workgroup
    assert chunks(nf[2]) == 102 and chunks(nf[3]) == chunks(nf[4]) == N_ANGLES   # 10 pairs again; 3 pairs: one angle each
    assert chunks(4) < N_ANGLES == chunks(2)                     # (the cut lies between two and three leaves at 256 CUs)


def test_sigma_bound_is_reproducible():
    """SIGMA_BOUND is what _sigma_bound gives for the twin's l2 Hessian at MEASURED_ENTRY_ERR."""
    Ht = _twin_small("l2")[2]
    assert np.max(np.abs(Ht - Ht.T)) <= 1e-12 * np.max(np.abs(Ht))
    bound = _sigma_bound(Ht, MEASURED_ENTRY_ERR)
    print(f"sigma bound {bound:.3e} at entry error {MEASURED_ENTRY_ERR:.1e}")
    assert 0.5 * SIGMA_BOUND <= bound <= SIGMA_BOUND, bound


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _loss_fn(method):
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    cfg, sa, batch, _ = ap._setup(False)
    cfg = copy.deepcopy(cfg)
    cfg["optimizer"]["loss_method"] = method
    return LossFunction(cfg, sa, batch), ThomsonParams(cfg["parameters"], 1, batch=False, activate=True), batch


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
def test_hessian_matches_twin(torch_mod, method):
    lf, tp, batch = _loss_fn(method)
    loss_t, grad_t, Ht = _twin_small(method)
    names, Et, Jt = ap._twin_dlm()
    cfg, _, _, lam = ap._setup(False)
    w, d, t = _wcol(cfg, lam), batch["e_data"], Et + batch["noise_e"]
    out = lf.angular_h_loss_wrt_params(tp, batch)
    assert [k for _, k in out["leaves"]] == names == LEAVES
    H = out["H"]
    ratio, ok = _hess_ok(H, Ht)
    gn_t = _gauss_newton(Jt, w, d, t, method)
    A = np.einsum("arc,rc->a", np.abs(Jt), w[None, :] * np.abs(_first_derivative(d, t, method)))   # sum_j w |l'| |t_a|
    gr = np.abs(out["grad"] - grad_t) / A
    lr = abs(out["loss"] - loss_t) / abs(loss_t)
    sig_t = _sigmas(Ht)
    sr = np.abs(out["sigmas"] - sig_t) / np.abs(sig_t)
    record(f"hessian[{method}]", f"max |H - H_twin| / sqrt|H_aa H_cc| {np.max(ratio):.3e} (bound {HESS_TOL:.0e}); grad / sum w|l'||t_a| "
           f"{np.max(gr):.3e}; loss {lr:.3e}; sigmas rel {np.max(sr):.3e}; eig(H_twin) min {np.min(np.linalg.eigvalsh(Ht)):.3e} max "
           f"{np.max(np.linalg.eigvalsh(Ht)):.3e}; sigmas " + " ".join(f"{n} {s:+.4e}" for n, s in zip(names, out["sigmas"])))
    print(method, "H ratio\n", ratio, "\ngrad ratio", gr, "loss", lr, "sigma rel", sr)
    assert ok, ratio
    # the gradient, each leaf within 1e-7 of its own accumulation sum (the bound of test_angular_vg_loss_dlm_matches_twin); under l2
    # also at the bound test_angular_gauss_newton_matches_twin holds it to
    assert np.all(np.abs(out["grad"] - grad_t) <= 1e-7 * A), gr
    if method == "l2":
        assert np.all(np.abs(out["grad"] - grad_t) <= 1e-7 * np.sqrt(np.diag(gn_t)) * np.sqrt(2.0 * loss_t) + 1e-7 * np.abs(grad_t))
    assert lr <= 1e-7
    assert np.array_equal(H, H.T) and np.array_equal(out["gn"], out["gn"].T)
    _, ok_gn = _hess_ok(out["gn"], gn_t) if method != "l1" else (None, not np.any(out["gn"]))
    assert ok_gn
    np.testing.assert_allclose(ap._get_sigmas(out["hess"], 1)[0], out["sigmas"], rtol=1e-12)
    assert out["hess"]["electron"]["Te"]["general"]["lam"].shape == (1, 1)
    if method == "l2":
        assert np.array_equal(np.sign(out["sigmas"]), np.sign(sig_t))
        # the call cannot be returning the Gauss-Newton matrix (the twin: 0.58), and reports what the fit found as the twin does
        assert abs(H[0, 1] - out["gn"][0, 1]) >= 0.1 * np.sqrt(abs(H[0, 0] * H[1, 1]))
        assert np.all(out["sigmas"][:4] < 0.0) and np.all(sig_t[:4] < 0.0)
        assert np.max(sr) <= SIGMA_BOUND, sr
        record("sigma_bound", f"largest entry error of the four methods {MEASURED_ENTRY_ERR:.1e} -> symmetric noise of ten times that on the "
               f"twin's l2 Hessian, 100 draws: largest relative change of a sigma {SIGMA_BOUND:.1e} (the bound); measured here {np.max(sr):.3e}")


@pytest.mark.gpu
def test_second_order_image_rows(torch_mod):
    lf, tp, batch = _loss_fn("l2")
    names, Et, Jt = ap._twin_dlm()
    cfg, _, _, lam = ap._setup(False)
    eng = lf.ts_diag.dlm_engine(True)
    lf.ts_diag._ats_prepare(eng, batch)
    act = [util.slot_of(k) for k in LEAVES]
    out = eng.angular_loss_hess(tp.X[0], act, batch["e_data"], batch["noise_e"], batch["e_amps"], _wcol(cfg, lam), "l2", want_images=True)
    assert "k_ffhess<1>" in eng.last_launch() and "k_ats_rownorm_jvp2" in eng.last_launch() and "k_ats_resunit_jvp2" in eng.last_launch()
    E, E1, E2 = (out[k].cpu().numpy() for k in ("E", "E1", "E2"))
    n = len(LEAVES)
    assert E2.shape == (n * (n + 1) // 2, ap.ROWS, ap.N_LAM)
    assert np.max(np.abs(E - Et)) <= 1e-7 * np.max(np.abs(Et))
    r1 = at.row_ratios(E1, Jt)
    assert np.max(r1) <= at.ROW_TOL, np.max(r1, axis=1)
    worst = {}
    for ka, kc in PAIRS:
        a, c = sorted((LEAVES.index(ka), LEAVES.index(kc)))
        worst[f"{ka},{kc}"] = float(np.max(at.row_ratios(E2[pair_index(a, c, n)], _twin_second(a, c))))
    record("second_order_rows", f"E1 {np.max(r1):.3e}; E2 " + " ".join(f"({k}) {v:.2e}" for k, v in worst.items()) + f" (bound {at.ROW_TOL:.0e})")
    assert max(worst.values()) <= at.ROW_TOL, worst
    assert not np.any(E2[pair_index(LEAVES.index("amp1"), LEAVES.index("amp2"), n)])
    np.testing.assert_allclose(out["phys"].cpu().numpy(), tp.physical_matrix()[0], rtol=1e-14)


def _engine_case(n_ion, keys=None):
    """Engine.angular_loss_hess on a deck of _ion_case at the engine level -> (case, engine, out, fe)"""
    from tsadar_amd.diagnostic import ThomsonScatteringDiagnostic
    from tsadar_amd.engine import Engine

    s = _ion_case(n_ion)
    mode = s["mode"]
    eng = Engine(s["cfg"], s["sa"], activate=True, fe_mode={"dlm": L.FE_DLM, "table": L.FE_PER_LINEOUT, "shared": None}[mode])
    assert eng.fe_mode == {"dlm": L.FE_DLM, "table": L.FE_PER_LINEOUT, "shared": L.FE_SHARED}[mode]
    ThomsonScatteringDiagnostic(s["cfg"], s["sa"])._ats_prepare(eng, dict(e_data=s["e_data"]))
    fe = orc.dlm_fe(s["m"], ap.NVX) if mode == "table" else None
    act = [util.slot_of(k) for k in (keys or s["keys"])]
    out = eng.angular_loss_hess(s["X"], act, s["e_data"], s["noise"], s["e_amps"], _wcol(s["cfg"], s["lam"]), "l2", fe=fe, want_images=True)
    return s, eng, out, fe


def _assert_image_bits(eng, out, fe, e_amps):
    """E is bit for bit tsff_ats_spectrum of tsff_form_factor at the physical parameters the call staged (explicit or shared tables)."""
    phys = out["phys"].cpu().numpy()
    P = eng.form_factor(0, phys[None, :], None if fe is None else fe[None, :])
    E = eng.ats_spectrum(P[0], e_amps, phys[L.P_LAM], phys[L.P_AMP1], phys[L.P_AMP2])
    assert np.array_equal(E.cpu().numpy(), out["E"].cpu().numpy())


@pytest.mark.gpu
def test_pairs_without_form_factor_launch_nothing(torch_mod):
    """Only amp1 and amp2 fitted (the three-species deck, an explicit table): no k_ffhess task, and the Hessian still is the twin's."""
    import torch
    from oracle import tsadar_oracle_torch as ot

    s, eng, out, fe = _engine_case(3, keys=("amp1", "amp2"))
    launched = eng.last_launch()
    assert not any(k.startswith("k_ffhess") for k in launched), launched
    assert "k_ats_resunit_jvp2" in launched and "k_ats_hess_reduce" in launched and "k_ats_rownorm_jvp2" not in launched
    _assert_image_bits(eng, out, fe, s["e_amps"])
    # the twin: the image is e_amps u amp(x) with u the image at unit amplitudes
    sm_x = s["X"]
    pc = s["cfg"]["parameters"]["general"]
    E = out["E"].cpu().numpy()
    phys = out["phys"].cpu().numpy()
    blue = s["lam"] < phys[L.P_LAM]
    U = np.where(blue[None, :], E / phys[L.P_AMP1], E / phys[L.P_AMP2])
    x0 = ot._t(np.array([sm_x[L.P_AMP1], sm_x[L.P_AMP2]]))

    def F(x):
        a1 = torch.sigmoid(x[0]) * (pc["amp1"]["ub"] - pc["amp1"]["lb"]) + pc["amp1"]["lb"]
        a2 = torch.sigmoid(x[1]) * (pc["amp2"]["ub"] - pc["amp2"]["lb"]) + pc["amp2"]["lb"]
        return ot._t(U) * torch.where(torch.as_tensor(blue)[None, :], a1, a2)

    assert pc["amp1"]["active"] and pc["amp2"]["active"]
    loss_t, grad_t, Ht = _twin_of_image(F, x0, _wcol(s["cfg"], s["lam"]), s["e_data"], s["noise"], "l2")
    H = out["hess"].cpu().numpy()
    ratio, ok = _hess_ok(H, Ht)
    record("hessian[amps_only]", f"max ratio {np.max(ratio):.3e} (bound {HESS_TOL:.0e})")
    assert ok, ratio
    assert H[0, 1] == 0.0 and np.array_equal(H, H.T)   # (no sample carries both amplitudes)
    assert abs(float(out["loss"].cpu()) - loss_t) <= 1e-7 * abs(loss_t)
    assert not np.any(out["E2"][1].cpu().numpy())


@pytest.mark.gpu
def test_zero_residual_is_gauss_newton(torch_mod):
    """Data = the device's own image + noise_e at the fitted point: H = gn, and gn is angular_gn_loss_wrt_params' matrix for the leaves
    that call differentiates exactly (all but m, whose first derivative there is a central difference of the table)."""
    from tsadar_amd.loss_function import LossFunction

    lf, tp, batch = _loss_fn("l2")
    E = lf.angular_jacobian(tp, batch)["ThryE"]
    b2 = dict(batch)
    b2["e_data"] = E + batch["noise_e"]
    lf2 = LossFunction(lf.cfg, ap._setup(False)[1], b2)
    out = lf2.angular_h_loss_wrt_params(tp, b2)
    gn = out["gn"]
    sc = np.sqrt(np.outer(np.diag(gn), np.diag(gn)))
    # (the DLM handle's image differs from the explicit-table handle's by the rounding of the table: a residual of ~1e-12 of the image)
    ratio = np.abs(out["H"] - gn) / sc
    ref = lf2.angular_gn_loss_wrt_params(tp, b2)["H"]
    keep = [i for i, k in enumerate(LEAVES) if k != "m"]
    r2 = (np.abs(gn - ref) / sc)[np.ix_(keep, keep)]
    record("zero_residual", f"max |H - gn| / sqrt(gn_aa gn_cc) {np.max(ratio):.3e}; gn vs angular_gn_loss_wrt_params (without m) {np.max(r2):.3e} "
           f"(bound {HESS_TOL:.0e})")
    assert np.all(ratio <= HESS_TOL), ratio
    assert np.all(r2 <= HESS_TOL), r2


@pytest.mark.gpu
@pytest.mark.parametrize("n_ion", [2, 3, 4])
def test_ion_counts_and_ties(torch_mod, n_ion):
    s, eng, out, fe = _engine_case(n_ion)
    assert f"k_ffhess<{n_ion}>" in eng.last_launch()
    loss_t, grad_t, Ht = s["twin"]
    H = out["hess"].cpu().numpy()
    ratio, ok = _hess_ok(H, Ht)
    record(f"hessian[ions{n_ion}]", f"leaves {' '.join(s['keys'])} ({s['mode']}): max ratio {np.max(ratio):.3e} (bound {HESS_TOL:.0e})")
    print(n_ion, s["keys"], "H ratio\n", ratio, "\nH_twin\n", Ht)
    assert ok, ratio
    assert np.array_equal(H, H.T)
    assert abs(float(out["loss"].cpu()) - loss_t) <= 1e-7 * abs(loss_t)
    if s["mode"] != "dlm":
        _assert_image_bits(eng, out, fe, s["e_amps"])


@pytest.mark.gpu
def test_deterministic(torch_mod):
    torch = torch_mod
    from tsadar_amd.engine import Engine

    lf, tp, batch = _loss_fn("l2")
    cfg, sa, _, lam = ap._setup(False)
    act = [util.slot_of(k) for k in LEAVES]
    args = (tp.X[0], act, batch["e_data"], batch["noise_e"], batch["e_amps"], _wcol(cfg, lam), "l2")
    eng = lf.ts_diag.dlm_engine(True)
    lf.ts_diag._ats_prepare(eng, batch)
    a = {k: v.cpu().numpy() for k, v in eng.angular_loss_hess(*args, want_images=True).items()}
    b = {k: v.cpu().numpy() for k, v in eng.angular_loss_hess(*args, want_images=True).items()}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # a second handle on another stream
    eng2 = Engine(lf.cfg, sa, activate=True, fe_mode=L.FE_DLM)
    lf.ts_diag._ats_prepare(eng2, batch)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = eng2.angular_loss_hess(*args, want_images=True)
    st.synchronize()
    for k in a:
        assert np.array_equal(a[k], c[k].cpu().numpy()), k


@pytest.mark.gpu
def test_loss_function_without_m_on_the_explicit_table(torch_mod):
    """LossFunction.angular_h_loss_wrt_params when m is not fitted: the deck's own engine (fe_mode PER_LINEOUT), the table from
    ``weights()``, against the twin's Hessian of that deck."""
    from tsadar_amd import ThomsonParams
    from tsadar_amd.loss_function import LossFunction

    s = _ion_case("no_m")
    cfg = copy.deepcopy(s["cfg"])
    batch = dict(e_data=s["e_data"], i_data=np.zeros((ap.ROWS, ap.N_LAM)), e_amps=s["e_amps"], i_amps=np.zeros(ap.ROWS), noise_e=s["noise"],
                 noise_i=np.array([0.0]))
    lf = LossFunction(cfg, s["sa"], batch)
    tp = ThomsonParams(cfg["parameters"], 1, batch=False, activate=True)
    out = lf.angular_h_loss_wrt_params(tp, batch)
    assert [k for _, k in out["leaves"]] == s["keys"]
    assert list(lf.ts_diag._engines) == [True] and lf.ts_diag.engine(True).fe_mode == L.FE_PER_LINEOUT
    loss_t, grad_t, Ht = s["twin"]
    ratio, ok = _hess_ok(out["H"], Ht)
    record("hessian[no_m_table]", f"max ratio {np.max(ratio):.3e} (bound {HESS_TOL:.0e})")
    assert ok, ratio
    assert abs(out["loss"] - loss_t) <= 1e-7 * abs(loss_t)
    np.testing.assert_allclose(ap._get_sigmas(out["hess"], 1)[0], out["sigmas"], rtol=1e-12)


def _raw_call(eng, x, act, n, d, nz, ea, wc, method, fe=None, skip=None):
    """tsff_angular_loss_hess as the binding sends it -> (return code, tsff_last_error, last_launch)"""
    import ctypes as C

    torch = eng.torch
    new = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=eng.device)
    k = max(n, 1)
    outs = dict(loss=new(1), grad=new(k), hess=new(k, k), gn=new(k, k))
    p = lambda name, t: C.c_void_p(None) if skip == name else eng._ptr(t)
    a = np.ascontiguousarray(act, dtype=np.int32)
    eng._sync_stream()
    rc = eng.lib.tsff_angular_loss_hess(eng.h, p("leaves", x), p("fe", fe), a.ctypes.data_as(C.POINTER(C.c_int32)), n, p("e_data", d), p("noise", nz),
                                        p("e_amps", ea), p("wcol", wc), method, p("loss", outs["loss"]), p("grad", outs["grad"]),
                                        p("hess", outs["hess"]), p("gn", outs["gn"]), None, None, None, None)
    msg = eng.lib.tsff_last_error(eng.h)
    return rc, (msg.decode() if msg else ""), eng.last_launch()


@pytest.mark.gpu
def test_c_abi_refusals(torch_mod):
    """Every refusal of tsff_angular_loss_hess returns its code with a tsff_last_error message and enqueues nothing."""
    from tsadar_amd.diagnostic import ThomsonScatteringDiagnostic
    from tsadar_amd.engine import Engine

    cfg, sa, batch, lam = ap._setup(False)
    cfg = copy.deepcopy(cfg)
    eng = Engine(cfg, sa, activate=True, fe_mode=L.FE_PER_LINEOUT)
    _, tp, _ = ap._loss_fn(False)
    x, d, nz = eng.dev(tp.X[0]), eng.dev(batch["e_data"]), eng.dev(batch["noise_e"])
    ea, wc = eng.dev(batch["e_amps"].reshape(-1)), eng.dev(_wcol(cfg, lam))
    fe = eng.dev(orc.dlm_fe(2.5, ap.NVX))
    Te, lamS = L.P_TE, L.P_LAM

    def refused(code, text, *args, **kw):
        rc, msg, launched = _raw_call(eng, *args, **kw)
        assert rc == code and text in msg and launched == [], (rc, msg, launched)

    refused(-2, "tsff_ats_setup", x, [Te, lamS], 2, d, nz, ea, wc, 0, fe=fe)
    ThomsonScatteringDiagnostic(cfg, sa)._ats_prepare(eng, batch)
    for name in ("leaves", "e_data", "e_amps", "wcol", "loss", "grad", "hess", "gn"):
        refused(-1, "bad argument", x, [Te, lamS], 2, d, nz, ea, wc, 0, fe=fe, skip=name)
    refused(-1, "n_active", x, [Te], 0, d, nz, ea, wc, 0, fe=fe)
    refused(-1, "loss_method", x, [Te], 1, d, nz, ea, wc, 4, fe=fe)
    refused(-1, "out of range", x, [Te, eng.NP], 2, d, nz, ea, wc, 0, fe=fe)
    refused(-1, "repeated", x, [Te, Te], 2, d, nz, ea, wc, 0, fe=fe)
    refused(-2, "TSFF_FE_DLM", x, [Te, L.P_M], 2, d, nz, ea, wc, 0, fe=fe)
    refused(-3, "A is not", x, [Te, L.P_ION0 + L.ION_A], 2, d, nz, ea, wc, 0, fe=fe)
    refused(-2, "needs fe", x, [Te, lamS], 2, d, nz, ea, wc, 0, fe=None)   # (what a handle of a 2-D f_e deck meets as well)
    # the call still runs after all that (noise_e may be NULL)
    rc, msg, launched = _raw_call(eng, x, [Te, lamS], 2, d, nz, ea, wc, 0, fe=fe, skip="noise")
    assert rc == 0 and "k_ffhess<1>" in launched, (rc, msg)
    eng.torch.cuda.synchronize()
    # the LDS budget: with the DLM order a leaf, 8200 + 12 nvx + 242 + 4 (29 + 25) doubles against 20480 -> nvx >= 986 at 241 angles
    for nvx, code in ((985, 0), (986, -2)):
        c2 = decks.deck_angular(1, nvx, ap.CCD, ap.START, ap.END)
        e2 = Engine(c2, sa, activate=True, fe_mode=L.FE_DLM)
        ThomsonScatteringDiagnostic(c2, sa)._ats_prepare(e2, batch)
        rc, msg, launched = _raw_call(e2, e2.dev(tp.X[0]), [Te, L.P_M], 2, e2.dev(batch["e_data"]), None, e2.dev(batch["e_amps"].reshape(-1)),
                                      e2.dev(_wcol(cfg, lam)), 0)
        e2.torch.cuda.synchronize()
        assert rc == code, (nvx, rc, msg)
        if code:
            assert "LDS budget exceeded" in msg and launched == []
        else:
            assert "k_ffhess<1>" in launched and "k_hess_mtab<1>" in launched
