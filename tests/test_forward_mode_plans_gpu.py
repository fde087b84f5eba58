"""The forward-mode kernels (k_jac_sweep, k_lm_step, k_ffjvp with k_fe_direction, k_hess_pairs with the DLM order as a leaf) past
their grid caps and the switches of their host plans, every lineout against the twin result of its member.

tests/test_jacobian.py, test_lm_device.py, test_form_factor_jvp.py and test_hessian_exact.py pin every shipped instantiation to the
torch twin at B = 2 .. 5 and at most 7 directions, where every persistent loop runs its body once and every plan takes its first
branch.  Each size below is the smallest that crosses one cut; when a constant changes, test_sizes_cross_the_cuts fails and names
the number to move:

  B = 1027  k_jac_sweep      jac_prepare launches min(B, kJacMaxWG = 1024) workgroups, the kernel walks b = blockIdx.x, + gridDim.x ..:
                             kJacMaxWG + 3 gives workgroups 0, 1, 2 a second lineout (and no other workgroup one).  One lineout past the
                             cap would do for the loop; three make the second lineouts 1024, 1025, 1026 the members 1, 2, 0 of K = 3
                             (1024 mod 3 = 1) and 4, 0, 1 of K = 5 (1024 mod 5 = 4) -- a workgroup's second lineout is never the member
                             of its first, so tables, scratch (A.xg, A.rows: per workgroup) or LDS scalars left from the first pass show
                             -- and give the LM case a workgroup that skips its first lineout and computes its second (0), one that
                             does the reverse (1) and one that computes both (2)
  B = 65, n_dir = 7          tsff_form_factor_jvp builds the table tangents for dblk directions at a time, dblk = min(max(gw, (384 / B) /
                             gw * gw), ceil(n_dir / gw) * gw): 65 is the smallest B with dblk = 3 = gw (B = 64: 6), so 7 directions
                             run as blocks of 3, 3 and 1 -- d0 = 3 and d0 = 6 re-run k_fe_direction and k_wgemm<2> into the same jv_*
                             buffers, offset fe_dot by d0 * B * nvx and end in a block of ONE direction (65 rows: a second GEMM row
                             tile of one row)
  nvx = 652, B = 2, n_dir = 2  three table lanes of k_ffjvp need 9840 + 16 nvx + n_angles + 4 (kNP_MAX + 1 + 25) doubles of LDS, one
                             lane 6560 + 8 nvx + ..: with 10 angles 652 is the smallest grid at which three lanes exceed the 160 KB
                             (651: 163 824 B, 652: 163 952 B against 163 840) and the plan falls back to gw = 1; any grid of 4 .. 4096
                             points is accepted by tsff_create, and at 652 every other kernel of the call fits (one lane of k_ffjvp
                             95 984 B, k_fe_direction 105 856 B; k_form_factor and k_form_factor_adj with the table adjoints ran):
                             the branch is alive
  B = 99, 6 leaves           k_hess_pairs runs min(B npair, kHessMaxWG = 1024) workgroups over the (lineout, pair) tasks, npair = 21:
                             99 is the smallest multiple of K = 3 with B npair >= 2 kHessMaxWG, every workgroup has at least two tasks,
                             and with the DLM order a leaf (fe_mode DLM: slot = b) a workgroup's second task reloads W, Wm, Wmm and
                             the three sets of Hermite coefficients of another lineout

The batches are TILED: lineout b is member b mod K of the K lineouts an existing case already pins to the twin (parameters, data,
amplitudes, noise, f_e and the directions alike), so the reference costs what the small case costs and EVERY lineout of the large
call is compared, at the bound the small case uses (test_jacobian.ROW_TOL, GN_TOL, angular_twin.ROW_TOL, test_hessian_exact.HESS_TOL,
SIGMA_RTOL; the LM loop bit for bit against lm.step and against a plain B = 5 run).  On top of that all repeats of a member within
one call are equal bit for bit: no kernel here adds across lineouts, every lineout is computed by one workgroup in a fixed order.
test_tiled_members_are_distinct (CPU) makes sure a row served from the wrong lineout or from the previous pass cannot pass: the
twin's rows of any two members differ by more than 100 times the bound.

Measured on an MI355X (profiles/forward_mode_plans_pytest.txt), the largest ratio over all lineouts against the bound of 1e-7: the
Jacobian 2.3e-9 (ions1, fe_const), 5.1e-9 (m), 2.6e-11 (ions2_one); Gauss-Newton 5.5e-10 (l2), 5.2e-9 (poisson), 3.2e-8 (m, its gradient);
P_dot 1.3e-9 in the direction blocks and 9.1e-11 on one table lane; the Hessian 1.2e-9.  The second-pass lineouts show the figures of
their members, all repeats were equal bit for bit, the LM record replays through lm.step bitwise: every path was correct as found.
That the cases can fail was tried once on a library built with three errors of this kind -- k_jac_sweep and k_hess_pairs loading
their tables on the first pass only, k_fe_direction reading fe_dot without d0 * B * nvx: exactly fe_const, m, m-l2, the direction
blocks and the Hessian failed (ratios 1.2 .. 1e4, at lineouts 1024, 1025 and 50), the cases on a shared table passed.
"""
import functools
import os
import re

import numpy as np
import pytest

import angular_twin as at
import test_form_factor_jvp as tff
import test_hessian_exact as the
import test_jacobian as tja
import test_lm_device as tlm
import util
from tsadar_amd import _lib as L
from tsadar_amd import lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tsadar_amd", "csrc")
RECORD = os.path.join(ROOT, "profiles", "forward_mode_plans_pytest.txt")

# the plans' constants (test_sizes_cross_the_cuts reads them back from the sources)
JAC_MAX_WG = 1024        # kJacMaxWG
HESS_MAX_WG = 1024       # kHessMaxWG
FFJVP_W = 3              # kFfjvpW: directions per group of k_ffjvp
DIR_ROWS = 384           # table rows (directions x lineouts) of one direction block
LDS_LIMIT = 160 * 1024   # kLdsLimit
N_ANGLES = 10            # util.sa_fit
NVX_RANGE = (4, 4096)    # what tsff_create accepts

B_JAC = JAC_MAX_WG + 3
JAC_CASES = ("ions1", "fe_const", "m", "ions2_one")
JAC_KERNEL = {"ions1": "k_jac_sweep<1, 3, true>", "m": "k_jac_sweep<1, 3, false>", "ions2_one": "k_jac_sweep<2, 1, false>"}
GN_CASES = {"ions1-l2": ("ions1", "l2"), "m-l2": ("m", "l2"), "ions1-poisson": ("ions1", "poisson")}
FF_CASE, FF_B, FF_NDIR, FF_SOME = "ni1_all", 65, 7, (0, 4, 6)
LANE_NVX, LANE_B, LANE_NDIR = 652, 2, 2
HESS_K, HESS_B, HESS_SEED = 3, 99, 111


def members(B, K):
    """lineout b of a tiled batch is member b mod K"""
    return np.arange(B) % K


def tiled(a, idx, axis=0):
    return np.ascontiguousarray(np.take(np.asarray(a), idx, axis=axis))


def tiled_batch(batch, idx):
    return {k: tiled(v, idx) for k, v in batch.items()}


def repeats_equal(a, idx, axis=0):
    """every lineout of ``a`` equals, bit for bit, the first lineout of its member (lineouts 0 .. K - 1 are the members themselves)"""
    K = int(idx.max()) + 1
    first = np.take(a, np.arange(K), axis=axis)
    return bool(np.array_equal(a, np.take(first, idx, axis=axis), equal_nan=True))


def ffjvp_smem_doubles(nvx, nlane, n_angles=N_ANGLES, W=FFJVP_W):
    """k_ffjvp.inc's ffjvp_smem_doubles"""
    n = 2 * L.NXI2 + L.NXI2 + 4 * nvx
    n += nlane * (L.NXI2 + 4 * nvx)
    n += n_angles + (1 + W) * ((L.n_params(4) + 1) + (9 + 4 * 4))
    return n


def direction_block(B, n_dir, gw):
    """form_factor_jvp_prepare's dblk"""
    want = max(1, DIR_ROWS // max(B, 1))
    return min(max(gw, want // gw * gw), -(-n_dir // gw) * gw)


def table_lanes(nvx):
    """form_factor_jvp_prepare's gw with fe_dot (None: refused)"""
    if 8 * ffjvp_smem_doubles(nvx, FFJVP_W) <= LDS_LIMIT:
        return FFJVP_W
    return 1 if 8 * ffjvp_smem_doubles(nvx, 1) <= LDS_LIMIT else None


# ---------------------------------------------------------------------------------------------------------------------
# CPU side: the members and their twin results, computed once
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gn_members(case):
    """per member of a Gauss-Newton case: (S [K, 3], grad [K, n], gn [K, n, n]) from the twin's J and spectra"""
    cid, method = GN_CASES[case]
    s = tja._with_method(tja._inputs(cid), method)
    w = tja._weights(s["cfg"])
    tw = tja._twin(cid)
    out = [tja._gn_reference(s["cfg"], {k: np.asarray(v)[b:b + 1] for k, v in s["batch"].items()}, w, *(t[b:b + 1] for t in tw))
           for b in range(tja.B)]
    return np.array([o[0] for o in out]), np.array([o[1][0] for o in out]), np.array([o[2][0] for o in out])


@functools.lru_cache(maxsize=None)
def ff_some():
    """the ni1_all members with fe_dot on the directions FF_SOME only (zero on the others), and their twin"""
    s = dict(tff._inputs(FF_CASE))
    fd = np.zeros_like(s["fd"])
    fd[list(FF_SOME)] = s["fd"][list(FF_SOME)]
    s["fd"] = fd
    return s, tff._twin_of(s)


@functools.lru_cache(maxsize=None)
def lane_case():
    s = tff._build(1, LANE_NVX, (), LANE_NDIR, "all", nb=LANE_B)
    return s, tff._twin_of(s)


@functools.lru_cache(maxsize=None)
def hess_members():
    """K lineouts of the PROD leaves (the DLM order among them, each lineout its own order) and their twin Hessians"""
    cfg = the._fit(nvx=128, active=the.PROD)()
    sa = util.sa_fit(HESS_K)
    batch = util.synthetic_batch(cfg, sa, HESS_K, seed=HESS_SEED)
    normed = util.random_lineouts(cfg, HESS_K, seed=HESS_SEED + 50, ranges=dict(m=(2.1, 4.2)))
    _, names, act = the._leaves(cfg)
    H = []
    for b in range(HESS_K):
        nb = {k: np.asarray(v)[b:b + 1] for k, v in normed.items()}
        bb = {k: np.asarray(v)[b:b + 1] for k, v in batch.items()}
        H.append(the._twin_hessian(cfg, util.sa_fit(1), nb, bb, names))
    return dict(cfg=cfg, sa=sa, batch=batch, normed=normed, names=names, act=act, X=util.normed_to_matrix(normed, 1), H=np.array(H))


def test_sizes_cross_the_cuts():
    """(no GPU needed; the GPU cases below are only as good as this cover)"""
    api = open(os.path.join(CSRC, "tsff_api.inc")).read()
    jac = open(os.path.join(CSRC, "k_jacobian.inc")).read()
    hes = open(os.path.join(CSRC, "k_hessian.inc")).read()
    ffj = open(os.path.join(CSRC, "k_ffjvp.inc")).read()
    header = open(os.path.join(ROOT, "include", "tsff.h")).read()
    # the constants above are the plans'
    assert int(re.search(r"constexpr int kJacMaxWG = (\d+);", api).group(1)) == JAC_MAX_WG, "move JAC_MAX_WG (B_JAC follows)"
    assert int(re.search(r"constexpr int kHessMaxWG = (\d+);", api).group(1)) == HESS_MAX_WG, "move HESS_MAX_WG and HESS_B"
    assert int(re.search(r"constexpr int kFfjvpW = (\d+);", api).group(1)) == FFJVP_W, "move FFJVP_W, FF_B and LANE_NVX"
    m = re.search(r"constexpr size_t kLdsLimit = (\d+) \* (\d+);", api)
    assert int(m.group(1)) * int(m.group(2)) == LDS_LIMIT, "move LDS_LIMIT and LANE_NVX"
    assert int(re.search(r"const int want = std::max\(1, (\d+) / std::max\(B, 1\)\);", api).group(1)) == DIR_ROWS, "move DIR_ROWS and FF_B"
    assert "p.dblk = std::min(std::max(p.gw, want / p.gw * p.gw), (n_dir + p.gw - 1) / p.gw * p.gw);" in api, "direction_block"
    assert "c.nwg = std::min(c.b.B, kJacMaxWG);" in api and "const int nwg = std::min(A.tasks, kHessMaxWG);" in api
    assert "for (int b = blockIdx.x; b < K.B; b += gridDim.x) {" in jac
    assert "for (int task = blockIdx.x; task < A.tasks; task += gridDim.x) {" in hes and "const int b = task / A.npair" in hes
    m = re.search(r"c->nvx < (\d+) \|\| c->nvx > (\d+)", api)
    assert (int(m.group(1)), int(m.group(2))) == NVX_RANGE, "move NVX_RANGE"
    # ffjvp_smem_doubles, term by term
    for term in ("size_t n = 2 * (size_t)kNXi2 + kNXi2 + 4 * (size_t)S.nvx;", "n += (size_t)nlane * ((size_t)kNXi2 + 4 * (size_t)S.nvx);",
                 "n += (size_t)S.n_angles + (size_t)(1 + W) * ((kNP_MAX + 1) + (9 + 4 * TSFF_MAX_ION));"):
        assert term in ffj, f"ffjvp_smem_doubles changed ({term}): restate it above and move LANE_NVX"
    assert int(re.search(r"#define TSFF_MAX_ION (\d+)", header).group(1)) == 4 and "constexpr int kNP_MAX = TSFF_NP(TSFF_MAX_ION);" in \
        open(os.path.join(CSRC, "tsff_device.h")).read()
    assert "p.smem = sizeof(double) * ffjvp_smem_doubles(h->S, tab ? kFfjvpW : 0, kFfjvpW);" in api
    assert "p.smem = sizeof(double) * ffjvp_smem_doubles(h->S, 1, kFfjvpW);" in api
    assert util.sa_fit(1)["sa"].size == N_ANGLES

    # 1-3: the persistent loop of k_jac_sweep -- workgroups 0, 1, 2 and no other get a second lineout, of another member
    nwg = min(B_JAC, JAC_MAX_WG)
    second = [w for w in range(nwg) if w + nwg < B_JAC]
    assert B_JAC == JAC_MAX_WG + 3 and second == [0, 1, 2] and B_JAC <= 2 * nwg, "move B_JAC"
    for K in (tja.B, tlm.B):
        idx = members(B_JAC, K)
        assert all(idx[w] != idx[w + nwg] for w in second), (K, "a workgroup's two lineouts are the same member: move B_JAC")
    assert tja.B == 3 and tlm.B == 5 and set(JAC_CASES) <= set(tja.CASES) and all(c in tja.CASES for c, _ in GN_CASES.values())
    # 4: the direction blocks -- 65 is the smallest B with blocks of three directions; 7 directions: 3, 3 and 1
    assert tff.CASES[FF_CASE][3] == FF_NDIR and tff.CASES[FF_CASE][4] == "all" and tff.B == 3
    assert table_lanes(tff.CASES[FF_CASE][1]) == FFJVP_W
    dblk = direction_block(FF_B, FF_NDIR, FFJVP_W)
    assert dblk == FFJVP_W and direction_block(FF_B - 1, FF_NDIR, FFJVP_W) > FFJVP_W, "move FF_B"
    assert FF_B == min(B for B in range(1, DIR_ROWS + 1) if direction_block(B, FF_NDIR, FFJVP_W) == FFJVP_W)
    assert [min(dblk, FF_NDIR - d0) for d0 in range(0, FF_NDIR, dblk)] == [3, 3, 1]
    assert all(direction_block(tff.B, c[3], FFJVP_W) >= c[3] for c in tff.CASES.values())   # (what the other tests run: one block)
    assert {d // dblk for d in FF_SOME} == {0, 1, 2} and len(FF_SOME) < FF_NDIR             # fe_dot in every block, not on every direction
    # 5: the one-lane fallback -- the smallest grid at which three lanes exceed the limit, and one lane fits there
    assert LANE_NVX == min(n for n in range(NVX_RANGE[0], NVX_RANGE[1] + 1) if table_lanes(n) != FFJVP_W), "move LANE_NVX"
    assert table_lanes(LANE_NVX) == 1 and table_lanes(LANE_NVX - 1) == FFJVP_W
    assert max(c[1] for c in tff.CASES.values()) < LANE_NVX                                   # (what the other tests run: three lanes)
    assert direction_block(LANE_B, LANE_NDIR, 1) == LANE_NDIR                                 # one block, LANE_NDIR groups of one lane
    # 6: k_hess_pairs -- every workgroup at least two tasks, B the smallest multiple of K with that
    n = len(the.PROD)
    npair = n * (n + 1) // 2
    assert "m" in the.PROD and npair == 21
    assert HESS_B % HESS_K == 0 and HESS_B * npair >= 2 * HESS_MAX_WG > (HESS_B - HESS_K) * npair, "move HESS_B"
    nwg = min(HESS_B * npair, HESS_MAX_WG)
    idx = members(HESS_B, HESS_K)
    assert all(w + nwg < HESS_B * npair for w in range(nwg))
    assert any(idx[w // npair] != idx[(w + nwg) // npair] for w in range(nwg))   # (and every second task is another lineout: slot = b)
    assert all(w // npair != (w + nwg) // npair for w in range(nwg))


def _pairs(K):
    return [(i, j) for i in range(K) for j in range(K) if i != j]


def _row_gap(a, b):
    """least over the rows (last axis) that are not identically zero in ``a`` of max |a - b| / max |a|"""
    a, b = np.asarray(a).reshape(-1, a.shape[-1]), np.asarray(b).reshape(-1, b.shape[-1])
    scale = np.max(np.abs(a), axis=-1)
    keep = scale > 0.0
    return float(np.min(np.max(np.abs(a - b), axis=-1)[keep] / scale[keep]))


def test_tiled_members_are_distinct():
    """A row served from the wrong lineout, or from the previous pass, must fail (no GPU needed): the twin's rows (J, grad, gn, H,
    P_dot) of any two members differ by more than 100 times the bound applied to them; the LM members (compared bit for bit) differ
    in their data."""
    for cid in JAC_CASES:
        JE, JI = tja._twin(cid)[:2]
        gap = min(min(_row_gap(JE[i], JE[j]), _row_gap(JI[i], JI[j])) for i, j in _pairs(tja.B))
        print(f"jacobian {cid}: least row difference between members {gap:.2e}")
        assert gap > 100 * tja.ROW_TOL, (cid, gap)
    for case in GN_CASES:
        S, g, gn = gn_members(case)
        for i, j in _pairs(tja.B):
            dg, dh = np.max(np.abs(g[i] - g[j])) / np.max(np.abs(g[i])), np.max(np.abs(gn[i] - gn[j])) / np.max(np.abs(gn[i]))
            assert dg > 100 * tja.GN_TOL and dh > 100 * tja.GN_TOL, (case, i, j, dg, dh)
    s = tlm._case("D1")
    for i, j in _pairs(tlm.B):
        assert not np.array_equal(s["batch"]["e_data"][i], s["batch"]["e_data"][j]) and not np.array_equal(s["batch"]["i_data"][i], s["batch"]["i_data"][j])
    for what, (inp, (P, Pd)) in (("all", (tff._inputs(FF_CASE), tff._twin(FF_CASE))), ("some", ff_some()), ("one lane", lane_case())):
        nb = inp["X"].shape[0]
        rows = Pd.reshape(Pd.shape[0], nb, -1)
        gap = min(_row_gap(rows[:, i], rows[:, j]) for i, j in _pairs(nb))
        print(f"form_factor_jvp {what}: least row difference between members {gap:.2e}")
        assert gap > 100 * at.ROW_TOL, (what, gap)
        for i, j in _pairs(nb):
            assert np.max(np.abs(P[i] - P[j]) / np.abs(P[i])) > 100 * 1e-7, what
    sm, tw = ff_some()
    full = tff._twin(FF_CASE)[1]
    for d in range(FF_NDIR):   # (a direction that lost or gained its fe_dot shows: the two calls differ where they should)
        rows = (tw[1][d].reshape(tff.B, -1), full[d].reshape(tff.B, -1))
        assert (_row_gap(*rows) > 100 * at.ROW_TOL) == (d not in FF_SOME), d
    H = hess_members()["H"]
    for i, j in _pairs(HESS_K):
        dh = np.max(np.abs(H[i] - H[j])) / np.max(np.abs(H[i]))
        assert dh > 100 * the.HESS_TOL, (i, j, dh)
        a, b = the._sigmas(H[i]), the._sigmas(H[j])
        assert np.max(np.abs(a - b) / np.abs(a)) > 100 * the.SIGMA_RTOL, (i, j)
    m = hess_members()["normed"]["m"]
    assert min(abs(m[i] - m[j]) for i, j in _pairs(HESS_K)) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _record(key, text):
    """One line per test in profiles/forward_mode_plans_pytest.txt: the test's previous line is replaced."""
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    lines = {}
    if os.path.exists(RECORD):
        lines = {l.split(" ", 1)[0]: l.rstrip("\n") for l in open(RECORD) if l.strip()}
    lines[key] = f"{key} {text}"
    with open(RECORD, "w") as f:
        f.write("".join(v + "\n" for _, v in sorted(lines.items())))


def _sweeps(eng):
    return [k for k in eng.last_launch() if k.startswith("k_jac_sweep<")]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", JAC_CASES)
def test_jacobian_second_pass(cid):
    """Engine.spectrum_jacobian at B = kJacMaxWG + 3: ions1 FE_SHARED on the row form (nothing reloaded, the xg scratch reused),
    fe_const PER_LINEOUT (W and hc reloaded), m FE_DLM with the order a leaf (W, hc, Wm, hcm reloaded), ions2_one one tangent."""
    _torch()
    s = tja._inputs(cid)
    idx = members(B_JAC, tja.B)
    eng = tja._engine(s)
    ea, ia = s["batch"]["e_amps"], s["batch"]["i_amps"]
    eng.spectrum_jacobian(s["X"], ea, ia, s["act"], fe=s["fe"])
    small = _sweeps(eng)
    JE, JI = eng.spectrum_jacobian(tiled(s["X"], idx), tiled(ea, idx), tiled(ia, idx), s["act"], fe=None if s["fe"] is None else tiled(s["fe"], idx))
    tja._sync()
    mine = _sweeps(eng)
    assert len(mine) == 1 and mine == small and mine[0] in tja.JAC_KERNELS, (eng.last_launch(), small)
    if cid in JAC_KERNEL:
        assert mine[0] == JAC_KERNEL[cid], mine
    else:   # the per-lineout constant tables: three tangents, the form the planner picks (recorded)
        assert mine[0] in ("k_jac_sweep<1, 3, true>", "k_jac_sweep<1, 3, false>"), mine
    assert (eng.fe_mode == L.FE_SHARED) == (cid in ("ions1", "ions2_one")) and (eng.fe_mode == L.FE_DLM) == (cid == "m")
    JE, JI = JE.cpu().numpy(), JI.cpu().numpy()
    tJE, tJI = tja._twin(cid)[:2]
    rE, rI = tja._row_ratios(JE, tJE[idx]), tja._row_ratios(JI, tJI[idx])
    worst = max(rE.max(), rI.max())
    same = repeats_equal(JE, idx) and repeats_equal(JI, idx)
    at_b = int(np.argmax(np.maximum(rE.max(axis=1), rI.max(axis=1))))
    print(f"{cid}: B = {B_JAC}: largest row ratio {worst:.3e} (ele {rE.max():.3e}, ion {rI.max():.3e}; lineout {at_b}), second pass "
          f"{max(rE[JAC_MAX_WG:].max(), rI[JAC_MAX_WG:].max()):.3e}, {mine[0]}, repeats bit-equal: {same}")
    _record(f"test_jacobian_second_pass[{cid}]", f"{mine[0].replace(' ', '')} B={B_JAC} max_row_ratio={worst:.3e} ele={rE.max():.3e} "
            f"ion={rI.max():.3e} repeats_bit_equal={same}")
    assert worst <= tja.ROW_TOL, (cid, s["names"], at_b, rE[at_b], rI[at_b])
    assert same, "repeats of a member differ within one call"


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(GN_CASES))
def test_gauss_newton_second_pass(case):
    """Engine.loss_gauss_newton at B = kJacMaxWG + 3: the per-workgroup A.rows scratch across passes; poisson, whose l'' depends on
    the spectrum."""
    _torch()
    cid, method = GN_CASES[case]
    s = tja._with_method(tja._inputs(cid), method)
    idx = members(B_JAC, tja.B)
    eng = tja._engine(s)
    w = tja._weights(s["cfg"])
    terms, grad, gn = [t.cpu().numpy() for t in eng.loss_gauss_newton(tiled(s["X"], idx), tiled_batch(s["batch"], idx), w, s["act"])]
    mine = _sweeps(eng)
    assert mine == [JAC_KERNEL[cid]] and "k_loss_reduce" in eng.last_launch(), eng.last_launch()
    S, g_ref, gn_ref = gn_members(case)
    S_all = (S * np.bincount(idx, minlength=tja.B)[:, None]).sum(axis=0)
    eg = np.max(np.abs(grad - g_ref[idx]), axis=1) / np.max(np.abs(g_ref[idx]), axis=1)
    eh = np.max(np.abs(gn - gn_ref[idx]), axis=(1, 2)) / np.max(np.abs(gn_ref[idx]), axis=(1, 2))
    es = np.max(np.abs(terms - S_all)) / np.max(np.abs(S_all))
    same = repeats_equal(grad, idx) and repeats_equal(gn, idx)
    print(f"{case}: B = {B_JAC}: grad within {eg.max():.3e}, gn within {eh.max():.3e} of the lineout's largest entry, loss sums within "
          f"{es:.3e}; second pass grad {eg[JAC_MAX_WG:].max():.3e}, gn {eh[JAC_MAX_WG:].max():.3e}; repeats bit-equal: {same}")
    _record(f"test_gauss_newton_second_pass[{case}]", f"{mine[0].replace(' ', '')} B={B_JAC} max_ratio={max(eg.max(), eh.max(), es):.3e} "
            f"grad={eg.max():.3e} gn={eh.max():.3e} loss_terms={es:.3e} repeats_bit_equal={same}")
    assert np.array_equal(gn, np.transpose(gn, (0, 2, 1)))
    assert np.all(eg <= tja.GN_TOL) and np.all(eh <= tja.GN_TOL), (int(np.argmax(eg)), eg.max(), int(np.argmax(eh)), eh.max())
    assert es <= tja.GN_TOL, (terms, S_all)
    assert same, "repeats of a member differ within one call"


@pytest.mark.gpu
def test_lm_second_pass_with_terminal_lineouts():
    """tsff_lm_fit on D1 tiled to B = kJacMaxWG + 3 with NaN data in lineouts 0 and 1025: from the second evaluation on workgroup 0
    skips its first lineout and computes its second, workgroup 1 the reverse, workgroup 2 computes both."""
    _torch()
    s = tlm._case("D1")
    K, n = tlm.B, s["n"]
    idx = members(B_JAC, K)
    eng, w = tlm._engine(s)
    plain = tlm._fit(eng, s, w, tlm.N_EVALS)
    big = dict(s, X0=tiled(s["X0"], idx), batch=tiled_batch(s["batch"], idx))
    bad = (0, JAC_MAX_WG + 1)
    for b in bad:
        blue = np.flatnonzero(s["masks"][1][idx[b]])
        big["batch"]["e_data"][b, blue[len(blue) // 2]] = np.nan
    r = tlm._fit(eng, big, w, tlm.N_EVALS)
    sweep = _sweeps(eng)
    assert len(sweep) == tlm.N_EVALS and set(sweep) == {"k_jac_sweep<1, 3, true>"}, sweep
    assert eng.last_launch().count("k_lm_step") == tlm.N_EVALS and eng.last_launch()[-1] == "k_lm_step"
    st = lm.unpack(r["state"], B_JAC, n)
    for b in bad:
        assert st.status[b] == lm.BAD_START and st.nfev[b] == 1 and st.nit[b] == 0 and np.isnan(st.f[b]), (b, st.status[b], st.nfev[b])
        assert np.array_equal(r["X"][b], big["X0"][b])
        assert np.all(np.isnan(r["xh"][1:, b])) and not np.any(np.isnan(r["xh"][0, b]))
    # the whole record through lm.step, bit for bit
    host, fs, nxt, won, lost = tlm._replay(r, n)
    tlm._assert_state(r, host, nxt, big)
    # every other lineout: its member in the plain B = 5 run, bit for bit
    good = np.setdiff1d(np.arange(B_JAC), bad)
    ref = lm.unpack(plain["state"], K, n)
    same = True
    for k in lm.State.FIELDS:
        a, c = getattr(st, k)[good], getattr(ref, k)[idx[good]]
        ok = np.array_equal(a, c, equal_nan=a.dtype.kind == "f")
        same = same and ok
        assert ok, (k, good[np.flatnonzero(np.any((a != c).reshape(len(good), -1), axis=1))[:8]])
    for k in ("xh", "eh", "X"):
        a, c = np.take(r[k], good, axis=r[k].ndim - 2), np.take(plain[k], idx[good], axis=r[k].ndim - 2)
        ok = np.array_equal(a, c, equal_nan=True)
        same = same and ok
        assert ok, k
    print(f"lm: B = {B_JAC}: status counts {np.bincount(st.status, minlength=7)}, accepted {won}, rejected {lost}, second-pass lineouts "
          f"status {st.status[JAC_MAX_WG:]}, nfev {st.nfev[JAC_MAX_WG:]}")
    _record("test_lm_second_pass_with_terminal_lineouts", f"{sweep[0].replace(' ', '')}+k_lm_step B={B_JAC} evals={tlm.N_EVALS} "
            f"max_row_ratio=0 (bitwise against lm.step and the B={K} run) repeats_bit_equal={same}")
    assert won >= 1 and np.all(st.nfev[good] > 1)


def _jvp_ratios(Pd, Pdt, idx):
    n_dir, nb = Pd.shape[0], Pd.shape[1]
    return at.row_ratios(Pd.reshape(n_dir, nb, -1), np.take(Pdt, idx, axis=1).reshape(n_dir, nb, -1))


@pytest.mark.gpu
def test_form_factor_jvp_direction_blocks():
    """tsff_form_factor_jvp at B = 65 with 7 directions: blocks of 3, 3 and 1 directions, fe_dot on all of them and on (0, 4, 6)."""
    torch = _torch()
    idx = members(FF_B, tff.B)
    eng = tff._engine(FF_CASE)
    worst, same = {}, True
    for what, (s, (Pt, Pdt)) in (("all", (tff._inputs(FF_CASE), tff._twin(FF_CASE))), ("some", ff_some())):
        X, fe = tiled(s["X"], idx), tiled(s["fe"], idx)
        P, Pd = eng.form_factor_jvp(0, X, fe, tiled(s["pd"], idx, axis=1), tiled(s["fd"], idx, axis=1), want_P=True)
        launched = eng.last_launch()
        # three direction blocks, each k_fe_direction, k_wgemm<2>, k_ffjvp<1, 3> (one k_wgemm<2> more in front: the W tables of the value)
        blocks = [i for i, k in enumerate(launched) if k == "k_fe_direction"]
        assert len(blocks) == 3 and all(launched[i:i + 3] == ["k_fe_direction", "k_wgemm<2>", "k_ffjvp<1, 3>"] for i in blocks), launched
        assert launched.count("k_ffjvp<1, 3>") == 3 and launched.count("k_wgemm<2>") == 3 + 1, launched
        assert launched[:launched.index("k_fe_direction")].count("k_wgemm<2>") == 1, launched
        assert torch.equal(P, eng.form_factor(0, X, fe))
        P, Pd = P.cpu().numpy(), Pd.cpu().numpy()
        assert np.max(np.abs(P - Pt[idx]) / np.abs(Pt[idx])) < 1e-7
        ratio = _jvp_ratios(Pd, Pdt, idx)
        worst[what] = float(np.max(ratio))
        ok = repeats_equal(P, idx) and repeats_equal(Pd, idx, axis=1)
        same = same and ok
        print(f"form_factor_jvp blocks, fe_dot on {what}: B = {FF_B}: max row ratio {worst[what]:.3e} (per direction {ratio.max(axis=1)}), "
              f"repeats bit-equal: {ok}")
    _record("test_form_factor_jvp_direction_blocks", f"k_ffjvp<1,3> B={FF_B} n_dir={FF_NDIR} max_row_ratio={max(worst.values()):.3e} "
            f"all={worst['all']:.3e} some={worst['some']:.3e} repeats_bit_equal={same}")
    assert max(worst.values()) <= at.ROW_TOL, worst
    assert same, "repeats of a member differ within one call"


@pytest.mark.gpu
def test_form_factor_jvp_one_table_lane():
    """The fallback gw = 1 of tsff_form_factor_jvp: at nvx = 652 three table lanes exceed the LDS, every direction runs in a
    launch of its own with one lane."""
    torch = _torch()
    from tsadar_amd.engine import Engine

    s, (Pt, Pdt) = lane_case()
    eng = Engine(s["cfg"], s["sa"], fe_mode=L.FE_PER_LINEOUT)
    P, Pd = eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"], want_P=True)
    launched = eng.last_launch()
    assert launched.count("k_ffjvp<1, 3>") == LANE_NDIR and launched.count("k_fe_direction") == 1, launched
    assert torch.equal(P, eng.form_factor(0, s["X"], s["fe"]))
    assert np.max(np.abs(P.cpu().numpy() - Pt) / np.abs(Pt)) < 1e-7
    ratio = _jvp_ratios(Pd.cpu().numpy(), Pdt, np.arange(LANE_B))
    print(f"form_factor_jvp one lane: nvx = {LANE_NVX}: max row ratio {np.max(ratio):.3e} ({ratio})")
    _record("test_form_factor_jvp_one_table_lane", f"k_ffjvp<1,3>x{LANE_NDIR} B={LANE_B} nvx={LANE_NVX} max_row_ratio={np.max(ratio):.3e} "
            "repeats_bit_equal=n/a")
    assert np.max(ratio) <= at.ROW_TOL, ratio
    # <Pbar, P_dot> = <grad_phys, phys_dot> + <grad_fe, fe_dot> against the shipped adjoint
    rng = np.random.default_rng(5)
    Pbar = torch.as_tensor(rng.standard_normal(tuple(Pd.shape[1:])), device=Pd.device) / Pd.abs().mean()
    gp, gf = [t.cpu().numpy() for t in eng.form_factor_grad(0, s["X"], s["fe"], Pbar, want_fe=True)]
    for k in range(LANE_NDIR):
        lhs = float((Pbar * Pd[k]).sum())
        rhs = float(np.sum(gp * s["pd"][k])) + float(np.sum(gf * s["fd"][k]))
        assert abs(lhs - rhs) <= 1e-7 * float((Pbar * Pd[k]).abs().sum()), (k, lhs, rhs)
    none, Pd2 = eng.form_factor_jvp(0, s["X"], s["fe"], s["pd"], s["fd"])
    assert none is None and torch.equal(Pd, Pd2)


@pytest.mark.gpu
def test_exact_hessian_second_pass_dlm_order():
    """Engine.loss_hess with the DLM order among the leaves at B npair >= 2 kHessMaxWG: every workgroup of k_hess_pairs runs a second
    task, on another lineout's W, Wm, Wmm and Hermite coefficients."""
    _torch()
    c = hess_members()
    idx = members(HESS_B, HESS_K)
    eng = the._engine_kw(c["cfg"], c["sa"])
    assert eng.fe_mode == L.FE_DLM
    terms, grad, hess = [t.cpu().numpy() for t in eng.loss_hess(tiled(c["X"], idx), tiled_batch(c["batch"], idx), the._weights(c["cfg"]), c["act"])]
    launched = eng.last_launch()
    for k in ("k_hess_mtab<1>", "k_hess_pairs<1>", "k_hess_finish"):
        assert k in launched, launched
    Ho = c["H"][idx]
    err = np.max(np.abs(hess - Ho), axis=(1, 2)) / np.max(np.abs(Ho), axis=(1, 2))
    same = repeats_equal(hess, idx) and repeats_equal(grad, idx)
    print(f"hessian: B = {HESS_B}: max |H - twin| / max |twin| per lineout {err.max():.3e} (members {[float(err[k]) for k in range(HESS_K)]}), "
          f"repeats bit-equal: {same}")
    _record("test_exact_hessian_second_pass_dlm_order", f"k_hess_mtab<1>+k_hess_pairs<1> B={HESS_B} max_row_ratio={err.max():.3e} "
            f"repeats_bit_equal={same}")
    assert np.array_equal(hess, np.transpose(hess, (0, 2, 1)))
    assert np.all(err <= the.HESS_TOL), (int(np.argmax(err)), err.max())
    for b in range(HESS_B):
        np.testing.assert_allclose(the._sigmas(hess[b]), the._sigmas(Ho[b]), rtol=the.SIGMA_RTOL)
    assert same, "repeats of a member differ within one call"
