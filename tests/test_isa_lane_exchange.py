"""Static check of the base-point exchange between lanes (EX) in every shipped instantiation that has it.

A pair's right-neighbour base point comes from the next lane's registers: five doubles, ten `v_mov_b32_dpp ... wave_shl:1`
(next_lane_f64, tsff_device.h).  The earlier forms went through LDS -- five `ds_write_b64` + five `ds_read_b64` behind two
wavefront barriers per angle (k_spectrum_fused, k_forward_pairs EXM 1) or ten `ds_bpermute_b32` (k_forward_pairs EXM 2).
k_spectrum_rows keeps the LDS form (the register form measured slower there, see its header) and is not listed.  This test
cross-compiles the 18 EX instantiations of the two kernels the library launches (tsff_api.inc: init_attributes and the dispatch
of launch_spectrum; no GPU needed, one compile of about a minute) and reads the device assembly:

* every angle loop -- an innermost loop that holds a `wave_shl:1` move -- holds exactly ten of them in the loss kernels and
  four in the forward-only one (the forward value reads xi_e and F of the neighbour point alone -- the finite difference along
  lambda -- and the compiler drops the three doubles only the reverse needs), no `ds_write` and no `ds_bpermute`; the kernel has
  as many such loops as it has sweeps (pairs per thread x {asymptotic, general} ion terms) and no `wave_shl:1` outside of them;
* the exchange costs no registers: spilled VGPRs and scratch bytes are not above, and the occupancy not below, what the same
  instantiation had with the exchange through LDS.  PARENT holds those figures, read from the kernel metadata
  (`.vgpr_spill_count`, `.private_segment_fixed_size`, `; Occupancy:`) of a build of the commit before the exchange moved into
  registers, by `isa.resources()`.  The one-sweep kernel stays at two wavefronts per SIMD.
"""
import pytest

import isa

_FUSED = "template __global__ void tsff::k_spectrum_fused<{n}, {gm}, {zh}, true>(tsff::KStatic, tsff::KCall, int, int, const double*);"
_PAIRS = "template __global__ void tsff::k_forward_pairs<{n}, {zh}, {exm}, {npair}>(tsff::KStatic, tsff::KCall, int, int, const double*);"
_B = {"false": 0, "true": 1}

# name -> (explicit instantiation, mangled-name prefix, number of sweeps, wave_shl:1 moves per angle)
KERNELS = {}
for _n in (1, 2):
    for _zh in ("false", "true"):
        for _gm in (0, 1):
            KERNELS[f"k_spectrum_fused<{_n}, {_gm}, {_zh}, true>"] = (
                _FUSED.format(n=_n, gm=_gm, zh=_zh), f"_ZN4tsff16k_spectrum_fusedILi{_n}ELi{_gm}ELb{_B[_zh]}ELb1EE", 4, 10)
        for _exm, _npair in ((2, 1), (1, 2)) + (((2, 2),) if _zh == "true" else ()):
            KERNELS[f"k_forward_pairs<{_n}, {_zh}, {_exm}, {_npair}>"] = (
                _PAIRS.format(n=_n, zh=_zh, exm=_exm, npair=_npair), f"_ZN4tsff15k_forward_pairsILi{_n}ELb{_B[_zh]}ELi{_exm}ELi{_npair}EE", 2 * _npair, 4)

# (spilled VGPRs, scratch bytes, occupancy) with the exchange through LDS / ds_bpermute: the commit before this one, resources()
PARENT = {
    "k_forward_pairs<1, false, 1, 2>": (0, 0, 4),
    "k_forward_pairs<1, false, 2, 1>": (0, 0, 4),
    "k_forward_pairs<1, true, 1, 2>": (0, 0, 4),
    "k_forward_pairs<1, true, 2, 1>": (0, 0, 4),
    "k_forward_pairs<1, true, 2, 2>": (0, 0, 4),
    "k_forward_pairs<2, false, 1, 2>": (0, 0, 3),
    "k_forward_pairs<2, false, 2, 1>": (0, 0, 4),
    "k_forward_pairs<2, true, 1, 2>": (0, 0, 3),
    "k_forward_pairs<2, true, 2, 1>": (0, 0, 4),
    "k_forward_pairs<2, true, 2, 2>": (0, 0, 3),
    "k_spectrum_fused<1, 0, false, true>": (2, 12, 2),
    "k_spectrum_fused<1, 0, true, true>": (6, 28, 2),
    "k_spectrum_fused<1, 1, false, true>": (33, 136, 2),
    "k_spectrum_fused<1, 1, true, true>": (33, 136, 2),
    "k_spectrum_fused<2, 0, false, true>": (76, 212, 2),
    "k_spectrum_fused<2, 0, true, true>": (76, 212, 2),
    "k_spectrum_fused<2, 1, false, true>": (108, 308, 2),
    "k_spectrum_fused<2, 1, true, true>": (98, 308, 2),
}


@pytest.fixture(scope="module")
def assembly():
    return isa.compile_assembly(v[0] for v in KERNELS.values())


def test_parent_table_is_complete():
    assert sorted(PARENT) == sorted(KERNELS)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_angle_loops_exchange_in_registers(assembly, name):
    _, prefix, nsweep, nmov = KERNELS[name]
    _, body = isa.function(assembly, prefix)
    insts, inner = isa.innermost_loops(body)
    angle = [(s, e) for s, e in inner if any("wave_shl:1" in t for t in insts[s:e + 1])]
    assert len(angle) == nsweep, (name, "angle loops", len(angle), nsweep)
    for s, e in angle:
        ops = insts[s:e + 1]
        shl = [t for t in ops if "wave_shl:1" in t]
        assert len(shl) == nmov and all(t.startswith("v_mov_b32_dpp") for t in shl), (name, s, e, shl)
        lds_out = [t for t in ops if t.startswith(("ds_write", "ds_bpermute", "ds_permute", "ds_swizzle"))]
        assert not lds_out, (name, s, e, lds_out)
    total = sum("wave_shl:1" in t for t in insts)
    assert total == nmov * nsweep, (name, "wave_shl:1 moves outside the angle loops", total)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_exchange_costs_no_registers(assembly, name):
    spill, scratch, occ = isa.resources(assembly, {k: v[1] for k, v in KERNELS.items()})[name]
    pspill, pscratch, pocc = PARENT[name]
    print(f"{name}: spilled VGPRs {spill} (parent {pspill}), scratch {scratch} B (parent {pscratch}), occupancy {occ} (parent {pocc})")
    assert spill <= pspill, (name, "spilled VGPRs", spill, pspill)
    assert scratch <= pscratch, (name, "scratch bytes", scratch, pscratch)
    assert occ >= pocc, (name, "occupancy", occ, pocc)
    if name.startswith("k_spectrum_fused"):
        assert occ == 2, (name, "occupancy", occ)
