"""Static check of the angle and tap loops of the one-sweep kernel (no GPU needed, one compile): what profiles/r12_loops_isa.txt lists.

Angle loops (innermost loops with the lane exchange's `wave_shl:1` moves), k_spectrum_fused<1, 0, false, true> and <1, 1, false, true>:
* the angle's constants (cos theta_a, w_a pref) arrive by ONE scalar load of the item's record (k_fused_prep) per iteration: no
  v_readfirstlane_b32 in the loop, exactly one s_load_dwordx4, and no more LDS reads than the lookups and the boundary point need
  (the two ds_read_b64 of the angle arrays are gone: the per-loop figures below are the parent's minus two);
* the VALU instructions of each loop (instructions that start with `v_`) are no more than the listed count.  The counts are those
  of the compiler the listing was made with; a later compiler may schedule differently but has no reason to need more.

Convolution loops (tests/test_isa_conv_pipeline.py's definition): one address step per phase array and no register copies --
at most four v_add_u32 and no v_mov_b64 in a body of 64 FMAs."""
import pytest

import isa
from test_isa_conv_pipeline import conv_loops, is_fma

_FUSED = "template __global__ void tsff::k_spectrum_fused<1, {gm}, false, true>(tsff::KStatic, tsff::KCall, int, int, const double*);"
# name -> (explicit instantiation, mangled-name prefix, [(VALU, LDS reads) of each angle loop, sorted])
KERNELS = {
    "k_spectrum_fused<1, 0, false, true>": (_FUSED.format(gm=0), "_ZN4tsff16k_spectrum_fusedILi1ELi0ELb0ELb1EE",
                                            [(354, 13), (358, 13), (476, 19), (484, 19)]),
    "k_spectrum_fused<1, 1, false, true>": (_FUSED.format(gm=1), "_ZN4tsff16k_spectrum_fusedILi1ELi1ELb0ELb1EE",
                                            [(407, 19), (413, 19), (529, 25), (537, 25)]),
}


@pytest.fixture(scope="module")
def assembly():
    return isa.compile_assembly(v[0] for v in KERNELS.values())


def angle_loops(body):
    insts, inner = isa.innermost_loops(body)
    return [ops for ops in (insts[s:e + 1] for s, e in inner) if any("wave_shl:1" in t for t in ops)]


def figures(ops):
    return sum(t.startswith("v_") for t in ops), sum(t.startswith("ds_read") for t in ops)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_angle_constants_come_by_one_scalar_load(assembly, name):
    _, prefix, listed = KERNELS[name]
    loops = angle_loops(isa.function(assembly, prefix)[1])
    assert len(loops) == 4, (name, len(loops))   # (two pairs) x (general, asymptotic)
    for ops in loops:
        print(name, "angle loop of %d instructions: VALU %d, LDS reads %d" % ((len(ops),) + figures(ops)))
        assert not [t for t in ops if t.startswith("v_readfirstlane")], name
        assert sum(t.startswith("s_load_dwordx4") for t in ops) == 1, name
        assert not [t for t in ops if t.startswith(("scratch_", "buffer_", "v_readlane", "v_writelane"))], name
    got = sorted(figures(ops) for ops in loops)
    for (valu, lds), (valu_max, lds_max) in zip(got, listed):
        assert valu <= valu_max, (name, "VALU instructions of an angle loop above the count profiles/r12_loops_isa.txt lists", got, listed)
        # (this bound IS the check that the two ds_read_b64 of the angle arrays are gone: an LDS read cannot be told by its address)
        assert lds <= lds_max, (name, "more LDS reads in an angle loop than the lookups and the boundary point need: the angle arrays are read again?", got, listed)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_convolution_loops_step_four_addresses_and_copy_nothing(assembly, name):
    _, prefix, _ = KERNELS[name]
    found = conv_loops(isa.function(assembly, prefix)[1])
    assert len(found) == 2, (name, len(found))
    for ops in found:
        adds, movs = sum(t.startswith("v_add_u32") for t in ops), sum(t.startswith("v_mov_b64") for t in ops)
        print(name, "convolution loop of %d instructions: %d FMAs, %d v_add_u32, %d v_mov_b64, VALU %d" %
              (len(ops), sum(map(is_fma, ops)), adds, movs, figures(ops)[0]))
        assert sum(map(is_fma, ops)) == 64 and adds <= 4 and movs == 0, (name, adds, movs)
