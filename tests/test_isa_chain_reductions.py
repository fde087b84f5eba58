"""Static check of the one-sweep kernel's wavefront reductions outside its angle and convolution loops (no GPU needed, one compile).

k_spectrum_fused<1, 0, false, true> (the headline instantiation) and <1, 1, false, true> (the DLM order among the leaves: the same
chain) sum their five mid-chain values and their lineout-scalar adjoints over the wavefront by reduce-scatter (wave_sums_scatter,
tsff_device.h; the schedule: wave_scatter.h, tests/test_reduce_scatter_model.py) instead of one six-step butterfly per value:

* the `ds_bpermute_b32` outside the angle and convolution loops are no more than the schedule needs if every exchange went through
  LDS -- two per exchange of a double, scatter exchanges of 14 and of 5 values: 2 x (16 + 9) -- plus what half_argmax keeps (six steps
  of a double and an int: 18).  The butterflies they replace took 2 x 6 x (14 + 5).  (The kernel sums 9 + 3 n_ion = 12 values at the
  end, not 14 -- the two block sums of its record need no wavefront sum -- and its exchanges at the offsets 32 and 16 are
  v_permlane32_swap / v_permlane16_swap, at 2 and 1 DPP moves: it stays well below the bound, which is the schedule's, not the code's.)
* none of them stands inside an angle or a convolution loop;
* no scratch traffic anywhere in the function.

The DLM instantiation spilled before this check existed (17 VGPRs, 72 B, 46 scratch instructions, none of them in the chain: the
intermediates of the k_s cache fill and two frequencies that no angle loop reads, kept across the sweeps for the cache's fallbacks).
kLeanKs (k_spectrum_fused.inc) keeps them out of registers there; both instantiations are at 0 spilled VGPRs, 0 B."""
import pytest

import isa
from test_isa_conv_pipeline import conv_loops
from test_isa_loops import KERNELS, angle_loops

STEPS = (32, 16, 8, 4, 2, 1)


def scatter_exchanges(n):
    """exchanges of the grouped reduction of n values: the values halve at 32, 16, 8, 4 while more than one is left"""
    c = 0
    for o in STEPS:
        if o >= 4 and n > 1:
            n = (n + 1) // 2
        c += n
    return c


GROUPS = (14, 5)                   # the end group (9 + 3 n_ion sums and the record's two block sums) and the mid-chain group
ARGMAX = len(STEPS) * (2 + 1)      # half_argmax: a double (two ds_bpermute_b32) and an int per step
BOUND = 2 * sum(scatter_exchanges(n) for n in GROUPS) + ARGMAX


@pytest.fixture(scope="module")
def assembly():
    return isa.compile_assembly(v[0] for v in KERNELS.values())


def test_bound_is_the_schedules():
    assert [scatter_exchanges(n) for n in GROUPS] == [7 + 4 + 2 + 1 + 1 + 1, 3 + 2 + 1 + 1 + 1 + 1]
    assert BOUND == 2 * (16 + 9) + 18 < 2 * len(STEPS) * sum(GROUPS) + ARGMAX


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_permutes_outside_the_loops(assembly, name):
    body = isa.function(assembly, KERNELS[name][1])[1]
    insts, _ = isa.innermost_loops(body)
    loops = angle_loops(body) + conv_loops(body)
    assert len(loops) == 6, (name, len(loops))
    total = sum(t.startswith("ds_bpermute_b32") for t in insts)
    inside = sum(t.startswith("ds_bpermute_b32") for ops in loops for t in ops)
    swaps = sum(t.startswith("v_permlane") for t in insts)
    print(f"{name}: ds_bpermute_b32 {total} ({inside} inside the angle and convolution loops), bound {BOUND}; lane swaps {swaps}")
    assert inside == 0, (name, inside)
    assert total - inside <= BOUND, (name, total, BOUND)
    assert not any(t.startswith("v_permlane") for ops in loops for t in ops), name


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_scratch_traffic(assembly, name):
    insts, _ = isa.innermost_loops(isa.function(assembly, KERNELS[name][1])[1])
    bad = [t for t in insts if t.startswith(("scratch_", "buffer_"))]
    print(f"{name}: {len(bad)} scratch instructions")
    assert not bad, (name, len(bad), bad[:4])
