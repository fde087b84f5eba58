"""Static check of the software-pipelined IRF convolutions (conv4_phase, k_conv.inc).

The phase-layout convolution walks its taps in groups of four; sixteen FP64 FMAs per group, four explicit chains.  The rolled
loop requested the operands of two groups (LDS reads of the window, scalar loads of the taps) at the top of an iteration and
waited for them in front of the first FMA: a round trip exposed before every 32 FMAs.  The pipelined loop requests the operands of
the NEXT two groups right behind the wait for the current ones, so that the requests are in flight while 32 FMAs issue.

This test cross-compiles the instantiations below (no GPU needed, one compile) and reads the device assembly.  A convolution loop
is an innermost loop with at least 32 FP64 FMAs, a scalar load and an LDS read, and no `wave_shl:1` move (which marks the angle
loops of the sweep).  In every convolution loop, walking the body cyclically,

* at least 32 FP64 FMAs lie between any `ds_read*` / `s_load*` and the next `s_waitcnt` that names `lgkmcnt` (0 in the rolled
  loop);
* there is no spill traffic: no `scratch_`, `buffer_`, `v_readlane` or `v_writelane` instruction.

The one-sweep kernel has two such loops (forward and adjoint convolution), the forward-only kernel one.
"""
import pytest

import isa

_FUSED = "template __global__ void tsff::k_spectrum_fused<{n}, {gm}, false, true>(tsff::KStatic, tsff::KCall, int, int, const double*);"
_PAIRS = "template __global__ void tsff::k_forward_pairs<1, true, 2, 2>(tsff::KStatic, tsff::KCall, int, int, const double*);"

# name -> (explicit instantiation, mangled-name prefix, number of convolution loops)
KERNELS = {
    "k_spectrum_fused<1, 0, false, true>": (_FUSED.format(n=1, gm=0), "_ZN4tsff16k_spectrum_fusedILi1ELi0ELb0ELb1EE", 2),
    "k_spectrum_fused<2, 0, false, true>": (_FUSED.format(n=2, gm=0), "_ZN4tsff16k_spectrum_fusedILi2ELi0ELb0ELb1EE", 2),
    "k_spectrum_fused<1, 1, false, true>": (_FUSED.format(n=1, gm=1), "_ZN4tsff16k_spectrum_fusedILi1ELi1ELb0ELb1EE", 2),
    "k_forward_pairs<1, true, 2, 2>": (_PAIRS, "_ZN4tsff15k_forward_pairsILi1ELb1ELi2ELi2EE", 1),
}
MIN_FMAS = 32   # two tap groups


def is_fma(t):
    return t.startswith(("v_fma_f64", "v_fmac_f64"))


def is_request(t):
    return t.startswith(("ds_read", "s_load"))


def is_lgkm_wait(t):
    return t.startswith("s_waitcnt") and "lgkmcnt" in t


def conv_loops(body):
    insts, inner = isa.innermost_loops(body)
    return [ops for ops in (insts[s:e + 1] for s, e in inner)
            if sum(map(is_fma, ops)) >= MIN_FMAS and any(t.startswith("s_load") for t in ops) and any(t.startswith("ds_read") for t in ops)
            and not any("wave_shl:1" in t for t in ops)]


def fmas_behind_requests(ops):
    """for every request of the loop body: the FP64 FMAs between it and the next wait on lgkmcnt, walking the body cyclically"""
    n, out = len(ops), []
    assert any(map(is_lgkm_wait, ops)), "no wait on lgkmcnt in the loop"
    for i, t in enumerate(ops):
        if not is_request(t):
            continue
        k, j = 0, (i + 1) % n
        while not is_lgkm_wait(ops[j]):
            k += is_fma(ops[j])
            j = (j + 1) % n
        out.append((t, k))
    return out


@pytest.fixture(scope="module")
def assembly():
    return isa.compile_assembly(v[0] for v in KERNELS.values())


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_requests_fly_under_the_fma_chains(assembly, name):
    _, prefix, nconv = KERNELS[name]
    found = conv_loops(isa.function(assembly, prefix)[1])
    assert len(found) == nconv, (name, "convolution loops", len(found), nconv)
    for ops in found:
        behind = fmas_behind_requests(ops)
        print(f"{name}: loop of {len(ops)} instructions, {sum(map(is_fma, ops))} FMAs, {len(behind)} requests, "
              f"FMAs between a request and the next lgkmcnt wait: min {min(k for _, k in behind)}")
        short = [(t, k) for t, k in behind if k < MIN_FMAS]
        assert not short, (name, short)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_spill_traffic_in_the_convolution_loops(assembly, name):
    _, prefix, nconv = KERNELS[name]
    found = conv_loops(isa.function(assembly, prefix)[1])
    assert len(found) == nconv, (name, "convolution loops", len(found), nconv)
    for ops in found:
        bad = [t for t in ops if t.startswith(("scratch_", "buffer_", "v_readlane", "v_writelane"))]
        assert not bad, (name, bad)
