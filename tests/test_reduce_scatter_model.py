"""The grouped wavefront sums of the one-sweep kernel (wave_sums_scatter, tsff_device.h) against the butterfly they replace: a NumPy
model of 64 lanes, and the device helper's schedule tables (tsadar_amd/csrc/wave_scatter.h) against the model.  No GPU.

The schedule, as the header states it: before the step at offset o = 32, 16, 8, 4 every lane holds n slots; h = (n + 1) / 2; the
lanes with bit o clear keep slots [0, h), the others [h, n); every lane sends what it does not keep to lane ^ o and adds what it
receives to what it keeps; n becomes h.  With one slot left, and at the offsets 2 and 1, the step is the butterfly's
v += v[lane ^ o].  The model runs exactly that on (lane, slot) arrays and keeps, beside the numbers, which value each slot of each lane
stands for (-1: padding).  The butterfly (wave_sum) is the six steps v += v[lane ^ o] on every value in every lane.

Checked for N = 1, 2, 5, 14, 16 (and the 12 and 15 the kernel uses) on random doubles of mixed sign with magnitudes 1e-300 .. 1e300:
* every lane the schedule names for value k holds exactly the bits the butterfly leaves in that lane (so do all others it does not
  name as padding), and every value is held by some lane;
* the number of exchanges is 7 + 4 + 2 + 1 + 1 + 1 = 16 for N = 14 and 3 + 2 + 1 + 1 + 1 + 1 = 9 for N = 5, against 6 N;
* the header's constexpr tables -- value of a lane, the packed nibble table and valid mask the device code reads, the exchange
  count -- printed by a host program compiled from the header itself, are the model's for every N = 1 .. 16."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "tsadar_amd", "csrc", "wave_scatter.h")
LANES = 64
SIZES = (1, 2, 5, 12, 14, 15, 16)


def butterfly(v):
    """wave_sum on v[lane, k]: what every lane holds after the six xor steps"""
    v = v.copy()
    lanes = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ o]
    return v


def reduce_scatter(v):
    """-> (sums[lane], value[lane] or -1, exchanges): the grouped reduction on v[lane, k]"""
    lanes = np.arange(LANES)
    n = v.shape[1]
    x = v.copy()                                        # x[lane, slot]
    value = np.tile(np.arange(n), (LANES, 1))           # which value a slot stands for; -1: padding
    exchanges = 0
    for o in (32, 16, 8, 4, 2, 1):
        if o >= 4 and n > 1:
            h = (n + 1) // 2
            up = (lanes & o) != 0
            lo, hi = x[:, :h], np.zeros((LANES, h))
            hi[:, :n - h] = x[:, h:]
            vlo, vhi = value[:, :h], np.full((LANES, h), -1)
            vhi[:, :n - h] = value[:, h:]
            keep = np.where(up[:, None], hi, lo)
            send = np.where(up[:, None], lo, hi)
            x = keep + send[lanes ^ o]
            value = np.where(up[:, None], vhi, vlo)
            # (the partner keeps the same slots' worth of the same values: it is on the same side of bit o only for lower bits)
            n = h
        else:
            x = x + x[lanes ^ o]
        exchanges += n
    assert n == 1 or v.shape[1] > 16
    return x[:, 0], value[:, 0], exchanges


def random_doubles(rng, shape):
    return rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-300, 300, size=shape)


@pytest.mark.parametrize("n", SIZES)
def test_grouped_sums_hold_the_butterflys_bits(n):
    rng = np.random.default_rng(100 + n)
    for _ in range(20):
        v = random_doubles(rng, (LANES, n))
        with np.errstate(over="ignore"):
            ref = butterfly(v)
            got, value, exchanges = reduce_scatter(v)
        for k in range(n):
            holders = np.nonzero(value == k)[0]
            assert holders.size > 0 and holders.size % 4 == 0, (n, k, holders)
            assert np.array_equal(got[holders].view(np.uint64), ref[holders, k].view(np.uint64)), (n, k)
            assert np.all(ref[holders, k] == ref[holders[0], k])   # (and the butterfly's sum is the same in all of them)
        assert exchanges == sum_of_halvings(n) <= 6 * n


def sum_of_halvings(n):
    c = 0
    for o in (32, 16, 8, 4, 2, 1):
        if o >= 4 and n > 1:
            n = (n + 1) // 2
        c += n
    return c


def test_exchange_counts_of_the_kernels_groups():
    assert sum_of_halvings(14) == 7 + 4 + 2 + 1 + 1 + 1 == 16
    assert sum_of_halvings(5) == 3 + 2 + 1 + 1 + 1 + 1 == 9


@pytest.fixture(scope="module")
def header_tables(tmp_path_factory):
    """N -> (value of every lane, packed values, valid mask, exchanges) as the header's constexpr functions give them"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("scatter")
    src, exe = str(d / "tables.cpp"), str(d / "tables")
    open(src, "w").write('#include <cstdio>\n#include "%s"\nint main() {\n  for (int n = 1; n <= tsff::kScatterMax; ++n) {\n'
                         '    std::printf("%%d %%llu %%u %%d", n, (unsigned long long)tsff::scatter_values(n), tsff::scatter_valid(n), tsff::scatter_exchanges(n));\n'
                         '    for (int l = 0; l < 64; ++l) std::printf(" %%d", tsff::scatter_value_of_lane(n, l));\n    std::printf("\\n");\n  }\n}\n' % HEADER)
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, src], check=True)
    out = {}
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines():
        f = [int(t) for t in line.split()]
        out[f[0]] = (np.array(f[4:]), f[1], f[2], f[3])
    return out


@pytest.mark.parametrize("n", range(1, 17))
def test_header_tables_are_the_models(header_tables, n):
    _, value, exchanges = reduce_scatter(np.ones((LANES, n)))
    lane_value, packed, valid, count = header_tables[n]
    assert np.array_equal(lane_value, value), (n, lane_value, value)
    assert count == exchanges
    for g in range(16):   # what the device code reads: nibble g / bit g for the lanes 4 g .. 4 g + 3, whose first one stores
        assert np.all(value[4 * g:4 * g + 4] == value[4 * g])
        assert ((valid >> g) & 1) == int(value[4 * g] >= 0), (n, g)
        if value[4 * g] >= 0:
            assert ((packed >> (4 * g)) & 15) == value[4 * g], (n, g)
    assert sorted(set(value[value >= 0])) == list(range(n))   # every value has a lane that stores it
