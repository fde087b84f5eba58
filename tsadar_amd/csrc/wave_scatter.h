// wave_scatter.h -- the schedule of the grouped wavefront sums (wave_sums_scatter, tsff_device.h).  Plain constexpr C++, no device
// code: tests/test_reduce_scatter_model.py compiles it for the host and compares its tables with a NumPy model of 64 lanes.
//
// N values per lane are summed over the 64 lanes of a wavefront by reduce-scatter along the xor butterfly's own tree.  Before the
// step at offset o (32, 16, 8, 4) every lane holds n slots (n = N at first).  With h = (n + 1) / 2, the lanes whose bit o is clear
// keep slots [0, h) and the others slots [h, n), which they renumber [0, n - h); every lane sends the slots it does not keep to
// lane ^ o and adds what it receives to what it keeps -- h exchanges -- and n becomes h.  Once one slot is left (and for the offsets
// 2 and 1 always), the step is the plain butterfly v += v[lane ^ o].  A lane's slot s stands for the value off + s, and it holds
// `size` <= n values that mean anything (the upper lanes of an odd n keep one value less: their last slot is padding).
// Every addition is the one the butterfly of wave_sum makes for that value in that lane at that offset -- the same two operands --
// so the lanes that hold value k at the end hold wave_sum's bits of it.  The offsets 2 and 1 never scatter: the four lanes
// 4 g .. 4 g + 3 end with the same value, and N <= 16.
#pragma once
#include <cstdint>

namespace tsff {

constexpr int kScatterMax = 16;   // values per call: one per group of four lanes at most

// value whose sum `lane` holds at the end, or -1: a lane that kept only padding
constexpr int scatter_value_of_lane(int N, int lane) {
  int off = 0, size = N, n = N;
  for (int o = 32; o >= 4 && n > 1; o >>= 1) {
    const int h = (n + 1) / 2;
    if (lane & o) { off += h; size = size > h ? size - h : 0; }
    else size = size < h ? size : h;
    n = h;
  }
  return size > 0 ? off : -1;
}

// exchanges (one double each way) of the whole schedule: N = 14 -> 7 + 4 + 2 + 1 + 1 + 1 = 16, N = 5 -> 3 + 2 + 1 + 1 + 1 + 1 = 9
constexpr int scatter_exchanges(int N) {
  int n = N, c = 0;
  for (int o = 32; o >= 1; o >>= 1) {
    if (o >= 4 && n > 1) n = (n + 1) / 2;
    c += n;
  }
  return c;
}

// the same per group of four lanes, packed: nibble g of scatter_values(N) is the value of lanes 4 g .. 4 g + 3, bit g of
// scatter_valid(N) says whether they hold one
constexpr uint64_t scatter_values(int N) {
  uint64_t t = 0;
  for (int g = 0; g < 16; ++g) {
    const int k = scatter_value_of_lane(N, 4 * g);
    t |= (uint64_t)(k < 0 ? 0 : k) << (4 * g);
  }
  return t;
}
constexpr uint32_t scatter_valid(int N) {
  uint32_t m = 0;
  for (int g = 0; g < 16; ++g) m |= (uint32_t)(scatter_value_of_lane(N, 4 * g) >= 0) << g;
  return m;
}

}  // namespace tsff
