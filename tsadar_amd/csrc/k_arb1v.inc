// k_arb1v.inc -- the free-form 1-D f_e generator (tsadar_amd.distribution.arbitrary_1v, the reference's Arbitrary1V.__call__) and
// its adjoint (distribution.arbitrary_1v_vjp) on the device: tsff_arb1v_table, tsff_arb1v_table_vjp and the TSFF_ANG_ARB1V
// generator of tsff_angular_fit.
//   forward: u = S fval (S: the constant forward-backward Butterworth matrix) -> f = exp(-ln 10 (7 u)^2) -> Z = sum f ->
//            f_e = f / Z / dvx;
//   adjoint: g_f = (fe_bar / dvx - sum fe_bar f_e) / Z -> g_u = g_f (-ln 10 f) 98 u -> grad = S^T g_u.
// gen_data: S[nv][nv] | S^T[nv][nv], row-major doubles (distribution.arb1v_gen_data): both products read their matrix along rows.
// ws (scratch): u[nv] | g_u[nv].  The adjoint's pointwise kernel rebuilds f, Z and f_e from u (nv <= 4096 exponentials), so the
// forward leaves u behind and nothing else; inside the fit the adjoint reuses the u of the epoch's forward.
//
// k_arb1v_matvec: y = M x, one wavefront per row and kArb1vRows rows per workgroup; the lanes stride along the row (coalesced:
// 64 consecutive doubles per load, every element of M read once, no LDS), four partial sums per lane in a fixed order, then the
// butterfly of wave_sum.  k_arb1v_point: one workgroup, the pointwise part and the two scalar sums.  Every sum has a fixed
// order and nothing is accumulated atomically: two calls on the same input give the same bits.
constexpr int kArb1vRows = kThreads / 64;
constexpr int kArb1vMaxNv = 4096;                        // the handle's nvx range
constexpr int kArb1vPer = kArb1vMaxNv / kThreads;        // points per thread of k_arb1v_point, kept in registers

inline size_t arb1v_ws_doubles(int nv) { return 2 * (size_t)nv; }

__global__ __launch_bounds__(kThreads) void k_arb1v_matvec(const double* __restrict__ M, const double* __restrict__ x, int nv,
                                                           double* __restrict__ y) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * kArb1vRows + (threadIdx.x >> 6);
  if (row >= nv) return;   // (uniform over the wavefront; the kernel has no barrier)
  const double* __restrict__ m = M + (size_t)row * nv;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int j = lane;
  for (; j + 192 < nv; j += 256) {
    a0 += m[j] * x[j];
    a1 += m[j + 64] * x[j + 64];
    a2 += m[j + 128] * x[j + 128];
    a3 += m[j + 192] * x[j + 192];
  }
  for (; j < nv; j += 64) a0 += m[j] * x[j];
  const double s = wave_sum((a0 + a1) + (a2 + a3));
  if (lane == 0) y[row] = s;
}

// fe_bar == nullptr: out = f_e[nv].  Otherwise out = g_u[nv], the adjoint of u given fe_bar = d loss / d f_e.
__global__ __launch_bounds__(kThreads) void k_arb1v_point(const double* __restrict__ u, int nv, double dvx, double ln10,
                                                          const double* __restrict__ fe_bar, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  double f[kArb1vPer];
  double z = 0.0;
#pragma unroll
  for (int k = 0; k < kArb1vPer; ++k) {
    const int j = threadIdx.x + k * kThreads;
    f[k] = 0.0;
    if (j < nv) {
      const double a = 7.0 * u[j];
      f[k] = exp(-ln10 * (a * a));
    }
    z += f[k];
  }
  const double Z = block_sum(z, red);
  if (!fe_bar) {
#pragma unroll
    for (int k = 0; k < kArb1vPer; ++k) {
      const int j = threadIdx.x + k * kThreads;
      if (j < nv) out[j] = f[k] / Z / dvx;
    }
    return;
  }
  double d = 0.0;
#pragma unroll
  for (int k = 0; k < kArb1vPer; ++k) {
    const int j = threadIdx.x + k * kThreads;
    if (j < nv) d += fe_bar[j] * (f[k] / Z / dvx);
  }
  const double dot = block_sum(d, red);
#pragma unroll
  for (int k = 0; k < kArb1vPer; ++k) {
    const int j = threadIdx.x + k * kThreads;
    if (j < nv) {
      const double gf = (fe_bar[j] / dvx - dot) / Z;
      out[j] = (gf * (-ln10 * f[k])) * (98.0 * u[j]);
    }
  }
}
