// k_ffjvp.inc -- forward mode of the raw 1-D form factor (tsff_form_factor_jvp): k_ffjvp.  Part of the single translation unit
// tsff_kernels.hip (included inside namespace tsff, after k_jacobian.inc).
//
// P_dot[d] = dP/dphys . phys_dot[d] + dP/dfe . fe_dot[d] for arbitrary directions d: the chain functions of k_fwdmode.inc on the
// value with W tangents of k_jacobian.inc (TN<W>), one group of W directions per launch.  The parameters are PHYSICAL, as
// k_form_factor takes them (Ti tying as load_phys applies it, no activation, no fraction renormalisation), so a direction seeds the
// physical parameters directly.  A direction of f_e reaches a point through the two tables: lane k of the group carries the tangent
// of W and the Hermite coefficients of the tangent of ln f_e along its own direction (k_fe_direction + the W-table GEMM), which the
// lookups add to that lane (MTabT's lanes).  Grid (B, angle chunks) as k_form_factor's; no atomics; DESIGN.md section 4.4c.
//
// Table convention: that of k_fwdmode.inc (Z' and W carry their slope, the Hermite ln f_e lookup its true derivative).

// one launch of k_ffjvp, passed by value
struct FfjvpArgs {
  int d0, nd;              // this launch: directions [d0, d0 + nd) of the call's n_dir, nd <= W
  int nlane;               // lanes that carry a table direction: 0 (no fe_dot) or nd
  const double* phys_dot;  // [n_dir][B][NP]
  const double2* htd;      // nlane > 0: [nd][B][nvx] (d ln f_e, its node slope) of this launch's directions
  const double* Wd;        // nlane > 0: [nd][B][1640] the tangents of W
  double* P_dot;           // [n_dir][B][G][npts][NA]
};

// LDS of one k_ffjvp workgroup (doubles): Z', W and the Hermite coefficients, the same two per table lane, the angles, the physical
// parameters and the lineout scalars with their W tangents
__host__ __device__ inline size_t ffjvp_smem_doubles(const KStatic& S, int nlane, int W) {
  size_t n = 2 * (size_t)kNXi2 + kNXi2 + 4 * (size_t)S.nvx;
  n += (size_t)nlane * ((size_t)kNXi2 + 4 * (size_t)S.nvx);
  n += (size_t)S.n_angles + (size_t)(1 + W) * ((kNP_MAX + 1) + (9 + 4 * TSFF_MAX_ION));
  return n;
}

template <int NI, int W>
__global__ __launch_bounds__(kThreads) void k_ffjvp(KStatic S, KCall K, FfjvpArgs A, int f, const double* __restrict__ omgs, int npts) {
  using N = TN<W>;
  constexpr int NPk = TSFF_NP(NI);
  extern __shared__ __align__(16) unsigned char smem[];
  double2* zp = reinterpret_cast<double2*>(smem);          // [1640] full Z' table
  double* Wt = reinterpret_cast<double*>(zp + kNXi2);      // [1640]
  double2* hc = reinterpret_cast<double2*>(Wt + kNXi2);    // [2 (nvx - 1)] (+ padding)
  double* Wd = reinterpret_cast<double*>(hc + 2 * S.nvx);  // [nlane][1640] tangents of W
  double2* hcd = reinterpret_cast<double2*>(Wd + (size_t)A.nlane * kNXi2);   // [nlane][2 nvx] Hermite coefficients of the tangents of ln f_e
  double* cosa = reinterpret_cast<double*>(hcd + (size_t)A.nlane * 2 * S.nvx);
  N* ph = reinterpret_cast<N*>(cosa + S.n_angles);          // [NP + 1]
  LineT<N, NI>* Lsh = reinterpret_cast<LineT<N, NI>*>(ph + kNP_MAX + 1);   // lineout scalars of the current gradient point
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = S.G, NA = S.n_angles, B = K.B, nvx = S.nvx;
  const int slot = S.shared_fe ? 0 : b;
  for (int i = tid; i < kNXi2; i += kThreads) { zp[i] = S.zpf[i]; Wt[i] = K.W[(size_t)slot * kNXi2 + i]; }
  for (int i = tid; i < NA; i += kThreads) cosa[i] = S.cos_sa[i];
  for (int i = tid; i < nvx - 1; i += kThreads) {
    double2 c01, c23;
    hermite_coeffs(K.ht[(size_t)slot * nvx + i], K.ht[(size_t)slot * nvx + i + 1], S.dv, c01, c23);
    hc[2 * i] = c01; hc[2 * i + 1] = c23;
  }
  for (int k = 0; k < A.nlane; ++k) {
    const double* __restrict__ wk = A.Wd + ((size_t)k * B + b) * kNXi2;
    const double2* __restrict__ hk = A.htd + ((size_t)k * B + b) * nvx;
    for (int i = tid; i < kNXi2; i += kThreads) Wd[(size_t)k * kNXi2 + i] = wk[i];
    for (int i = tid; i < nvx - 1; i += kThreads) {
      double2 c01, c23;
      hermite_coeffs(hk[i], hk[i + 1], S.dv, c01, c23);
      hcd[(size_t)k * 2 * nvx + 2 * i] = c01; hcd[(size_t)k * 2 * nvx + 2 * i + 1] = c23;
    }
  }
  // ---- the physical parameters with the group's seeds (load_phys without activation: Ti tying only) ----
  if (tid == 0) {
    const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
    for (int s = 0; s < NPk; ++s) {
      N v = N::of(xpar[s]);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < A.nd) v.d[k] = A.phys_dot[((size_t)(A.d0 + k) * B + b) * S.NP + s];
      ph[s] = v;
    }
    for (int s = 1; s < NI; ++s)
      if (S.ti_same[s]) ph[TSFF_P_ION0 + 4 * s + TSFF_ION_TI] = ph[TSFF_P_ION0 + TSFF_ION_TI];
  }
  __syncthreads();
  const Tables T = make_tables(S, zp, Wt, nullptr, hc);
  MTabT<N> Mt;
  Mt.on = false; Mt.Wm = nullptr; Mt.Wmm = nullptr; Mt.hcm = nullptr; Mt.hcmm = nullptr; Mt.m = N::of(0.0);
  Mt.nlane = A.nlane; Mt.Wd = Wd; Mt.hcd = hcd; Mt.hstride = 2 * nvx;
  const size_t dstride = (size_t)B * G * npts * NA;   // one direction of P_dot
  const int nstrips = (npts + kStrip - 1) / kStrip;

  for (int g = 0; g < G; ++g) {
    if (g > 0) __syncthreads();   // (every reader of the previous gradient point's scalars is done)
    if (tid == 0) make_lines_hd<NI>(ph, S.lam_shift[f], g, G, *Lsh);
    __syncthreads();
    const LineT<N, NI>& L = *Lsh;   // (read from LDS where used, as in k_jac_sweep: the scalars and their tangents stay out of the registers)
    double* __restrict__ out = A.P_dot + (size_t)A.d0 * dstride + ((size_t)b * G + g) * npts * NA;
    for (int st = tid; st < nstrips; st += kThreads) {
      const int j0 = kStrip * st;
      for (int a = blockIdx.y; a < NA; a += gridDim.y) {   // (few lineouts, many angles: the angles are spread over blockIdx.y)
        const double ct = cosa[a];
        BaseT<N> b0;
        base_hd<NI>(omgs[min(j0, npts - 1)], ct, L, T, Mt, b0);
        for (int q = 0; q < kStrip; ++q) {
          __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (as in k_hess_pairs: the scalars are re-read per point, not hoisted)
          const int j = j0 + q;
          if (j >= npts) break;
          const bool has_next = j + 1 < npts;
          const double ws = omgs[j];
          BaseT<N> b1;
          base_hd<NI>(omgs[min(j + 1, npts - 1)], ct, L, T, Mt, b1);
          const N v = point_hd<NI>(b0, b1, has_next, L, T, Mt) * L.pref * (ws * ws);
#pragma unroll
          for (int k = 0; k < W; ++k)
            if (k < A.nd) out[(size_t)k * dstride + (size_t)j * NA + a] = v.d[k];
          b0 = b1;
        }
      }
    }
  }
}
