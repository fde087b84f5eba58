// k_form_factor.inc -- raw 1-D form factor P[b][g][lambda][theta] and its adjoint for arbitrary seeds.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).

// ------------------------------------------------------------------------------------------
// k_form_factor: raw FormFactor.__call__ (form_factor.py:163-298) -> P[b][g][j][a], physical
// parameters in, no instrument chain.  One workgroup per lineout; any npts.
// ------------------------------------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(kThreads) void k_form_factor(KStatic S, KCall K, int f, const double* __restrict__ omgs,
                                                          int npts, double* __restrict__ P) {
  const int b = blockIdx.x, tid = threadIdx.x;
  extern __shared__ __align__(16) unsigned char smem[];
  const Smem m = carve(smem, S, 1, 0, false);
  Tables T;
  load_tables(m, S, K, S.shared_fe ? 0 : b, false, T);
  Phys<NI> p;
  load_phys<NI>(K.params + (size_t)b * S.NP, S.p_scale, S.p_shift, S.p_sig, S.ti_same, false, p);
  __syncthreads();
  const int G = S.G, NA = S.n_angles;
  const int nstrips = (npts + kStrip - 1) / kStrip;
  for (int st = tid; st < nstrips; st += kThreads) {
    const int j0 = st * kStrip;
    double ws[kStrip + 1];
#pragma unroll
    for (int q = 0; q <= kStrip; ++q) ws[q] = omgs[min(j0 + q, npts - 1)];
    for (int g = 0; g < G; ++g) {
      LineS<NI> L;
      make_lines<NI>(p, S.lam_shift[f], g, G, L);
      double ksv[kStrip + 1];
#pragma unroll
      for (int q = 0; q <= kStrip; ++q) ksv[q] = ks_eval(ws[q], L.wpe2);
      for (int a = blockIdx.y; a < NA; a += gridDim.y) {   // (few lineouts, many angles: the angles are spread over blockIdx.y)
        const double ct = m.cosa[a];
        Base b0;
        base_eval<NI>(ws[0], ksv[0], ct, L, T, b0);
#pragma unroll
        for (int q = 0; q < kStrip; ++q) {
          const int j = j0 + q;
          const bool has_next = (j + 1) < npts;
          Base b1;
          base_eval<NI>(ws[q + 1], ksv[q + 1], ct, L, T, b1);
          if (j < npts) P[(((size_t)b * G + g) * npts + j) * NA + a] = point_forward<NI>(ws[q], b0, b1, has_next, L, T);
          b0 = b1;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_form_factor_adj: reverse of k_form_factor for an arbitrary seed Pbar[b][g][j][a] (the angular instrument chain hands
// one back per (wavelength, angle) point, unlike the fit path whose seed is a spectrum adjoint times the angle
// weights).  The reverse sweep of k_spectrum with the same device functions: every point is recomputed and reversed,
// the lineout-scalar adjoints are reduced per workgroup and added to LBacc[b][g][:] (k_ff_lines_adj finishes the chain to
// the physical parameters), and with GM == 2 the adjoints of the two distribution-function tables are gathered in LDS
// and added to Wb_out / Hy_out / Hs_out (k_wgemm_t and k_fe_adjoint chain them to f_e, as for tsff_loss_grad_fe).
// Grid (B, angle chunks).
// ------------------------------------------------------------------------------------------
template <int NI, int GM>
__global__ __launch_bounds__(kThreads) void k_form_factor_adj(KStatic S, KCall K, int f, const double* __restrict__ omgs,
                                                              int npts, const double* __restrict__ Pbar,
                                                              double* __restrict__ LBacc) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  extern __shared__ __align__(16) unsigned char smem[];
  const Smem m = carve(smem, S, 1, GM, false);
  Tables T;
  load_tables(m, S, K, S.shared_fe ? 0 : b, false, T);
  Phys<NI> p;
  load_phys<NI>(K.params + (size_t)b * S.NP, S.p_scale, S.p_shift, S.p_sig, S.ti_same, false, p);
  if (GM == 2) {
    T.Wb = m.Wm; T.Hy = reinterpret_cast<double*>(m.hcm); T.Hs = T.Hy + S.nvx;
    for (int i = tid; i < kNXi2; i += kThreads) T.Wb[i] = 0.0;
    for (int i = tid; i < 2 * S.nvx; i += kThreads) T.Hy[i] = 0.0;
  }
  __syncthreads();
  constexpr int NLB = 9 + 3 * NI;
  const int G = S.G, NA = S.n_angles;
  const int nstrips = (npts + kStrip - 1) / kStrip;
  FeAcc fa;
  fe_acc_init(fa);
  for (int g = 0; g < G; ++g) {
    LineS<NI> L, LB;
    make_lines<NI>(p, S.lam_shift[f], g, G, L);
    zero_lines<NI>(LB);
    for (int st = tid; st < nstrips; st += kThreads) {
      const int j0 = st * kStrip;
      double ws[kStrip + 1], ksv[kStrip + 1];
#pragma unroll
      for (int q = 0; q <= kStrip; ++q) { ws[q] = omgs[min(j0 + q, npts - 1)]; ksv[q] = ks_eval(ws[q], L.wpe2); }
      for (int a = blockIdx.y; a < NA; a += gridDim.y) {
        const double ct = m.cosa[a];
        Base b0;
        base_eval<NI>(ws[0], ksv[0], ct, L, T, b0);
        double cxe = 0.0, cF = 0.0;
#pragma unroll
        for (int q = 0; q < kStrip; ++q) {
          const int j = j0 + q;
          const bool has_next = (j + 1) < npts;
          Base b1;
          base_eval<NI>(ws[q + 1], ksv[q + 1], ct, L, T, b1);
          if (j < npts) {
            BaseAdj ba;
            double xen, Fn;
            point_reverse<NI, GM>(b0, b1, has_next, L, T,
                                  Pbar[(((size_t)b * G + g) * npts + j) * NA + a] * (L.pref * ws[q] * ws[q]), ba, xen, Fn, LB, fa);
            ba.xe += cxe; ba.F += cF;
            base_reverse<NI, GM>(ct, b0, L, T, ba, LB, fa);
            cxe = xen; cF = Fn;
          }
          b0 = b1;
        }
        if (j0 + kStrip < npts) {  // the strip's right neighbour receives the D-coupling of the last point
          BaseAdj ba;
          ba.k2 = ba.ik = ba.wd = 0.0; ba.xe = cxe; ba.F = cF;
          base_reverse<NI, GM>(ct, b0, L, T, ba, LB, fa);
        }
      }
    }
    lines_adjoint_finalize<NI>(L, LB);   // deferred wavefront-uniform factors of point_reverse
    double lb[NLB];
    lines_adj_store<NI>(LB, lb);
    // one partial per wavefront and angle chunk, plain stores; k_lbacc_reduce adds them in a fixed order
    const int nworker = (int)gridDim.y * (kThreads / 64), worker = (int)blockIdx.y * (kThreads / 64) + (tid >> 6);
#pragma unroll
    for (int k = 0; k < NLB; ++k) {
      const double v = wave_sum(lb[k]);
      if (lane == 0) LBacc[(((size_t)b * G + g) * nworker + worker) * NLB + k] = v;
    }
  }
  if (GM == 2) {
    fe_flush_w(fa, T.Wb);
    fe_flush_h(fa, T.Hy, T.Hs);
    __syncthreads();
    // per angle chunk: [chunk][B][.] blocks, summed over the chunks in order by k_sum_chunks (no global atomics)
    const size_t cw = (size_t)blockIdx.y * K.B * kNXi2, ch = (size_t)blockIdx.y * 2 * K.B * S.nvx;
    for (int i = tid; i < kNXi2; i += kThreads) K.Wb_out[cw + (size_t)b * kNXi2 + i] = T.Wb[i];
    for (int i = tid; i < S.nvx; i += kThreads) {
      K.Hy_out[ch + (size_t)b * S.nvx + i] = T.Hy[i];
      K.Hs_out[ch + (size_t)b * S.nvx + i] = T.Hs[i];
    }
  }
}

// a[i] = sum over c < nchunk of a[c * n + i] (in order): the per-angle-chunk table adjoints of k_form_factor_adj
__global__ __launch_bounds__(kThreads) void k_sum_chunks(double* __restrict__ a, long n, int nchunk) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    double v = a[i];
    for (int c = 1; c < nchunk; ++c) v += a[(size_t)c * n + i];
    a[i] = v;
  }
}
