// k_jacobian.inc -- Jacobian of the model spectra w.r.t. the fitted leaves and the Gauss-Newton curvature of the fit loss:
// k_jac_sweep.  Part of the single translation unit tsff_kernels.hip (included inside namespace tsff, after k_hessian.inc).
//
// First-order forward mode through the chain k_hessian.inc differentiates (k_fwdmode.inc: generic over the number type): one
// workgroup evaluates a lineout with a value and W tangents side by side -- table lookups, exp, reciprocals, square roots and the
// Hermite cell are evaluated once per point and shared by the W leaves of a group; the groups of W leaves follow each other when
// the call has more active leaves.  The spectrum of a feature ((1 + W) npts doubles) lives in LDS.  Per binned sample j the
// tangents of Thry_f[j] are the Jacobian rows J_f[a][j]; they go to the caller (tsff_spectrum_jacobian) or, for
// tsff_loss_gauss_newton, into the workgroup's scratch rows from which
//   gn[a][c] = sum_k w_k sum_{j in mask_k} l''(d_j, t_j) J[a][j] J[c][j],   grad[a] = sum_k w_k sum_{j in mask_k} l'(d_j, t_j) J[a][j]
// are summed in a fixed order (thread-strided partials, wave_sum, block_sum; no atomics).  DESIGN.md section 4.4b.
//
// Where the hand-written reverse of the pair sweeps exists (1-2 ion species, one gradient point, no DLM order among the leaves, no
// raw feature) the sweep runs in its row form instead (k_jac_sweep<NI, 3, true>, jac_rows_sweep below); the tail is the same.
//
// Table convention: that of k_fwdmode.inc (Z' and W carry their slope, the Hermite ln f_e lookup its true derivative).

template <int W>
struct TN {   // a value and W first-order tangents
  double v, d[W];
  static constexpr bool kSecondOrder = false;
  static constexpr int kLanes = W;   // (each tangent may carry a table direction of its own: MTabT)
  static __device__ __forceinline__ TN of(double c) {
    TN r;
    r.v = c;
#pragma unroll
    for (int k = 0; k < W; ++k) r.d[k] = 0.0;
    return r;
  }
};
#define TSFF_TN_EACH for (int k = 0; k < W; ++k)
template <int W> __device__ __forceinline__ TN<W> operator+(TN<W> x, TN<W> y) {
  TN<W> r; r.v = x.v + y.v;
#pragma unroll
  TSFF_TN_EACH r.d[k] = x.d[k] + y.d[k];
  return r;
}
template <int W> __device__ __forceinline__ TN<W> operator-(TN<W> x, TN<W> y) {
  TN<W> r; r.v = x.v - y.v;
#pragma unroll
  TSFF_TN_EACH r.d[k] = x.d[k] - y.d[k];
  return r;
}
template <int W> __device__ __forceinline__ TN<W> operator-(TN<W> x) {
  TN<W> r; r.v = -x.v;
#pragma unroll
  TSFF_TN_EACH r.d[k] = -x.d[k];
  return r;
}
template <int W> __device__ __forceinline__ TN<W> operator+(TN<W> x, double c) { x.v += c; return x; }
template <int W> __device__ __forceinline__ TN<W> operator+(double c, TN<W> x) { x.v += c; return x; }
template <int W> __device__ __forceinline__ TN<W> operator-(TN<W> x, double c) { x.v -= c; return x; }
template <int W> __device__ __forceinline__ TN<W> operator-(double c, TN<W> x) {
  TN<W> r; r.v = c - x.v;
#pragma unroll
  TSFF_TN_EACH r.d[k] = -x.d[k];
  return r;
}
template <int W> __device__ __forceinline__ TN<W> operator*(TN<W> x, double c) {
  TN<W> r; r.v = x.v * c;
#pragma unroll
  TSFF_TN_EACH r.d[k] = x.d[k] * c;
  return r;
}
template <int W> __device__ __forceinline__ TN<W> operator*(double c, TN<W> x) { return x * c; }
template <int W> __device__ __forceinline__ TN<W> operator*(TN<W> x, TN<W> y) {
  TN<W> r; r.v = x.v * y.v;
#pragma unroll
  TSFF_TN_EACH r.d[k] = __builtin_fma(x.d[k], y.v, x.v * y.d[k]);
  return r;
}
// f(x) from f and f' (the curvature belongs to the second-order number)
template <int W> __device__ __forceinline__ TN<W> hd_chain(TN<W> x, double f, double d1, double) {
  TN<W> r; r.v = f;
#pragma unroll
  TSFF_TN_EACH r.d[k] = d1 * x.d[k];
  return r;
}
template <int W> __device__ __forceinline__ TN<W> hd_xm(TN<W> x, TN<W> m, double f, double fx, double fm, double, double, double) {
  TN<W> r; r.v = f;
#pragma unroll
  TSFF_TN_EACH r.d[k] = __builtin_fma(fx, x.d[k], fm * m.d[k]);
  return r;
}
// 1/x and sqrt(x) from the hardware seeds with one refinement step (frcp, fsqrt2: what the spectrum kernels use), in place of the
// generic forms' IEEE division and library sqrt
template <int W> __device__ __forceinline__ TN<W> hd_rcp(TN<W> x) {
  const double r = frcp(x.v);
  return hd_chain(x, r, -r * r, 0.0);
}
template <int W> __device__ __forceinline__ TN<W> hd_sqrt(TN<W> x) {
  double s, is;
  fsqrt2(x.v, s, is);
  return hd_chain(x, s, 0.5 * is, 0.0);
}
// (the chain's two exponentials, of ln f_e in [-50, 2] and of -xi_i^2 <= 0: the polynomial exp of the spectrum kernels)
template <int W> __device__ __forceinline__ TN<W> hd_exp(TN<W> x) {
  const double e = fexp(x.v);
  return hd_chain(x, e, e, 0.0);
}
template <int W> __device__ __forceinline__ TN<W> operator/(TN<W> x, TN<W> y) { return x * hd_rcp(y); }
template <int W> __device__ __forceinline__ TN<W> operator/(double c, TN<W> y) { return c * hd_rcp(y); }
#undef TSFF_TN_EACH

// one tsff_spectrum_jacobian / tsff_loss_gauss_newton call, passed by value
struct JacArgs {
  int n;                 // number of active leaves
  int slot[kNP_MAX];     // their parameter slots, in ravel order
  int with_m;            // the DLM order m is an active leaf: the m-derivative tables take part
  int want_gn;           // tsff_loss_gauss_newton: loss, gradient and Gauss-Newton matrix (else the Jacobian rows go to jac)
  double* jac[2];        // [B][n][1024] per feature, or nullptr
  double* xg;            // the row form (ROWS): per workgroup (1 + n) * npts doubles of scratch, the feature's spectrum and its n tangents
  double* rows;          // want_gn: per workgroup n * 1024 doubles of scratch (the rows of the current feature)
  double* grad;          // [B][n]
  double* gn;            // [B][n][n]
  double w[3];           // weights of S_iaw, S_blue, S_red
  int fit_denoms;        // want_gn, l2: the denominators are constants folded into w (the fit loss), not |d| + 1e-10
  const int32_t* skip;   // [B] or nullptr: the persistent workgroups pass over lineout b when skip[b] != 0 (nothing of it is written)
};

// sample j of the LDS spectrum: the four samples of a strip lie a quarter of the (padded) array apart, so that the threads of a
// wavefront, which own consecutive strips, touch consecutive doubles
constexpr int kJacPad = 8;
__host__ __device__ inline int jac_qstride(int npts) { return npts / kStrip + kJacPad; }
__device__ __forceinline__ int jac_at(int j, int qs) { return (j & (kStrip - 1)) * qs + (j >> 2); }
static_assert(kStrip == 4, "jac_at is written for strips of four samples");

// LDS of one k_jac_sweep workgroup (doubles): the tables (with_m: dW/dm and the Hermite coefficients of d ln f_e / dm), angles,
// the physical parameters, the maximum, the lineout scalars, and the spectrum with its W tangents
__host__ __device__ inline size_t jac_smem_doubles(const KStatic& S, bool with_m, int W) {
  size_t n = 2 * (size_t)kNXi2 + kNXi2 + 4 * (size_t)S.nvx + 2 * (size_t)S.n_angles + 16;
  if (with_m) n += (size_t)kNXi2 + 4 * (size_t)S.nvx;
  n += (size_t)(1 + W) * ((kNP_MAX + 1) + 1 + (9 + 4 * TSFF_MAX_ION));
  n += (size_t)(1 + W) * kStrip * jac_qstride(S.npts);
  return n;
}

// the row form (ROWS, below): fields of a row, and the LDS of its workgroup
__host__ __device__ constexpr int jac_row_fields(int NI) { return 8 + 3 * NI; }   // wpe2, wL, kL, ivTe, a_e, pref, Ud, Vd | ixi, a_i, cs per species
__host__ __device__ inline size_t jac_rows_smem_doubles(const KStatic& S, int n) {
  return jac_smem_doubles(S, false, 3) + (size_t)jac_row_fields(TSFF_MAX_ION) * n + 10 + 4 * TSFF_MAX_ION;
}

// l'(d, t) and l''(d, t) w.r.t. the model value t, and the value, with the denominators of _loss_for_hess_fn_ (|d| + 1e-10 for l2)
// or, fit_denoms, with l2's taken as constants that the weights carry (LossFunction.__loss__: e = r^2, e' = -2 r, e'' = 2)
__device__ __forceinline__ void jac_loss(int method, bool fit_denoms, double d, double t, double& e, double& e1, double& e2) {
  const double r = d - t;
  if (method == TSFF_LOSS_L2) {
    const double iu = fit_denoms ? 1.0 : 1.0 / (fabs(d) + 1e-10);
    e = r * r * iu; e1 = -2.0 * r * iu; e2 = 2.0 * iu;
  } else if (method == TSFF_LOSS_LOGCOSH) {
    const double th = tanh(r);
    e = log(cosh(r)); e1 = -th; e2 = 1.0 - th * th;
  } else {   // poisson
    const double it = 1.0 / t;
    e = t - d * log(t); e1 = 1.0 - d * it; e2 = d * it * it;
  }
}

// the physical parameters of lineout b with the seeds of the group of leaves starting at g0 (stage_phys: activation, Ti tying,
// fraction renormalisation); one thread
template <int NI, int W>
__device__ __forceinline__ void jac_stage_phys(const KStatic& S, const KCall& K, const JacArgs& A, int b, int g0, TN<W>* ph) {
  using N = TN<W>;
  constexpr int NPk = TSFF_NP(NI);
  const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
  for (int s = 0; s < NPk; ++s) {
    N v = N::of(xpar[s]);
#pragma unroll
    for (int k = 0; k < W; ++k)
      if (g0 + k < A.n && A.slot[g0 + k] == s) v.d[k] = 1.0;
    if (S.p_sig[s]) v = hd_sigmoid(v);
    ph[s] = v * S.p_scale[s] + S.p_shift[s];
  }
  tie_and_renorm<NI>(S, ph);
}

// the row sweep of one (lineout, feature): x_j and its n tangents into xg[(1 + n)][npts] (before the factor ws^2); all threads,
// returns behind a barrier
template <int NI, int W>
__device__ __forceinline__ void jac_rows_sweep(const KStatic& S, const KCall& K, const JacArgs& A, int b, int f, const Tables& T,
                                               TN<W>* ph, LineT<TN<W>, NI>* Lt, LineS<NI>* Lv, double* dl, const double* cosa,
                                               const double* wsa, double* __restrict__ xg) {
  constexpr int NF = jac_row_fields(NI);
  const int tid = threadIdx.x, n = A.n, npts = S.npts, NA = S.n_angles;
  if (tid == 0) {   // the lineout scalars and their tangents w.r.t. every leaf, group by group
    for (int g0 = (n - 1) / W * W; g0 >= 0; g0 -= W) {   // (the first group last: ph is left with its seeds for the tail)
      jac_stage_phys<NI, W>(S, K, A, b, g0, ph);
      make_lines_hd<NI>(ph, S.lam_shift[f], 0, 1, *Lt);
      const LineT<TN<W>, NI>& Q = *Lt;
      for (int k = 0; k < W && g0 + k < n; ++k) {
        double* d = dl + g0 + k;
        d[0] = Q.wpe2.d[k]; d[n] = Q.wL.d[k]; d[2 * n] = Q.kL.d[k]; d[3 * n] = Q.ivTe.d[k]; d[4 * n] = Q.a_e.d[k];
        d[5 * n] = Q.pref.d[k]; d[6 * n] = Q.Ud.d[k]; d[7 * n] = Q.Vd.d[k];
        for (int s = 0; s < NI; ++s) { d[(8 + 3 * s) * n] = Q.ixi[s].d[k]; d[(9 + 3 * s) * n] = Q.a_i[s].d[k]; d[(10 + 3 * s) * n] = Q.cs[s].d[k]; }
      }
      if (g0 == 0) {
        LineS<NI>& V = *Lv;
        V.wpe2 = Q.wpe2.v; V.wL = Q.wL.v; V.kL = Q.kL.v; V.ivTe = Q.ivTe.v; V.a_e = Q.a_e.v; V.pref = Q.pref.v; V.Ud = Q.Ud.v; V.Vd = Q.Vd.v;
        V.i2wL = Q.i2wL.v; V.m = 0.0;
        for (int s = 0; s < NI; ++s) { V.ixi[s] = Q.ixi[s].v; V.a_i[s] = Q.a_i[s].v; V.cs[s] = Q.cs[s].v; V.hai[s] = Q.hai[s].v; }
      }
    }
  }
  __syncthreads();
  LineS<NI> L = *Lv;   // (identical in every lane: SGPRs)
  L.wpe2 = uni(L.wpe2); L.wL = uni(L.wL); L.i2wL = uni(L.i2wL); L.kL = uni(L.kL); L.ivTe = uni(L.ivTe);
  L.a_e = uni(L.a_e); L.pref = uni(L.pref); L.Ud = uni(L.Ud); L.Vd = uni(L.Vd);
#pragma unroll
  for (int s = 0; s < NI; ++s) { L.ixi[s] = uni(L.ixi[s]); L.a_i[s] = uni(L.a_i[s]); L.cs[s] = uni(L.cs[s]); L.hai[s] = uni(L.hai[s]); }
  const double cw = -0.5 * L.i2wL * L.i2wL, ipref = 1.0 / L.pref;
  const double* __restrict__ omgs = S.omgs[f];
  // a thread walks pairs of consecutive samples with one chain of base points, as the pair sweeps do: two rows live at a time
  for (int pr = tid; pr < npts / kPair; pr += kThreads) {
    const int j0 = kPair * pr;
    double ws[kPair + 1], ks[kPair + 1];
#pragma unroll
    for (int q = 0; q <= kPair; ++q) { ws[q] = omgs[min(j0 + q, npts - 1)]; ks[q] = ks_eval(ws[q], L.wpe2); }
    LineS<NI> J[kPair];
    KsAcc KA[kPair];
    double xa[kPair];
#pragma unroll
    for (int q = 0; q < kPair; ++q) { zero_lines<NI>(J[q]); xa[q] = 0.0; KA[q].p1a = KA[q].p2a = KA[q].p1b = KA[q].p2b = 0.0; }
    for (int a = 0; a < NA; ++a) {
      const double ct = uni(cosa[a]), wa = uni(wsa[a] * L.pref);
      Base b0;
      base_eval<NI>(ws[0], ks[0], ct, L, T, b0);
#pragma unroll
      for (int q = 0; q < kPair; ++q) {
        Base b1;
        base_eval<NI>(ws[q + 1], ks[q + 1], ct, L, T, b1);
        row_step<NI, 0, false, false>(b0, b1, j0 + q + 1 < npts, L, T, ct, wa, cw, xa[q], J[q], KA[q]);
        b0 = b1;
      }
    }
#pragma unroll
    for (int q = 0; q < kPair; ++q) {
      ks_columns<NI>(KA[q], ks[q], ks[q + 1], L, J[q]);
      const int j = j0 + q;
      const LineS<NI>& R = J[q];
      const double rp = xa[q] * ipref;   // d x_j / d pref = x_j / pref
      xg[j] = xa[q];
      for (int c = 0; c < n; ++c) {
        const double* d = dl + c;
        double t = R.wpe2 * d[0];
        t = __builtin_fma(R.wL, d[n], t); t = __builtin_fma(R.kL, d[2 * n], t); t = __builtin_fma(R.ivTe, d[3 * n], t);
        t = __builtin_fma(R.a_e, d[4 * n], t); t = __builtin_fma(rp, d[5 * n], t); t = __builtin_fma(R.Ud, d[6 * n], t);
        t = __builtin_fma(R.Vd, d[7 * n], t);
#pragma unroll
        for (int s = 0; s < NI; ++s) {
          t = __builtin_fma(R.ixi[s], d[(8 + 3 * s) * n], t);
          t = __builtin_fma(-0.5 * R.a_i[s], d[(9 + 3 * s) * n], t);   // (the deferred factor of point_fused: hai = -a_i / 2)
          t = __builtin_fma(R.cs[s], d[(10 + 3 * s) * n], t);
        }
        xg[(size_t)(1 + c) * npts + j] = t;
      }
    }
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------
// k_jac_sweep: persistent workgroups of 256 threads, one lineout per task, the groups of W leaves one after the other.
// ------------------------------------------------------------------------------------------
// The row form of the sweep (ROWS; 1-2 ion species, one gradient point, no DLM order among the leaves, no raw feature): per (sample,
// angle) the value and the hand-written reverse of the pair-sweep kernels (row_step, k_pairs.inc) leave, per sample, the row
// d x_j / d (lineout scalars) in registers -- about the cost of one forward and one reverse for ALL leaves.  Each row is then
// contracted with the tangents of the lineout scalars w.r.t. the leaves (make_lines_hd on TN<W>, once per lineout and feature) into
// x_j's n tangents, which go to the workgroup's scratch; the groups of W leaves only run the tail (taps, normalisation, amplitudes).

template <int NI, int W, bool ROWS = false>
__global__ __launch_bounds__(kThreads, ((NI == 1 || ROWS) ? 2 : 1)) void k_jac_sweep(KStatic S, KCall K, JacArgs A) {
  using N = TN<W>;
  constexpr int NPk = TSFF_NP(NI);
  constexpr int BPT = TSFF_NBINS / kThreads;
  extern __shared__ __align__(16) unsigned char smem[];
  double2* zp = reinterpret_cast<double2*>(smem);          // [1640] full Z' table
  double* Wt = reinterpret_cast<double*>(zp + kNXi2);      // [1640]
  double2* hc = reinterpret_cast<double2*>(Wt + kNXi2);    // [2 (nvx - 1)] (+ padding)
  double* Wm = reinterpret_cast<double*>(hc + 2 * S.nvx);  // with_m: [1640] dW/dm, [2 nvx] Hermite coefficients of d ln f_e / dm
  double2* hcm = reinterpret_cast<double2*>(Wm + kNXi2);
  double* cosa = A.with_m ? reinterpret_cast<double*>(hcm + 2 * S.nvx) : Wm;
  double* wsa = cosa + S.n_angles;
  double* red = wsa + S.n_angles;                           // [16]
  N* ph = reinterpret_cast<N*>(red + 16);                   // [NP + 1]
  N* Msh = ph + kNP_MAX + 1;                                // the maximum of the binned spectrum
  LineT<N, NI>* Lsh = reinterpret_cast<LineT<N, NI>*>(Msh + 1);   // lineout scalars of the current gradient point
  double* xs = reinterpret_cast<double*>(Msh + 1) + (1 + W) * (9 + 4 * TSFF_MAX_ION);   // [(1 + W)][4][qs]
  const int tid = threadIdx.x;
  const int npts = S.npts, ppp = S.ppp, G = S.G, NA = S.n_angles, n = A.n;
  const int qs = jac_qstride(npts), cs = kStrip * qs;   // (cs: one component of the spectrum)
  constexpr int NF = jac_row_fields(NI);
  double* dl = xs + (1 + W) * cs;                                  // ROWS: [NF][n] tangents of the lineout scalars w.r.t. the leaves
  LineS<NI>* Lv = reinterpret_cast<LineS<NI>*>(dl + jac_row_fields(TSFF_MAX_ION) * n);   // ROWS: the lineout scalars
  double* __restrict__ xg = ROWS ? A.xg + (size_t)blockIdx.x * (1 + n) * npts : nullptr;
  double* __restrict__ rows = A.want_gn ? A.rows + (size_t)blockIdx.x * n * TSFF_NBINS : nullptr;
  for (int i = tid; i < kNXi2; i += kThreads) zp[i] = S.zpf[i];
  for (int i = tid; i < NA; i += kThreads) { cosa[i] = S.cos_sa[i]; wsa[i] = S.w_sa[i] / (double)S.G; }   // (the angle's weight over the gradient points)
  int slot_prev = -1;

  for (int b = blockIdx.x; b < K.B; b += gridDim.x) {
    if (A.skip && A.skip[b] != 0) continue;   // (the same for the whole workgroup)
    const int slot = S.shared_fe ? 0 : b;
    __syncthreads();   // (the previous lineout's readers of the tables are done)
    if (slot != slot_prev) {
      for (int i = tid; i < kNXi2; i += kThreads) Wt[i] = K.W[(size_t)slot * kNXi2 + i];
      for (int i = tid; i < S.nvx - 1; i += kThreads) {
        double2 c01, c23;
        hermite_coeffs(K.ht[(size_t)slot * S.nvx + i], K.ht[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
        hc[2 * i] = c01; hc[2 * i + 1] = c23;
        if (A.with_m) {
          hermite_coeffs(K.htm[(size_t)slot * S.nvx + i], K.htm[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
          hcm[2 * i] = c01; hcm[2 * i + 1] = c23;
        }
      }
      if (A.with_m)
        for (int i = tid; i < kNXi2; i += kThreads) Wm[i] = K.Wm[(size_t)slot * kNXi2 + i];
      slot_prev = slot;
    }
    const Tables T = make_tables(S, zp, Wt, nullptr, hc);
    double lsum[3] = {0.0, 0.0, 0.0};
    bool first_feature = true;

    for (int f = 0; f < 2; ++f) {
      if (!S.load[f] || (!A.want_gn && !A.jac[f])) continue;
      const double* __restrict__ omgs = S.omgs[f];
      const double wA = f == TSFF_FEATURE_ELE ? A.w[1] : A.w[0], wB = f == TSFF_FEATURE_ELE ? A.w[2] : 0.0;
      double e1w[BPT], e2w[BPT];   // want_gn: w l' and w l'' of this thread's bins (zero outside the fitted ranges)

      for (int g0 = 0; g0 < n; g0 += W) {
        __syncthreads();   // (every reader of the previous group's ph and spectrum is done)
        // ---- physical parameters with the group's seeds (stage_phys: activation, Ti tying, fraction renormalisation) ----
        if (tid == 0 && !(ROWS && g0 == 0)) jac_stage_phys<NI, W>(S, K, A, b, g0, ph);
        if constexpr (ROWS) {
          if (g0 == 0) jac_rows_sweep<NI, W>(S, K, A, b, f, T, ph, Lsh, Lv, dl, cosa, wsa, xg);   // (ends behind a barrier, ph with the first group's seeds)
          {  // the group's spectrum and tangents from the scratch, with the factor ws^2 and the notch filter of the electron feature
            const bool filt = f == TSFF_FEATURE_ELE && S.filt;
            for (int j = tid; j < npts; j += kThreads) {
              const double w = omgs[j];
              const double c = filt ? w * w * S.filt[j] : w * w;
              double* x = xs + j;   // (the row form fills by sample: the spectrum lies in sample order)
              x[0] = c * xg[j];
#pragma unroll
              for (int k = 0; k < W; ++k) x[(k + 1) * cs] = g0 + k < n ? c * xg[(size_t)(1 + g0 + k) * npts + j] : 0.0;
            }
          }
          __syncthreads();
        } else {
          for (int i = tid; i < (1 + W) * cs; i += kThreads) xs[i] = 0.0;
          __syncthreads();
          MTabT<N> Mt;
          Mt.on = A.with_m != 0; Mt.Wm = Wm; Mt.Wmm = nullptr; Mt.hcm = hcm; Mt.hcmm = nullptr; Mt.m = ph[TSFF_P_M];

          // ================= sweep over (gradient point, sample, angle) =================
          for (int g = 0; g < G; ++g) {
            if (g > 0) __syncthreads();   // (every reader of the previous gradient point's scalars is done)
            if (tid == 0) make_lines_hd<NI>(ph, S.lam_shift[f], g, G, *Lsh);
            __syncthreads();
            const LineT<N, NI>& L = *Lsh;   // (read from LDS where used: the scalars and their tangents stay out of the registers)
            for (int st = tid; st < npts / kStrip; st += kThreads) {
              const int j0 = kStrip * st;
              for (int a = 0; a < NA; ++a) {
                const double ct = cosa[a];
                const N wa = wsa[a] * L.pref;
                BaseT<N> b0;
                base_hd<NI>(omgs[j0], ct, L, T, Mt, b0);
                for (int q = 0; q < kStrip; ++q) {   // (each thread owns its strip: plain read-modify-write of the LDS spectrum)
                  __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (as in k_hess_pairs: the scalars are re-read per point, not hoisted)
                  const int j = j0 + q;
                  const bool has_next = j + 1 < npts;
                  BaseT<N> b1;
                  base_hd<NI>(omgs[min(j + 1, npts - 1)], ct, L, T, Mt, b1);
                  const N v = wa * point_hd<NI>(b0, b1, has_next, L, T, Mt);
                  double* x = xs + q * qs + st;
                  x[0] += v.v;
#pragma unroll
                  for (int k = 0; k < W; ++k) x[(k + 1) * cs] += v.d[k];
                  b0 = b1;
                }
              }
            }
          }
          __syncthreads();
          {  // the factor ws^2 and the notch filter of the electron feature
            const bool filt = f == TSFF_FEATURE_ELE && S.filt;
            for (int j = tid; j < npts; j += kThreads) {
              const double w = omgs[j];
              const double c = filt ? w * w * S.filt[j] : w * w;
              double* x = xs + jac_at(j, qs);
#pragma unroll
              for (int k = 0; k <= W; ++k) x[k * cs] *= c;
            }
          }
          __syncthreads();
        }
        // ================= IRF taps + bin average, arg-max normalisation, amplitudes =================
        const int nh = S.ntaps[f], toff = S.toff[f];
        const double* __restrict__ taps = S.taps[f];
        N yb[BPT];
        double M = -1.0e300;
        int pstar = 0;
#pragma unroll
        for (int r = 0; r < BPT; ++r) {
          const int pbin = tid + kThreads * r;
          N y = N::of(0.0);
          const int i0 = pbin * ppp + toff;
          const int t0 = max(0, -i0), t1 = min(nh, npts - i0);   // (the taps that fall on samples)
          for (int t = t0; t < t1; ++t) {
            const double gt = taps[t];
            const double* x = xs + (ROWS ? i0 + t : jac_at(i0 + t, qs));
            y.v = __builtin_fma(gt, x[0], y.v);
#pragma unroll
            for (int k = 0; k < W; ++k) y.d[k] = __builtin_fma(gt, x[(k + 1) * cs], y.d[k]);
          }
          yb[r] = y;
          if (r == 0 || y.v > M) { M = y.v; pstar = pbin; }
        }
        block_argmax(M, pstar, red);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BPT; ++r)
          if (tid + kThreads * r == pstar) *Msh = yb[r];
        __syncthreads();
        const bool raw = S.raw[f];
        const N invM = raw ? N::of(1.0) : hd_rcp(*Msh);
        const double amps = raw ? 1.0 : K.amps[f][b];
        const N lam = ph[TSFF_P_LAM];
#pragma unroll
        for (int r = 0; r < BPT; ++r) {
          const int pbin = tid + kThreads * r;
          N Ap;
          if (f == TSFF_FEATURE_ELE) Ap = amps * (S.lam_bin[f][pbin] < lam.v ? ph[TSFF_P_AMP1] : ph[TSFF_P_AMP2]);
          else Ap = raw ? N::of(1.0) : amps * ph[TSFF_P_AMP3];
          const N t = Ap * yb[r] * invM;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            if (g0 + k >= n) continue;
            if (A.want_gn) rows[(size_t)(g0 + k) * TSFF_NBINS + pbin] = t.d[k];
            else if (A.jac[f]) A.jac[f][((size_t)b * n + g0 + k) * TSFF_NBINS + pbin] = t.d[k];
          }
          if (A.want_gn && g0 == 0) {   // the loss and its derivatives w.r.t. the model value, once per feature
            const uint8_t mk = S.mask[f][pbin];
            double e = 0.0, e1 = 0.0, e2 = 0.0;
            const double wb = ((mk & 1) ? wA : 0.0) + ((mk & 2) ? wB : 0.0);
            if (mk & 3) {
              double tv = t.v;
              if (K.noise[f]) tv += K.noise[f][(size_t)b * TSFF_NBINS + pbin];
              jac_loss(S.loss_method, A.fit_denoms != 0, K.data[f][(size_t)b * TSFF_NBINS + pbin], tv, e, e1, e2);
            }
            e1w[r] = wb * e1; e2w[r] = wb * e2;
            if (f == TSFF_FEATURE_ELE) { lsum[1] += (mk & 1) ? e : 0.0; lsum[2] += (mk & 2) ? e : 0.0; }
            else lsum[0] += (mk & 1) ? e : 0.0;
          }
        }
      }
      if (!A.want_gn) continue;
      // ================= gradient and Gauss-Newton matrix of this feature (each thread reads back the rows it wrote) =================
      double* __restrict__ gb = A.grad + (size_t)b * n;
      double* __restrict__ hb = A.gn + (size_t)b * n * n;
      for (int a = 0; a < n; ++a) {
        double ja[BPT], pg = 0.0;
#pragma unroll
        for (int r = 0; r < BPT; ++r) {
          ja[r] = rows[(size_t)a * TSFF_NBINS + tid + kThreads * r];
          pg = __builtin_fma(e1w[r], ja[r], pg);
        }
        pg = block_sum(pg, red);
        if (tid == 0) gb[a] = first_feature ? pg : gb[a] + pg;
        for (int c = a; c < n; ++c) {
          double ph2 = 0.0;
#pragma unroll
          for (int r = 0; r < BPT; ++r) ph2 = __builtin_fma(e2w[r] * ja[r], rows[(size_t)c * TSFF_NBINS + tid + kThreads * r], ph2);
          ph2 = block_sum(ph2, red);
          if (tid == 0) {
            const double h = first_feature ? ph2 : hb[a * n + c] + ph2;
            hb[a * n + c] = h;
            hb[c * n + a] = h;
          }
        }
      }
      first_feature = false;
    }
    if (A.want_gn) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double s = block_sum(lsum[k], red);
        if (tid == 0) K.lpart[(size_t)b * 3 + k] = s;
      }
    }
  }
}
