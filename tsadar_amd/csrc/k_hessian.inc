// k_hessian.inc -- exact per-lineout Hessian of the fit loss (LossFunction._loss_for_hess_fn_, loss_function.py:170-188):
// k_hess_pairs, k_hess_finish.  Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).
//
// Second-order forward mode with hyper-dual numbers (v, d/da, d/dc, d2/da dc): one task per (lineout, pair of active leaves
// a <= c) evaluates the whole chain -- parameter transform, lineout scalars, every (sample, angle, gradient point), the factor
// ws^2 and the notch filter, IRF taps + binning, arg-max normalisation, amplitudes, loss -- in hyper-dual arithmetic, and
// leaves the three masked sums S_iaw, S_blue, S_red with their first and mixed second derivatives.  k_hess_finish weights
// them into grad[b][a] and the symmetric hess[b][a][c].  DESIGN.md section 4.4.
//
// The chain functions are those of k_fwdmode.inc, written once over the number type: HD here, the value with W first-order tangents
// in k_jacobian.inc (TN<W>).  Table convention: k_fwdmode.inc.

struct HD {   // hyper-dual number: value, the two first derivatives and the mixed second derivative
  double v, a, b, ab;
  static constexpr bool kSecondOrder = true;
  static constexpr int kLanes = 0;   // (no tangent lanes that carry a table direction of their own: MTabT)
  static __device__ __forceinline__ HD of(double c) { return HD{c, 0.0, 0.0, 0.0}; }
};
__device__ __forceinline__ HD hd(double v) { return HD{v, 0.0, 0.0, 0.0}; }
__device__ __forceinline__ HD operator+(HD x, HD y) { return HD{x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab}; }
__device__ __forceinline__ HD operator-(HD x, HD y) { return HD{x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab}; }
__device__ __forceinline__ HD operator-(HD x) { return HD{-x.v, -x.a, -x.b, -x.ab}; }
__device__ __forceinline__ HD operator+(HD x, double c) { return HD{x.v + c, x.a, x.b, x.ab}; }
__device__ __forceinline__ HD operator+(double c, HD x) { return x + c; }
__device__ __forceinline__ HD operator-(HD x, double c) { return HD{x.v - c, x.a, x.b, x.ab}; }
__device__ __forceinline__ HD operator-(double c, HD x) { return HD{c - x.v, -x.a, -x.b, -x.ab}; }
__device__ __forceinline__ HD operator*(HD x, double c) { return HD{x.v * c, x.a * c, x.b * c, x.ab * c}; }
__device__ __forceinline__ HD operator*(double c, HD x) { return x * c; }
__device__ __forceinline__ HD operator*(HD x, HD y) {
  return HD{x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, x.ab * y.v + x.a * y.b + x.b * y.a + x.v * y.ab};
}
// f(x) from f, f', f''
__device__ __forceinline__ HD hd_chain(HD x, double f, double d1, double d2) {
  return HD{f, d1 * x.a, d1 * x.b, d1 * x.ab + d2 * x.a * x.b};
}
// (hd_rcp, hd_sqrt, hd_exp, hd_sigmoid: the generic forms of k_fwdmode.inc)
__device__ __forceinline__ HD operator/(HD x, HD y) { return x * hd_rcp(y); }
__device__ __forceinline__ HD operator/(double c, HD y) { return c * hd_rcp(y); }
// f(x, m) of a table lookup from its partial derivatives (fxx: curvature in x; fxm, fmm: through the m-dependence of the table)
__device__ __forceinline__ HD hd_xm(HD x, HD m, double f, double fx, double fm, double fxx, double fxm, double fmm) {
  return HD{f, fx * x.a + fm * m.a, fx * x.b + fm * m.b,
            fx * x.ab + fm * m.ab + fxx * x.a * x.b + fxm * (x.a * m.b + m.a * x.b) + fmm * m.a * m.b};
}
template <int NI>
using LineHD = LineT<HD, NI>;
using BaseHD = BaseT<HD>;
using MTab = MTabT<HD>;

// the active leaves of one tsff_loss_hess call, passed by value
struct HessArgs {
  int n;                  // number of active leaves
  int npair;              // n (n + 1) / 2
  int slot[kNP_MAX];      // their parameter slots, in ravel order
  int tasks;              // B * npair
  int with_m;             // the DLM order m is an active leaf: the m-derivative tables take part
  const double2* htmm;    // with_m: [slots][nvx] second m-derivative of (ln f_e, node slope)   (k_hess_mtab)
  const double* Wmm;      // with_m: [slots][1640] d2W/dm2                                      (k_wgemm_w on k_hess_mtab's rows)
};

// pair p of the upper triangle, row-major: (0,0), (0,1), ..., (0,n-1), (1,1), ...
__device__ __forceinline__ void hess_pair(int p, int n, int& a, int& c) {
  a = 0;
  while (p >= n - a) { p -= n - a; ++a; }
  c = a + p;
}

// loss functional e(d, t) of one sample with the denominators of _loss_for_hess_fn_ (|d| + 1e-10, l1 / l2) in hyper-dual arithmetic.
// The functional itself is defined in k_chain.inc (loss_point, with the denominator rule in bin_loss); this form evaluates l2 and l1
// as hyper-dual products of r, whose last bit hd_chain on loss_point's derivatives would not reproduce.
__device__ __forceinline__ HD loss_hd(int method, double d, HD t) {
  const HD r = d - t;
  HD e;
  if (method == TSFF_LOSS_L2) e = r * r;
  else if (method == TSFF_LOSS_L1) e = r * (r.v > 0.0 ? 1.0 : (r.v < 0.0 ? -1.0 : 0.0));
  else if (method == TSFF_LOSS_LOGCOSH) { const double th = tanh(r.v); e = hd_chain(r, log(cosh(r.v)), th, 1.0 - th * th); }
  else { const double it = 1.0 / t.v; e = hd_chain(t, t.v - d * log(t.v), 1.0 - d * it, d * it * it); }
  if (method == TSFF_LOSS_L2 || method == TSFF_LOSS_L1) e = e * (1.0 / (fabs(d) + 1e-10));
  return e;
}

__device__ __forceinline__ HD block_sum_hd(HD x, double* red) {
  return HD{block_sum(x.v, red), block_sum(x.a, red), block_sum(x.b, red), block_sum(x.ab, red)};
}

// LDS of one k_hess_pairs workgroup (doubles)
// (with_m: dW/dm, d2W/dm2 and the two Hermite coefficient tables of the m-derivatives of ln f_e)
constexpr int kLineHDDoubles = 4 * (9 + 4 * TSFF_MAX_ION);
__host__ __device__ inline size_t hess_smem_doubles(const KStatic& S, bool with_m) {
  size_t n = 2 * (size_t)kNXi2 + kNXi2 + 4 * (size_t)S.nvx + 2 * (size_t)S.n_angles + 4 * (size_t)(kNP_MAX + 1) + 4 + 16 + kLineHDDoubles;
  if (with_m) n += 2 * (size_t)kNXi2 + 8 * (size_t)S.nvx;
  return n;
}

// ------------------------------------------------------------------------------------------
// k_hess_pairs: persistent workgroups of 256 threads; task t = b * npair + p (lineout b, pair p of active leaves).
// xws: per workgroup 4 * npts doubles of global scratch (the hyper-dual spectrum of one feature).
// out[t][3][4]: (S_iaw, S_blue, S_red) x (value, d/da, d/dc, d2/da dc).
// ------------------------------------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(kThreads) void k_hess_pairs(KStatic S, KCall K, HessArgs A, double* __restrict__ xws,
                                                         double* __restrict__ out) {
  constexpr int NPk = TSFF_NP(NI);
  extern __shared__ __align__(16) unsigned char smem[];
  double2* zp = reinterpret_cast<double2*>(smem);          // [1640] full Z' table
  double* Wt = reinterpret_cast<double*>(zp + kNXi2);      // [1640]
  double2* hc = reinterpret_cast<double2*>(Wt + kNXi2);    // [2 (nvx - 1)] (+ padding)
  double* cosa = reinterpret_cast<double*>(hc + 2 * S.nvx);
  double* wsa = cosa + S.n_angles;
  HD* ph = reinterpret_cast<HD*>(wsa + S.n_angles);         // [NP + 1]
  HD* Msh = ph + kNP_MAX + 1;                               // the maximum of the binned spectrum
  double* red = reinterpret_cast<double*>(Msh + 1);         // [16]
  LineHD<NI>* Lsh = reinterpret_cast<LineHD<NI>*>(red + 16); // lineout scalars of the current gradient point (one copy per workgroup)
  double* Wm = red + 16 + kLineHDDoubles;                    // with_m: [1640] dW/dm, [1640] d2W/dm2, [2 nvx] x 2 Hermite coefficients
  double* Wmm = Wm + kNXi2;
  double2* hcm = reinterpret_cast<double2*>(Wmm + kNXi2);
  double2* hcmm = hcm + 2 * S.nvx;
  const int tid = threadIdx.x;
  const int npts = S.npts, ppp = S.ppp, G = S.G, NA = S.n_angles;
  double* __restrict__ x0 = xws + (size_t)blockIdx.x * 4 * npts;
  double* __restrict__ x1 = x0 + npts;
  double* __restrict__ x2 = x1 + npts;
  double* __restrict__ x3 = x2 + npts;
  for (int i = tid; i < kNXi2; i += kThreads) zp[i] = S.zpf[i];
  for (int i = tid; i < NA; i += kThreads) { cosa[i] = S.cos_sa[i]; wsa[i] = S.w_sa[i]; }
  int slot_prev = -1;

  for (int task = blockIdx.x; task < A.tasks; task += gridDim.x) {
    const int b = task / A.npair, p = task - b * A.npair;
    int ia, ic;
    hess_pair(p, A.n, ia, ic);
    const int sa = A.slot[ia], sc = A.slot[ic];
    const int slot = S.shared_fe ? 0 : b;
    __syncthreads();   // (the previous task's readers of the tables and of ph are done)
    if (slot != slot_prev) {
      for (int i = tid; i < kNXi2; i += kThreads) Wt[i] = K.W[(size_t)slot * kNXi2 + i];
      for (int i = tid; i < S.nvx - 1; i += kThreads) {
        double2 c01, c23;
        hermite_coeffs(K.ht[(size_t)slot * S.nvx + i], K.ht[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
        hc[2 * i] = c01; hc[2 * i + 1] = c23;
        if (A.with_m) {
          hermite_coeffs(K.htm[(size_t)slot * S.nvx + i], K.htm[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
          hcm[2 * i] = c01; hcm[2 * i + 1] = c23;
          hermite_coeffs(A.htmm[(size_t)slot * S.nvx + i], A.htmm[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
          hcmm[2 * i] = c01; hcmm[2 * i + 1] = c23;
        }
      }
      if (A.with_m)
        for (int i = tid; i < kNXi2; i += kThreads) { Wm[i] = K.Wm[(size_t)slot * kNXi2 + i]; Wmm[i] = A.Wmm[(size_t)slot * kNXi2 + i]; }
      slot_prev = slot;
    }
    // ---- physical parameters with the two seeds (stage_phys: activation, Ti tying, fraction renormalisation) ----
    if (tid == 0) {
      const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
      for (int s = 0; s < NPk; ++s) {
        HD v = HD{xpar[s], s == sa ? 1.0 : 0.0, s == sc ? 1.0 : 0.0, 0.0};
        if (S.p_sig[s]) v = hd_sigmoid(v);
        ph[s] = v * S.p_scale[s] + S.p_shift[s];
      }
      tie_and_renorm<NI>(S, ph);
    }
    __syncthreads();
    const Tables T = make_tables(S, zp, Wt, nullptr, hc);
    MTab Mt;
    Mt.on = A.with_m != 0; Mt.Wm = Wm; Mt.Wmm = Wmm; Mt.hcm = hcm; Mt.hcmm = hcmm; Mt.m = ph[TSFF_P_M];
    HD sums[3] = {hd(0.0), hd(0.0), hd(0.0)};

    for (int f = 0; f < 2; ++f) {
      if (!S.load[f]) continue;
      const double* __restrict__ omgs = S.omgs[f];
      // ================= sweep over (gradient point, sample, angle) =================
      for (int j = tid; j < npts; j += kThreads) { x0[j] = 0.0; x1[j] = 0.0; x2[j] = 0.0; x3[j] = 0.0; }
      __syncthreads();
      for (int g = 0; g < G; ++g) {
        if (g > 0) __syncthreads();   // (every reader of the previous gradient point's scalars is done)
        if (tid == 0) make_lines_hd<NI>(ph, S.lam_shift[f], g, G, *Lsh);
        __syncthreads();
        const LineHD<NI>& L = *Lsh;   // (read from LDS where used: the hyper-dual scalars stay out of the registers)
        for (int st = tid; st < npts / kStrip; st += kThreads) {
          const int j0 = kStrip * st;
          for (int a = 0; a < NA; ++a) {
            const double ct = cosa[a];
            const HD wa = (wsa[a] / (double)G) * L.pref;
            BaseHD b0;
            base_hd<NI>(omgs[j0], ct, L, T, Mt, b0);
            for (int q = 0; q < kStrip; ++q) {   // (each thread owns its strip: plain read-modify-write of the scratch spectrum)
              // (a compiler-only fence: the lineout scalars are re-read from LDS per point instead of being hoisted into
              //  registers for the whole strip -- with 3-4 ion species they alone would take 200 VGPRs and push the loop into scratch)
              __atomic_signal_fence(__ATOMIC_SEQ_CST);
              const int j = j0 + q;
              const bool has_next = j + 1 < npts;
              BaseHD b1;
              base_hd<NI>(omgs[min(j + 1, npts - 1)], ct, L, T, Mt, b1);
              const HD v = wa * point_hd<NI>(b0, b1, has_next, L, T, Mt);
              x0[j] += v.v; x1[j] += v.a; x2[j] += v.b; x3[j] += v.ab;
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
          x0[j] *= c; x1[j] *= c; x2[j] *= c; x3[j] *= c;
        }
      }
      __syncthreads();
      // ================= IRF taps + bin average, arg-max normalisation, amplitudes, loss =================
      constexpr int BPT = TSFF_NBINS / kThreads;
      const int nh = S.ntaps[f], toff = S.toff[f];
      const double* __restrict__ taps = S.taps[f];
      HD yb[BPT];
      double M = -1.0e300;
      int pstar = 0;
#pragma unroll
      for (int r = 0; r < BPT; ++r) {
        const int pbin = tid + kThreads * r;
        HD y = hd(0.0);
        const int i0 = pbin * ppp + toff;
        for (int t = 0; t < nh; ++t) {
          const int i = i0 + t;
          if (i < 0 || i >= npts) continue;
          const double gt = taps[t];
          y = y + HD{gt * x0[i], gt * x1[i], gt * x2[i], gt * x3[i]};
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
      const HD invM = raw ? hd(1.0) : hd_rcp(*Msh);
      const double amps = raw ? 1.0 : K.amps[f][b];
      const HD lam = ph[TSFF_P_LAM];
      HD s0 = hd(0.0), s1 = hd(0.0);
#pragma unroll
      for (int r = 0; r < BPT; ++r) {
        const int pbin = tid + kThreads * r;
        const uint8_t mk = S.mask[f][pbin];
        if (!(mk & 3)) continue;
        HD Ap;
        if (f == TSFF_FEATURE_ELE) Ap = amps * (S.lam_bin[f][pbin] < lam.v ? ph[TSFF_P_AMP1] : ph[TSFF_P_AMP2]);
        else Ap = raw ? hd(1.0) : amps * ph[TSFF_P_AMP3];
        HD t = Ap * yb[r] * invM;
        if (K.noise[f]) t = t + K.noise[f][(size_t)b * TSFF_NBINS + pbin];
        const HD e = loss_hd(S.loss_method, K.data[f][(size_t)b * TSFF_NBINS + pbin], t);
        if (mk & 1) s0 = s0 + e;
        if (mk & 2) s1 = s1 + e;
      }
      s0 = block_sum_hd(s0, red);
      s1 = block_sum_hd(s1, red);
      if (f == TSFF_FEATURE_ELE) { sums[1] = s0; sums[2] = s1; }
      else sums[0] = s0;
      __syncthreads();   // (the next feature overwrites the scratch spectrum)
    }
    if (tid == 0) {
      double* o = out + (size_t)task * 12;
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[4 * k] = sums[k].v; o[4 * k + 1] = sums[k].a; o[4 * k + 2] = sums[k].b; o[4 * k + 3] = sums[k].ab; }
    }
  }
}

// k_hess_finish: one thread per lineout.  grad[b][a] = sum_k w_k dS_k/da (pair (a, a)), hess[b][a][c] = hess[b][c][a] =
// sum_k w_k d2S_k/da dc, lpart[b][k] = S_k (the value of pair 0; every pair carries the same value).
__global__ __launch_bounds__(kThreads) void k_hess_finish(const double* __restrict__ tout, HessArgs A, int B, double w0, double w1,
                                                          double w2, double* __restrict__ lpart, double* __restrict__ grad,
                                                          double* __restrict__ hess) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= B) return;
  const int n = A.n;
  const double* __restrict__ t = tout + (size_t)b * A.npair * 12;
  for (int k = 0; k < 3; ++k) lpart[(size_t)b * 3 + k] = t[4 * k];
  int p = 0;
  for (int a = 0; a < n; ++a)
    for (int c = a; c < n; ++c, ++p) {
      const double* o = t + (size_t)p * 12;
      const double h = (w0 * o[3] + w1 * o[7]) + w2 * o[11];
      hess[((size_t)b * n + a) * n + c] = h;
      hess[((size_t)b * n + c) * n + a] = h;
      if (c == a) grad[(size_t)b * n + a] = (w0 * o[1] + w1 * o[5]) + w2 * o[9];
    }
}

// k_hess_mtab: the second m-derivatives of the per-lineout DLM tables (fe_mode DLM, m an active leaf).  grid B, 256 threads.
// DLM1V (base.py:277-294) is linear in m inside a cell of the m axis and then divided by its own sum, so with
// f_i = a_i + t(m) d_i:  d2 ln f_i / dm2 = (sum d / sum f)^2 t'^2 - (d_i / f_i)^2 t'^2  (zero outside [2, 5], where the
// interpolation clamps).  Outputs: htmm [B][nvx] = (d2 ln f_e / dm2, its node slope), and the rows of the W-table GEMM for
// d2W/dm2 in k_fe_vectors' layout, X [B][4][1024] = (A'', s'', 0, 0), cst [B][2] = (sum fdif'', 0), from
// ratmod'' = ratmod (H_m^2 + H_mm) at the xi1 nodes (H = ln f_e interpolated; H_m, H_mm the Hermite interpolants of the
// tangent tables).  A shipped k_wgemm_w launch turns the rows into d2W/dm2 (W is linear in ratdf, DESIGN section 4.2).
template <int NI>
__global__ __launch_bounds__(kThreads) void k_hess_mtab(KStatic S, const double* __restrict__ params, const double2* __restrict__ ht,
                                                        const double2* __restrict__ htm, double2* __restrict__ htmm_out,
                                                        double* __restrict__ X, double* __restrict__ cst) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* hc = reinterpret_cast<double2*>(smem);   // [2 nvx] x 3: coefficients of ln f_e, d/dm, d2/dm2
  double2* hcm = hc + 2 * S.nvx;
  double2* hcmm = hcm + 2 * S.nvx;
  double* lmm = reinterpret_cast<double*>(hcmm + 2 * S.nvx);   // [nvx]
  double* rat = lmm + S.nvx;                                   // [1024] ratmod''
  double* rdf = rat + kNXi1;                                   // [1024] ratdf''
  double* red = rdf + kNXi1;                                   // [8]
  const int b = blockIdx.x, tid = threadIdx.x, nvx = S.nvx;
  const DlmCell cell = dlm_cell<NI>(S, params + (size_t)b * S.NP);
  double part = 0.0, dpart = 0.0;
  for (int i = tid; i < nvx; i += kThreads) {
    double f, df;
    dlm_node(S, cell, i, f, df);
    part += f;
    dpart += df;
  }
  const double tot = block_sum(part, red);
  const double dtot = block_sum(dpart, red);
  const double rt = dtot / tot;
  for (int i = tid; i < nvx; i += kThreads) {
    double f, df;
    dlm_node(S, cell, i, f, df);
    const double q = df / f;   // (df = 0 outside the m axis)
    lmm[i] = rt * rt - q * q;
  }
  __syncthreads();
  double2* htmm_b = htmm_out + (size_t)b * nvx;
  for (int i = tid; i < nvx; i += kThreads) htmm_b[i] = make_double2(lmm[i], node_slopes(lmm, i, nvx, S.dv));
  __syncthreads();
  const double2* ht_b = ht + (size_t)b * nvx;
  const double2* htm_b = htm + (size_t)b * nvx;
  for (int i = tid; i < nvx - 1; i += kThreads) {
    hermite_coeffs(ht_b[i], ht_b[i + 1], S.dv, hc[2 * i], hc[2 * i + 1]);
    hermite_coeffs(htm_b[i], htm_b[i + 1], S.dv, hcm[2 * i], hcm[2 * i + 1]);
    hermite_coeffs(htmm_b[i], htmm_b[i + 1], S.dv, hcmm[2 * i], hcmm[2 * i + 1]);
  }
  __syncthreads();
  const Tables T = make_tables(S, nullptr, nullptr, nullptr, hc);
  Tables Tm = T, Tmm = T;
  Tm.hc = hcm; Tmm.hc = hcmm;
  for (int i = tid; i < kNXi1; i += kThreads) {
    const double x = S.xi1[i];
    double H, dH, Hm, dHm, Hmm, dHmm;
    hermite_lookup_c(T, x, H, dH);
    hermite_lookup_c(Tm, x, Hm, dHm);
    hermite_lookup_c(Tmm, x, Hmm, dHmm);
    const bool out = x < T.vx0 || x > T.vxlast;
    rat[i] = out ? 0.0 : exp(H) * (Hm * Hm + Hmm);
  }
  __syncthreads();
  ratdf_central(S.xi1, rat, rdf);
  __syncthreads();
  double* Xb = X + (size_t)b * 4 * kNXi1;
  double c0 = ratdf_rows(S.xi1, rdf, Xb, Xb + kNXi1);
  for (int i = tid; i < kNXi1; i += kThreads) { Xb[2 * kNXi1 + i] = 0.0; Xb[3 * kNXi1 + i] = 0.0; }
  c0 = block_sum(c0, red);
  if (tid == 0) { cst[2 * b] = c0; cst[2 * b + 1] = 0.0; }
}
