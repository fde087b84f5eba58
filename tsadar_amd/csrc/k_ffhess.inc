// k_ffhess.inc -- second-order forward mode of the raw 1-D form factor (tsff_angular_loss_hess): k_ffhess.  Part of the single
// translation unit tsff_kernels.hip (included inside namespace tsff, after k_ffjvp.inc).
//
// P2[q] = d2 P / dx_a dx_c for the pair q = (a, c), a <= c, of the fitted NORMALISED leaves that reach the form factor (every slot but
// the three amplitudes): the per-point sweep of k_ffjvp -- make_lines_hd, base_hd, point_hd of k_fwdmode.inc, strips along the
// wavelength, the angles spread over blockIdx.y -- on the hyper-dual number HD of k_hessian.inc.  The leaves are staged as
// k_hess_pairs stages them (normalised parameters, activation, tie_and_renorm, all in HD with the two seeds at the slots of a and
// c), so the second derivative of the sigmoid, of a tied Ti and of the fraction renormalisation comes from the chain itself (the
// tie's is not reached by a test of this kernel: the electron feature does not feel an ion temperature measurably).  With
// the DLM order a leaf the MTabT<HD> tables (Wm, Wmm, hcm, hcmm) take part as in k_hess_pairs.
//
// One plasma condition (the ARTS image: B = 1).  Grid (pairs, angle chunks): a pair per blockIdx.x, not a persistent loop -- every
// pair costs the same sweep and stages the same tables, a handful of pairs times the angle chunks already fills the device, and
// nothing is carried from one pair to the next.  The diagonal pair (a, a) also leaves the first derivative P1[a] (its d/da
// component), so the first-order images need no pass of their own.  Every output element is written by exactly one thread: no
// atomics, two calls are bit-identical.  DESIGN.md section 4.4c.3.
//
// Table convention: that of k_fwdmode.inc (Z' and W carry their slope and no curvature, the Hermite ln f_e lookup its true
// derivatives, the DLM table piecewise linear in m before its normalisation).

// one launch of k_ffhess, passed by value
struct FfhessArgs {
  int nf;                 // fitted leaves that reach the form factor
  int npair;              // nf (nf + 1) / 2: pairs in hess_pair's order over those leaves
  int slot[kNP_MAX];      // their parameter slots, in ravel order
  int with_m;             // the DLM order m is one of them: the m-derivative tables take part
  const double2* htmm;    // with_m: [nvx] second m-derivative of (ln f_e, node slope)   (k_hess_mtab)
  const double* Wmm;      // with_m: [1640] d2W/dm2                                      (k_wgemm_w on k_hess_mtab's rows)
  double* P1;             // [nf][G][npts][NA] first derivatives
  double* P2;             // [npair][G][npts][NA] mixed second derivatives
};

// LDS of one k_ffhess workgroup (doubles): Z', W, the Hermite coefficients, the angles (an even count: what follows holds double2),
// the hyper-dual parameters and lineout scalars; with_m: dW/dm, d2W/dm2 and the two Hermite coefficient tables of the m-derivatives
__host__ __device__ inline size_t ffhess_smem_doubles(const KStatic& S, bool with_m) {
  size_t n = 2 * (size_t)kNXi2 + kNXi2 + 4 * (size_t)S.nvx + (((size_t)S.n_angles + 1) & ~(size_t)1) + 4 * (size_t)(kNP_MAX + 1) + kLineHDDoubles;
  if (with_m) n += 2 * (size_t)kNXi2 + 8 * (size_t)S.nvx;
  return n;
}

template <int NI>
__global__ __launch_bounds__(kThreads) void k_ffhess(KStatic S, KCall K, FfhessArgs A, int f, const double* __restrict__ omgs, int npts) {
  constexpr int NPk = TSFF_NP(NI);
  extern __shared__ __align__(16) unsigned char smem[];
  double2* zp = reinterpret_cast<double2*>(smem);          // [1640] full Z' table
  double* Wt = reinterpret_cast<double*>(zp + kNXi2);      // [1640]
  double2* hc = reinterpret_cast<double2*>(Wt + kNXi2);    // [2 (nvx - 1)] (+ padding)
  double* cosa = reinterpret_cast<double*>(hc + 2 * S.nvx);
  HD* ph = reinterpret_cast<HD*>(cosa + ((S.n_angles + 1) & ~1));   // [NP + 1]
  LineHD<NI>* Lsh = reinterpret_cast<LineHD<NI>*>(ph + kNP_MAX + 1);   // lineout scalars of the current gradient point
  double* Wm = reinterpret_cast<double*>(ph + kNP_MAX + 1) + kLineHDDoubles;   // with_m: [1640] dW/dm, [1640] d2W/dm2, [2 nvx] x 2 coefficients
  double* Wmm = Wm + kNXi2;
  double2* hcm = reinterpret_cast<double2*>(Wmm + kNXi2);
  double2* hcmm = hcm + 2 * S.nvx;
  const int tid = threadIdx.x, q = blockIdx.x;
  const int G = S.G, NA = S.n_angles, nvx = S.nvx;
  int ia, ic;
  hess_pair(q, A.nf, ia, ic);
  const int sa = A.slot[ia], sc = A.slot[ic];
  for (int i = tid; i < kNXi2; i += kThreads) { zp[i] = S.zpf[i]; Wt[i] = K.W[i]; }
  for (int i = tid; i < NA; i += kThreads) cosa[i] = S.cos_sa[i];
  for (int i = tid; i < nvx - 1; i += kThreads) {
    double2 c01, c23;
    hermite_coeffs(K.ht[i], K.ht[i + 1], S.dv, c01, c23);
    hc[2 * i] = c01; hc[2 * i + 1] = c23;
    if (A.with_m) {
      hermite_coeffs(K.htm[i], K.htm[i + 1], S.dv, c01, c23);
      hcm[2 * i] = c01; hcm[2 * i + 1] = c23;
      hermite_coeffs(A.htmm[i], A.htmm[i + 1], S.dv, c01, c23);
      hcmm[2 * i] = c01; hcmm[2 * i + 1] = c23;
    }
  }
  if (A.with_m)
    for (int i = tid; i < kNXi2; i += kThreads) { Wm[i] = K.Wm[i]; Wmm[i] = A.Wmm[i]; }
  // ---- physical parameters with the two seeds (stage_phys: activation, Ti tying, fraction renormalisation) ----
  if (tid == 0) {
    const double* __restrict__ xpar = K.params;
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
  const size_t img = (size_t)G * npts * NA;   // one image of P
  const int nstrips = (npts + kStrip - 1) / kStrip;

  for (int g = 0; g < G; ++g) {
    if (g > 0) __syncthreads();   // (every reader of the previous gradient point's scalars is done)
    if (tid == 0) make_lines_hd<NI>(ph, S.lam_shift[f], g, G, *Lsh);
    __syncthreads();
    const LineHD<NI>& L = *Lsh;   // (read from LDS where used, as in k_hess_pairs: the hyper-dual scalars stay out of the registers)
    double* __restrict__ o2 = A.P2 + (size_t)q * img + (size_t)g * npts * NA;
    double* __restrict__ o1 = ia == ic ? A.P1 + (size_t)ia * img + (size_t)g * npts * NA : nullptr;
    for (int st = tid; st < nstrips; st += kThreads) {
      const int j0 = kStrip * st;
      for (int a = blockIdx.y; a < NA; a += gridDim.y) {   // (one plasma condition, many angles: the angles are spread over blockIdx.y)
        const double ct = cosa[a];
        BaseHD b0;
        base_hd<NI>(omgs[min(j0, npts - 1)], ct, L, T, Mt, b0);
        for (int r = 0; r < kStrip; ++r) {
          __atomic_signal_fence(__ATOMIC_SEQ_CST);   // (as in k_hess_pairs: the scalars are re-read per point, not hoisted)
          const int j = j0 + r;
          if (j >= npts) break;
          const bool has_next = j + 1 < npts;
          const double ws = omgs[j];
          BaseHD b1;
          base_hd<NI>(omgs[min(j + 1, npts - 1)], ct, L, T, Mt, b1);
          const HD v = point_hd<NI>(b0, b1, has_next, L, T, Mt) * L.pref * (ws * ws);
          o2[(size_t)j * NA + a] = v.ab;
          if (o1) o1[(size_t)j * NA + a] = v.a;
          b0 = b1;
        }
      }
    }
  }
}

// k_ats_hess_reduce: the loss of _loss_for_hess_fn_ on the ARTS image t = E + noise_e with its gradient, exact Hessian and
// Gauss-Newton part, from the image E [rows][nJ], its first derivatives E1 [n][rows][nJ] and second derivatives E2 [n (n + 1) / 2]
// [rows][nJ] (hess_pair's order):
//   hess[a][c] = sum_j w_j (l''(d_j, t_j) t_a t_c + l'(d_j, t_j) t_ac),   gn[a][c] = sum_j w_j l''(d_j, t_j) t_a t_c,
//   grad[a] = sum_j w_j l'(d_j, t_j) t_a,   loss = sum_j w_j l(d_j, t_j),
// w_j = wcol[column of j], l the functional of loss_hd (denominators |d| + 1e-10 for l2 and l1).  One workgroup per pair walks the
// image in a fixed order (thread-strided, then block_sum): no atomics, two calls are bit-identical.  Both triangles of hess and gn
// are written; the diagonal pairs write grad, pair 0 the loss.  (Here and not in k_ats.inc: loss_hd is k_hessian.inc's.)
__global__ __launch_bounds__(kThreads) void k_ats_hess_reduce(const double* __restrict__ E, const double* __restrict__ E1,
                                                              const double* __restrict__ E2, const double* __restrict__ noise,
                                                              const double* __restrict__ data, const double* __restrict__ wcol, int rows,
                                                              int nJ, int method, int n, double* __restrict__ loss,
                                                              double* __restrict__ grad, double* __restrict__ hess, double* __restrict__ gn) {
  __shared__ double red[16];
  const int p = blockIdx.x;
  int a, c;
  hess_pair(p, n, a, c);
  const long img = (long)rows * nJ;
  const double* __restrict__ Ea = E1 + (size_t)a * img;
  const double* __restrict__ Ec = E1 + (size_t)c * img;
  const double* __restrict__ Eac = E2 + (size_t)p * img;
  double sl = 0.0, sg = 0.0, sh = 0.0, sn = 0.0;
  for (long i = threadIdx.x; i < img; i += kThreads) {
    const double w = wcol[i % nJ];
    if (w == 0.0) continue;   // (a column outside the fit ranges: poisson's log of such a sample is not asked for)
    const double t = E[i] + (noise ? noise[i] : 0.0), d = data[i];
    const HD e = loss_hd(method, d, HD{t, Ea[i], Ec[i], Eac[i]});
    const HD e0 = loss_hd(method, d, HD{t, Ea[i], Ec[i], 0.0});
    sl += w * e.v; sg += w * e.a; sh += w * e.ab; sn += w * e0.ab;
  }
  sl = block_sum(sl, red);
  sg = block_sum(sg, red);
  sh = block_sum(sh, red);
  sn = block_sum(sn, red);
  if (threadIdx.x == 0) {
    hess[(size_t)a * n + c] = sh; hess[(size_t)c * n + a] = sh;
    gn[(size_t)a * n + c] = sn; gn[(size_t)c * n + a] = sn;
    if (a == c) grad[a] = sg;
    if (p == 0) *loss = sl;
  }
}
