// k_lm.inc -- one pass of the per-lineout Levenberg-Marquardt fit (tsff_lm_fit): k_lm_step.  After each evaluation of
// k_jac_sweep (want_gn: the per-lineout sums of the loss, its gradient and its Gauss-Newton matrix at the point the fit asked
// for), k_lm_step takes the evaluation into every lineout's state and writes the next point to evaluate into params.  The
// lineouts do not couple: one wavefront owns one lineout, nothing depends on B or on the grid, and there are no atomics.
//
// Bit contract: every operation is the one tsadar_amd/lm.py (the host restatement, lm.step) does, in the same order and in
// double, with nothing fused (the pragma keeps the compiler from contracting a multiply and an add into an FMA; a helper
// carries its own, the pragma's scope being the compound statement it appears in); division and sqrt are the correctly
// rounded IEEE operations.  The scalar part runs identically in every lane of the wavefront.  The Cholesky factorisation of
// A + lam I goes column by column: every lane forms the pivot (the same ordered sum), lane r takes row j + 1 + r of the column
// (an ordered sum of its own); the two substitutions are ordered sums that every lane forms.
//
// State (doubles; lm.py, include/tsff.h): [status int32 x B, padded to a whole double | B records], a record being
// [f, lam, nu, pred, nit, nfev, 0, 0 | x[n] | g[n] | A[n][n]].  The status words double as the skip flags of k_jac_sweep: a
// lineout whose status is not 0 is not evaluated again and nothing of it changes.
constexpr int kLmWaves = 4;      // lineouts per workgroup of k_lm_step
constexpr int kLmRecHdr = 8;     // doubles in front of x in a lineout's record (lm.REC_HDR)
enum { kLmRunning = 0, kLmConvGrad, kLmConvF, kLmSmallStep, kLmStopCount, kLmNoStep, kLmBadStart };

__host__ __device__ constexpr long lm_rec_doubles(int n) { return kLmRecHdr + 2L * n + (long)n * n; }
__host__ __device__ constexpr long lm_rec_offset(int B) { return (B + 1L) / 2; }
__host__ __device__ constexpr long lm_eval_doubles(int n) { return 1L + n + (long)n * n; }   // a lineout's row of eval_hist
__host__ __device__ constexpr long lm_wave_doubles(int n) { return 2L * n * n + 5L * n; }    // LDS of one wavefront: A, L | g, x, y, delta, x_trial

struct LmArgs {   // one tsff_lm_fit call, passed by value
  int n, B, NP;
  int slot[kNP_MAX];                                      // the trained leaves' parameter slots, in ravel order
  double w[3];                                            // weights of S_iaw, S_blue, S_red
  double tau, gtol, ftol, xtol, maxiter, maxfun, lam_max;
};

// the wavefront's lanes see each other's LDS writes
__device__ __forceinline__ void lm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool lm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for a NaN)

// lm.cholesky: the lower factor of A + lam I into Lm, column by column -> every pivot was positive and finite (uniform)
__device__ __forceinline__ bool lm_cholesky(const double* A, double lam, int n, int lane, double* Lm) {
#pragma clang fp contract(off)
  for (int j = 0; j < n; ++j) {
    double s = A[j * n + j] + lam;
    for (int k = 0; k < j; ++k) s = s - Lm[j * n + k] * Lm[j * n + k];
    if (!(s > 0.0 && lm_finite(s))) return false;
    const double d = sqrt(s);
    if (lane == 0) Lm[j * n + j] = d;
    for (int i = j + 1 + lane; i < n; i += 64) {
      double t = A[i * n + j];
      for (int k = 0; k < j; ++k) t = t - Lm[i * n + k] * Lm[j * n + k];
      Lm[i * n + j] = t / d;
    }
    lm_wave_sync();
  }
  return true;
}

// lm.solve: L L^T delta = -g, every lane the same ordered sums (y and delta: each lane reads back what it wrote itself; the
// lanes write the same values)
__device__ __forceinline__ void lm_solve(const double* Lm, const double* g, int n, double* y, double* delta) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; ++i) {
    double t = -g[i];
    for (int k = 0; k < i; ++k) t = t - Lm[i * n + k] * y[k];
    y[i] = t / Lm[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < n; ++k) t = t - Lm[k * n + i] * delta[k];
    delta[i] = t / Lm[i * n + i];
  }
}

__device__ __forceinline__ double lm_norm(const double* v, int n) {
#pragma clang fp contract(off)
  double s = 0.0;
  for (int a = 0; a < n; ++a) s = s + v[a] * v[a];
  return sqrt(s);
}

// lpart [B][3], grad [B][n], gn [B][n][n]: the evaluation (k_jac_sweep with want_gn) at params' active slots; x_hist [B][n] and
// eval_hist [B][1 + n + n n] (either may be null): this evaluation's rows, NaN for a lineout that was terminal already
__global__ __launch_bounds__(kLmWaves * 64) void k_lm_step(LmArgs P, const double* __restrict__ lpart, const double* __restrict__ grad,
                                                            const double* __restrict__ gn, double* __restrict__ params,
                                                            double* __restrict__ state, double* __restrict__ x_hist,
                                                            double* __restrict__ eval_hist) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * kLmWaves + wave, n = P.n, nn = n * n;
  if (b >= P.B) return;   // (the whole wavefront; no workgroup barrier below)
  double* A = reinterpret_cast<double*>(smem) + (size_t)wave * lm_wave_doubles(n);   // [n][n] the accepted matrix
  double* Lm = A + nn;             // [n][n] the factor
  double* g = Lm + nn;             // [n] the accepted gradient
  double* x = g + n;               // [n] the accepted point
  double* y = x + n;               // [n]
  double* delta = y + n;           // [n]
  double* xt = delta + n;          // [n] the point the evaluation ran at
  int32_t* status = reinterpret_cast<int32_t*>(state);
  double* rec = state + lm_rec_offset(P.B) + (size_t)b * lm_rec_doubles(n);
  double* xh = x_hist ? x_hist + (size_t)b * n : nullptr;
  double* eh = eval_hist ? eval_hist + (size_t)b * lm_eval_doubles(n) : nullptr;
  double* xpar = params + (size_t)b * P.NP;
  if (status[b] != kLmRunning) {
    const double nan = __builtin_nan("");
    if (xh) for (int a = lane; a < n; a += 64) xh[a] = nan;
    if (eh) for (int i = lane; i < 1 + n + nn; i += 64) eh[i] = nan;
    return;
  }
  const double* __restrict__ Gb = grad + (size_t)b * n;
  const double* __restrict__ Hb = gn + (size_t)b * nn;
  const double F = (P.w[0] * lpart[(size_t)b * 3] + P.w[1] * lpart[(size_t)b * 3 + 1]) + P.w[2] * lpart[(size_t)b * 3 + 2];
  double f = rec[0], lam = rec[1], nu = rec[2], pred = rec[3], nit = rec[4], nfev = rec[5];
  for (int a = lane; a < n; a += 64) {
    const double v = xpar[P.slot[a]];
    xt[a] = v;
    if (xh) xh[a] = v;
  }
  if (eh) {
    if (lane == 0) eh[0] = F;
    for (int a = lane; a < n; a += 64) eh[1 + a] = Gb[a];
    for (int i = lane; i < nn; i += 64) eh[1 + n + i] = Hb[i];
  }
  // ---- the evaluation into the state (lm.step) ----
  const bool first = nfev == 0.0, finite = lm_finite(F);
  const bool won = !first && finite && pred > 0.0 && F < f;
  const bool take = first || won;
  const double f_old = f;
  nfev = nfev + 1.0;
  if (won) {
    const double rho = (f_old - F) / pred;
    const double t = 2.0 * rho - 1.0;
    const double shrink = 1.0 - t * t * t;
    lam = lam * (shrink > 1.0 / 3.0 ? shrink : 1.0 / 3.0);
    nu = 2.0;
    nit = nit + 1.0;
  } else if (first) {
    double d = Hb[0];
    for (int a = 1; a < n; ++a) {
      const double v = Hb[a * n + a];
      if (v > d) d = v;
    }
    lam = (lm_finite(d) && d > 0.0) ? P.tau * d : P.tau;
    nu = 2.0;
  } else {
    lam = lam * nu;
    nu = 2.0 * nu;
  }
  // the accepted (x, g, A) into LDS: the evaluation's when it is taken (then into the record too), else the record's
  for (int a = lane; a < n; a += 64) {
    if (take) { rec[kLmRecHdr + a] = xt[a]; rec[kLmRecHdr + n + a] = Gb[a]; }
    x[a] = take ? xt[a] : rec[kLmRecHdr + a];
    g[a] = take ? Gb[a] : rec[kLmRecHdr + n + a];
  }
  for (int i = lane; i < nn; i += 64) {
    const double v = take ? Hb[i] : rec[kLmRecHdr + 2 * n + i];
    if (take) rec[kLmRecHdr + 2 * n + i] = v;
    A[i] = v;
  }
  if (take) f = F;
  lm_wave_sync();
  int st = kLmRunning;
  if (first && !finite) st = kLmBadStart;
  if (take && st == kLmRunning) {
    double m = 0.0;
    for (int a = 0; a < n; ++a) {
      const double v = fabs(g[a]);
      if (v > m || v != v) m = v;
    }
    if (m <= P.gtol) st = kLmConvGrad;
  }
  if (won && st == kLmRunning && f_old - F <= P.ftol * f_old) st = kLmConvF;
  if (st == kLmRunning && (nit >= P.maxiter || nfev >= P.maxfun)) st = kLmStopCount;
  // ---- the proposal: a failed factorisation raises the damping and tries again (lam grows by nu = 2, 4, 8, ...: a few
  // dozen rounds take it past any finite lam_max) ----
  bool go = false;
  while (st == kLmRunning) {
    if (!(lam > 0.0 && lam <= P.lam_max)) { st = kLmNoStep; break; }
    if (!lm_cholesky(A, lam, n, lane, Lm)) {
      lam = lam * nu;
      nu = 2.0 * nu;
      lm_wave_sync();   // (the next round's writers of Lm come after this round's readers)
      continue;
    }
    lm_solve(Lm, g, n, y, delta);
    if (lm_norm(delta, n) <= P.xtol * (lm_norm(x, n) + P.xtol)) { st = kLmSmallStep; break; }
    double p = 0.0;
    for (int a = 0; a < n; ++a) p = p + delta[a] * (lam * delta[a] - g[a]);
    pred = 0.5 * p;
    go = true;
    break;
  }
  // ---- the next point to evaluate, or the accepted one of a lineout that has ended ----
  for (int a = lane; a < n; a += 64) xpar[P.slot[a]] = go ? x[a] + delta[a] : x[a];
  if (lane == 0) {
    rec[0] = f; rec[1] = lam; rec[2] = nu; rec[3] = pred; rec[4] = nit; rec[5] = nfev;
    status[b] = st;
  }
}
