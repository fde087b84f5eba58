// k_lbfgs.inc -- unbounded L-BFGS-B on the packed buffer of tsff_loss_grad_packed (the reference's default 1-D loop,
// _1d_scipy_loop_, inverse/loops.py:20-56: scipy.optimize.minimize(method="L-BFGS-B", jac=True) with bounds=None), so that a
// whole fit is enqueued at once (tsff_lbfgs_fit).  After each evaluation of f and g at the point the optimiser asked for,
// tsff_lbfgs_fit enqueues a fixed number of launches of k_lbfgs_step (kLbPasses(maxcor)); each launch is one pass of the
// optimiser's state machine -- a reduction of the previous pass's partial sums, the scalar logic, one sweep over the vectors --
// and the passes an evaluation does not need (a line-search trial needs two) return at once.  The state lives in the
// caller's buffer.  Many workgroups share each sweep; the kernel boundary between passes is the only grid-wide seam.
//
// Bit contract: every operation is the one tsadar_amd/lbfgs.py (the host restatement) does, in the same order and in double,
// with nothing fused (the pragma keeps the compiler from contracting a multiply and an add into an FMA); division and sqrt are
// the correctly rounded IEEE operations.  Inner products use one fixed two-level order (lbfgs.dot): with G = lb_blocks(n)
// workgroups of kLbThreads threads, global thread t = blockIdx * kLbThreads + threadIdx accumulates p_t, p_{t+NT}, ...
// sequentially from 0 (NT = G kLbThreads); each workgroup reduces its kLbThreads partials by the halving tree a[i] + a[i + h]
// (LDS for h >= 64, wave-0 shuffles below) into one partial per workgroup; the next pass reduces the G workgroup partials by
// the same halving tree (every workgroup redundantly, so all see the same value).  A thread owns the same elements in every
// pass, so a pass can update a vector and accumulate the next inner product over the updated values without changing any bit.
// The scalar part (the More-Thuente line search, the stopping tests) runs identically in every thread.
//
// Launch k of an evaluation reads the header hdr[k & 1] and the partials part[k & 1] and writes hdr[(k + 1) & 1] (workgroup 0)
// and part[(k + 1) & 1], so no workgroup reads what another one of the same launch writes; kLbPasses is even, so every
// evaluation starts from hdr[0].
//
// State buffer (doubles): [hdr[0], hdr[1]: 2 x kLbHdr | s'y of the ring: maxcor | alphas: maxcor | part[2][2][kLbMaxBlocks] |
// pad to 8 | x0 | g0 | d | q | S ring: maxcor x n | Y ring: maxcor x n], n = n_active x B in ravel order (trained leaf
// outermost, lineout innermost -- the packed gradient's order).  All zeros is the start: the first evaluation is at x0 = params.
constexpr int kLbThreads = 256;
constexpr int kLbMaxBlocks = 64;
constexpr int kLbHdr = 32;      // doubles reserved for one LbHdr
constexpr int kLbMaxCor = 64;
enum { kLbRunning = 0, kLbConvGrad = 1, kLbConvF = 2, kLbStopIter = 3, kLbStopFun = 4, kLbAbnormal = 5 };
// the pass a launch runs (launch 0 of every evaluation takes the evaluation)
enum { kPcIdle = 0, kPcDecide, kPcStore, kPcTlA, kPcTlB, kPcTlC, kPcTlD, kPcLsStart };

struct LbHdr {
  int32_t status, started, nit, nfev, nskip, col, head, ifun;
  int32_t brackt, stage, pc, pk;   // pk: the pair index of the two-loop pass
  double f0, gd0, stp, gamma;      // f and g'd at the line search's start (the last accepted iterate), trial step, H0 scale
  double finit, ginit, gtest, width, width1, stx, fx, gx, sty, fy, gy, stmin, stmax;   // dcsrch
  double gdn;                      // g'd at the accepted trial (the pair's s'y)
};
static_assert(sizeof(LbHdr) <= kLbHdr * sizeof(double), "LbHdr outgrew its reserve");
static_assert(offsetof(LbHdr, f0) == 6 * sizeof(double), "tsadar_amd.lbfgs.HDR_F0 reads f0 at double 6");

// member-wise copies (a whole-struct copy leaves the header in scratch memory)
#define TSFF_LB_FIELDS(X) X(status) X(started) X(nit) X(nfev) X(nskip) X(col) X(head) X(ifun) X(brackt) X(stage) X(pc) X(pk) \
  X(f0) X(gd0) X(stp) X(gamma) X(finit) X(ginit) X(gtest) X(width) X(width1) X(stx) X(fx) X(gx) X(sty) X(fy) X(gy) X(stmin)  \
  X(stmax) X(gdn)
__device__ __forceinline__ void lb_copy(LbHdr& dst, const LbHdr& src) {
#define TSFF_LB_COPY(f) dst.f = src.f;
  TSFF_LB_FIELDS(TSFF_LB_COPY)
#undef TSFF_LB_COPY
}

// workgroups of a fit over n unknowns (lbfgs.blocks): the power of two >= n / 512, at most kLbMaxBlocks
__host__ __device__ inline int lb_blocks(long n) {
  const long want = (n + 511) / 512;
  int g = 1;
  while (g < want && g < kLbMaxBlocks) g <<= 1;
  return g;
}
__host__ __device__ constexpr int lb_passes(int maxcor) { return 2 * maxcor + 6; }   // launches per evaluation (even)
__host__ __device__ constexpr long lb_part_offset(int maxcor) { return 2L * kLbHdr + 2L * maxcor; }
__host__ __device__ constexpr long lb_vec_offset(int maxcor) { return (lb_part_offset(maxcor) + 4L * kLbMaxBlocks + 7) & ~7L; }

__device__ inline double lb_min(double a, double b) { return b < a ? b : a; }   // Python's min / max of two
__device__ inline double lb_max(double a, double b) { return b > a ? b : a; }
__device__ inline double lb_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ inline double lb_maxc(double m, double a) { return (a > m || a != a) ? a : m; }   // a NaN propagates

// the workgroup's halving tree over one value per thread -> the workgroup's partial (valid in thread 0)
template <bool MAX>
__device__ __forceinline__ double lb_wg_reduce(double v, double* red) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int h = kLbThreads / 2; h >= 64; h >>= 1) {
    if (t < h) red[t] = MAX ? lb_maxc(red[t], red[t + h]) : red[t] + red[t + h];
    __syncthreads();
  }
  double x = 0.0;
  if (t < 64) {
    x = red[t];
    for (int h = 32; h >= 1; h >>= 1) {   // lane i < h: a[i] + a[i + h]
      const double y = __shfl_down(x, h, 64);
      x = MAX ? lb_maxc(x, y) : x + y;
    }
  }
  __syncthreads();
  return x;
}

// the halving tree over the G workgroup partials of the previous pass, returned to every thread
template <bool MAX>
__device__ __forceinline__ double lb_grid_total(const double* part, int G, double* bcast) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t < 64) {
    double x = t < G ? part[t] : 0.0;
    for (int h = G / 2; h >= 1; h >>= 1) {
      const double y = __shfl_down(x, h, 64);
      x = MAX ? lb_maxc(x, y) : x + y;
    }
    if (t == 0) *bcast = x;
  }
  __syncthreads();
  const double r = *bcast;
  __syncthreads();
  return r;
}

// MINPACK-2 dcstep (lbfgs.dcstep)
__device__ __forceinline__ void lb_dcstep(double& stx, double& fx, double& dx, double& sty, double& fy, double& dy, double& stp, double fp, double dp,
                          int& brackt, double stpmin, double stpmax) {
#pragma clang fp contract(off)
  const bool opp = (dp > 0.0 && dx < 0.0) || (dp < 0.0 && dx > 0.0);
  double stpf;
  if (fp > fx) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = lb_max(lb_max(fabs(theta), fabs(dx)), fabs(dp));
    double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp < stx) gamma = -gamma;
    const double p = (gamma - dx) + theta;
    const double q = ((gamma - dx) + gamma) + dp;
    const double r = p / q;
    const double stpc = stx + r * (stp - stx);
    const double stpq = stx + ((dx / ((fx - fp) / (stp - stx) + dx)) / 2.0) * (stp - stx);
    stpf = fabs(stpc - stx) <= fabs(stpq - stx) ? stpc : stpc + (stpq - stpc) / 2.0;
    brackt = 1;
  } else if (opp) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = lb_max(lb_max(fabs(theta), fabs(dx)), fabs(dp));
    double gamma = s * sqrt((theta / s) * (theta / s) - (dx / s) * (dp / s));
    if (stp > stx) gamma = -gamma;
    const double p = (gamma - dp) + theta;
    const double q = ((gamma - dp) + gamma) + dx;
    const double r = p / q;
    const double stpc = stp + r * (stx - stp);
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
    brackt = 1;
  } else if (fabs(dp) < fabs(dx)) {
    const double theta = 3.0 * (fx - fp) / (stp - stx) + dx + dp;
    const double s = lb_max(lb_max(fabs(theta), fabs(dx)), fabs(dp));
    double gamma = s * sqrt(lb_max(0.0, (theta / s) * (theta / s) - (dx / s) * (dp / s)));
    if (stp > stx) gamma = -gamma;
    const double p = (gamma - dp) + theta;
    const double q = (gamma + (dx - dp)) + gamma;
    const double r = p / q;
    double stpc;
    if (r < 0.0 && gamma != 0.0) stpc = stp + r * (stx - stp);
    else if (stp > stx) stpc = stpmax;
    else stpc = stpmin;
    const double stpq = stp + (dp / (dp - dx)) * (stx - stp);
    if (brackt) {
      stpf = fabs(stpc - stp) < fabs(stpq - stp) ? stpc : stpq;
      if (stp > stx) stpf = lb_min(stp + 0.66 * (sty - stp), stpf);
      else stpf = lb_max(stp + 0.66 * (sty - stp), stpf);
    } else {
      stpf = fabs(stpc - stp) > fabs(stpq - stp) ? stpc : stpq;
      stpf = lb_clip(stpf, stpmin, stpmax);
    }
  } else {
    if (brackt) {
      const double theta = 3.0 * (fp - fy) / (sty - stp) + dy + dp;
      const double s = lb_max(lb_max(fabs(theta), fabs(dy)), fabs(dp));
      double gamma = s * sqrt((theta / s) * (theta / s) - (dy / s) * (dp / s));
      if (stp > sty) gamma = -gamma;
      const double p = (gamma - dp) + theta;
      const double q = ((gamma - dp) + gamma) + dy;
      const double r = p / q;
      stpf = stp + r * (sty - stp);
    } else if (stp > stx) {
      stpf = stpmax;
    } else {
      stpf = stpmin;
    }
  }
  // fp > fx: sty <- stp; else (opp: sty <- stx), stx <- stp  (as value selects: a select of addresses would live in scratch)
  const bool up = fp > fx;
  const double nsty = up ? stp : (opp ? stx : sty), nfy = up ? fp : (opp ? fx : fy), ndy = up ? dp : (opp ? dx : dy);
  const double nstx = up ? stx : stp, nfx = up ? fx : fp, ndx = up ? dx : dp;
  sty = nsty; fy = nfy; dy = ndy;
  stx = nstx; fx = nfx; dx = ndx;
  stp = stpf;
}

constexpr double kLbStpMax = 1e10, kLbFtol = 1e-3, kLbGtol = 0.9, kLbXtol = 0.1;
constexpr double kLbEps = 2.220446049250313e-16;

// dcsrch's START (lbfgs.LineSearch.start)
__device__ __forceinline__ void lb_ls_start(LbHdr& H, double f, double g, double stp) {
#pragma clang fp contract(off)
  H.brackt = 0; H.stage = 1;
  H.finit = f; H.ginit = g;
  H.gtest = kLbFtol * g;
  H.width = kLbStpMax - 0.0;
  H.width1 = H.width / 0.5;
  H.stx = 0.0; H.fx = f; H.gx = g;
  H.sty = 0.0; H.fy = f; H.gy = g;
  H.stmin = 0.0; H.stmax = stp + 4.0 * stp;
}

// dcsrch on phi(stp) = f, phi'(stp) = g (lbfgs.LineSearch._next): true = accept stp; false = evaluate at the new stp
__device__ __forceinline__ bool lb_ls_next(LbHdr& H, double& stp, double f, double g) {
#pragma clang fp contract(off)
  const double ftest = H.finit + stp * H.gtest;
  if (H.stage == 1 && f <= ftest && g >= 0.0) H.stage = 2;
  bool done = false;
  if (H.brackt && (stp <= H.stmin || stp >= H.stmax)) done = true;
  if (H.brackt && H.stmax - H.stmin <= kLbXtol * H.stmax) done = true;
  if (stp == kLbStpMax && f <= ftest && g <= H.gtest) done = true;
  if (stp == 0.0 && (f > ftest || g >= H.gtest)) done = true;
  if (f <= ftest && fabs(g) <= kLbGtol * -H.ginit) done = true;
  if (done) return true;
  // (one call site on local copies: the two forms of the reference's branches, the modified function of stage 1 and f itself)
  const bool mod = H.stage == 1 && f <= H.fx && f > ftest;
  double stx = H.stx, sty = H.sty, fx, gx, fy, gy, fp, gp;
  int brackt = H.brackt;
  if (mod) {
    fp = f - stp * H.gtest;
    fx = H.fx - H.stx * H.gtest;
    fy = H.fy - H.sty * H.gtest;
    gp = g - H.gtest;
    gx = H.gx - H.gtest;
    gy = H.gy - H.gtest;
  } else {
    fp = f; fx = H.fx; fy = H.fy; gp = g; gx = H.gx; gy = H.gy;
  }
  lb_dcstep(stx, fx, gx, sty, fy, gy, stp, fp, gp, brackt, H.stmin, H.stmax);
  H.stx = stx; H.sty = sty; H.brackt = brackt;
  if (mod) {
    H.fx = fx + stx * H.gtest;
    H.fy = fy + sty * H.gtest;
    H.gx = gx + H.gtest;
    H.gy = gy + H.gtest;
  } else {
    H.fx = fx; H.fy = fy; H.gx = gx; H.gy = gy;
  }
  if (H.brackt) {
    if (fabs(H.sty - H.stx) >= 0.66 * H.width1) stp = H.stx + 0.5 * (H.sty - H.stx);
    H.width1 = H.width;
    H.width = fabs(H.sty - H.stx);
    H.stmin = lb_min(H.stx, H.sty);
    H.stmax = lb_max(H.stx, H.sty);
  } else {
    H.stmin = stp + 1.1 * (stp - H.stx);
    H.stmax = stp + 4.0 * (stp - H.stx);
  }
  stp = lb_clip(stp, 0.0, kLbStpMax);
  if ((H.brackt && (stp <= H.stmin || stp >= H.stmax)) || (H.brackt && H.stmax - H.stmin <= kLbXtol * H.stmax)) stp = H.stx;
  return false;
}

// the sweep a pass does over the vectors (one per launch)
enum { kEvNone = 0, kEvEval0, kEvEval, kEvTrial, kEvRestore, kEvNegG, kEvY, kEvStore, kEvTlA, kEvTlB, kEvTlC, kEvTlD };

__global__ __launch_bounds__(kLbThreads) void k_lbfgs_step(const double* __restrict__ packed, double w0, double w1, double w2,
                                                           const int* __restrict__ act, int n_act, int B, int NP,
                                                           double* __restrict__ params, double* __restrict__ state, int maxcor,
                                                           double tol, double gtol, int maxiter, int maxfun, int maxls, int launch,
                                                           double* __restrict__ f_out, int* __restrict__ info) {
#pragma clang fp contract(off)
  __shared__ double red[kLbThreads];
  __shared__ double bcast;
  const int tid = threadIdx.x, G = gridDim.x, m = maxcor;
  const int par = launch & 1;
  LbHdr H;
  lb_copy(H, *reinterpret_cast<const LbHdr*>(state + par * kLbHdr));
  double* sy = state + 2 * kLbHdr;
  double* alpha = sy + m;
  const double* pin = state + lb_part_offset(m) + par * 2 * kLbMaxBlocks;
  double* pout = state + lb_part_offset(m) + (par ^ 1) * 2 * kLbMaxBlocks;
  const long n = (long)n_act * B;
  double* x0 = state + lb_vec_offset(m);
  double* g0 = x0 + n;
  double* d = g0 + n;
  double* q = d + n;
  double* S = q + n;
  double* Y = S + (long)m * n;
  const double f = (w0 * packed[0] + w1 * packed[1]) + w2 * packed[2];
  const double* g = packed + 3;
  const bool lead = blockIdx.x == 0 && tid == 0;

  int ev = kEvNone;
  double e_stp = 0.0, e_a = 0.0;   // the sweep's scalars
  int e_j = 0, e_j2 = 0, e_slot = -1;
  if (launch == 0) {   // the evaluation
    if (H.status != kLbRunning) {
      if (lead && f_out) *f_out = __longlong_as_double(0x7ff8000000000000LL);   // after the end: not used
      H.pc = kPcIdle;
    } else {
      H.nfev += 1;
      if (lead && f_out) *f_out = f;
      ev = H.started ? kEvEval : kEvEval0;
      H.pc = kPcDecide;
    }
  } else if (H.pc == kPcDecide) {   // f, g'd, max|g| at the point just evaluated
    const double gd = lb_grid_total<false>(pin, G, &bcast);
    const double mx = lb_grid_total<true>(pin + kLbMaxBlocks, G, &bcast);
    H.pc = kPcIdle;
    if (!H.started) {
      H.started = 1;
      H.f0 = f;
      if (mx <= gtol) {
        H.status = kLbConvGrad;
      } else {
        ev = kEvNegG;
        H.pc = kPcLsStart;
      }
    } else {
      double stp = H.stp;
      if (lb_ls_next(H, stp, f, gd)) {   // accepted: a new iterate
        H.nit += 1;
        const double f_old = H.f0;
        if (H.nit >= maxiter) H.status = kLbStopIter;
        else if (H.nfev > maxfun) H.status = kLbStopFun;
        else if (mx <= gtol) H.status = kLbConvGrad;
        else if (f_old - f <= tol * lb_max(lb_max(fabs(f_old), fabs(f)), 1.0)) H.status = kLbConvF;
        if (H.status == kLbRunning) {
          H.gdn = gd;
          ev = kEvY;
          H.pc = kPcStore;
        } else {
          H.f0 = f;   // the result: params hold the accepted trial
        }
      } else {
        H.ifun += 1;
        if (H.ifun - 1 >= maxls) {   // maxls evaluations in this line search: restart from its start point
          if (H.col == 0) {
            H.status = kLbAbnormal;
            ev = kEvRestore;
          } else {
            H.col = 0;
            H.head = 0;
            ev = kEvNegG;
            H.pc = kPcLsStart;
          }
        } else {
          H.stp = stp;
          e_stp = stp;
          ev = kEvTrial;
        }
      }
    }
  } else if (H.pc == kPcStore) {   // y'y: store the pair unless it is skipped (s'y as L-BFGS-B forms it), start the direction
    const double yy = lb_grid_total<false>(pin, G, &bcast);
    const double s_y = (H.gdn - H.gd0) * H.stp;
    if (s_y <= kLbEps * (-H.gd0 * H.stp)) {
      H.nskip += 1;
    } else {
      if (H.col < m) {
        e_slot = (H.head + H.col) % m;
        H.col += 1;
      } else {
        e_slot = H.head;
        H.head = (H.head + 1) % m;
      }
      if (lead) sy[e_slot] = s_y;
      H.gamma = s_y / yy;
    }
    H.f0 = f;
    e_stp = H.stp;
    ev = kEvStore;
    if (H.col == 0) {
      H.pc = kPcLsStart;   // (the sweep also forms d = -g)
    } else {
      e_j = (H.head + H.col - 1) % m;   // the newest pair
      H.pk = 1;
      H.pc = H.col > 1 ? kPcTlA : kPcTlB;
    }
  } else if (H.pc == kPcTlA) {   // first loop, pair k - 1 done: alpha, then q -= alpha y and s_k'q
    const int c = H.col, k = H.pk;
    const int jp = (H.head + c - k) % m, j = (H.head + c - 1 - k) % m;
    const double a = lb_grid_total<false>(pin, G, &bcast) / sy[jp];
    if (lead) alpha[k - 1] = a;
    ev = kEvTlA; e_a = a; e_j = jp; e_j2 = j;
    H.pk = k + 1;
    H.pc = H.pk < c ? kPcTlA : kPcTlB;
  } else if (H.pc == kPcTlB) {   // the oldest pair: alpha, q -= alpha y, r = gamma q, y'r
    const int c = H.col;
    const int j = H.head % m;
    const double a = lb_grid_total<false>(pin, G, &bcast) / sy[j];
    if (lead) alpha[c - 1] = a;
    ev = kEvTlB; e_a = a; e_j = j;
    H.pk = c - 1;
    H.pc = c > 1 ? kPcTlC : kPcTlD;
  } else if (H.pc == kPcTlC) {   // second loop at pair k: beta, r += (alpha - beta) s, then the next newer pair's y'r
    const int c = H.col, k = H.pk;
    const int jk = (H.head + c - 1 - k) % m, jn = (H.head + c - k) % m;
    const double b = lb_grid_total<false>(pin, G, &bcast) / sy[jk];
    ev = kEvTlC; e_a = alpha[k] - b; e_j = jk; e_j2 = jn;
    H.pk = k - 1;
    H.pc = H.pk >= 1 ? kPcTlC : kPcTlD;
  } else if (H.pc == kPcTlD) {   // the newest pair: d = -(r + (alpha - beta) s), g'd and d'd
    const int j0 = (H.head + H.col - 1) % m;
    const double b = lb_grid_total<false>(pin, G, &bcast) / sy[j0];
    ev = kEvTlD; e_a = alpha[0] - b; e_j = j0;
    H.pc = kPcLsStart;
  } else if (H.pc == kPcLsStart) {   // g'd, d'd of the new direction: the first trial of its line search
    const double gd = lb_grid_total<false>(pin, G, &bcast);
    const double dd = lb_grid_total<false>(pin + kLbMaxBlocks, G, &bcast);
    H.pc = kPcIdle;
    if (!(gd >= 0.0)) {
      const double stp = H.nit == 0 ? lb_min(1.0 / sqrt(dd), kLbStpMax) : 1.0;
      H.gd0 = gd;
      lb_ls_start(H, H.f0, gd, stp);
      H.stp = stp;
      H.ifun = 1;
      e_stp = stp;
      ev = kEvTrial;
    } else if (H.col == 0) {   // not a descent direction with an empty memory: abnormal, params back to the accepted point
      H.status = kLbAbnormal;
      ev = kEvRestore;
    } else {   // reset the memory and try -g
      H.col = 0;
      H.head = 0;
      ev = kEvNegG;
      H.pc = kPcLsStart;
    }
  }

  // the sweep: global thread t owns elements t, t + NT, ...
  if (ev != kEvNone) {
    const long NT = (long)G * kLbThreads;
    double p0 = 0.0, p1 = 0.0;
    for (long i = (long)blockIdx.x * kLbThreads + tid; i < n; i += NT) {
      const long kk = i / B;
      const long o = (i - kk * B) * NP + act[kk];
      switch (ev) {
        case kEvEval0: {
          x0[i] = params[o];
          g0[i] = g[i];
          p1 = lb_maxc(p1, fabs(g[i]));
          break;
        }
        case kEvEval: {
          p0 = p0 + g[i] * d[i];
          p1 = lb_maxc(p1, fabs(g[i]));
          break;
        }
        case kEvTrial: params[o] = x0[i] + e_stp * d[i]; break;
        case kEvRestore: params[o] = x0[i]; break;
        case kEvNegG: {
          const double gi = g0[i];
          const double di = -gi;
          d[i] = di;
          p0 = p0 + gi * di;
          p1 = p1 + di * di;
          break;
        }
        case kEvY: {
          const double y = g[i] - g0[i];
          q[i] = y;
          p0 = p0 + y * y;
          break;
        }
        case kEvStore: {
          if (e_slot >= 0) {
            S[e_slot * n + i] = e_stp * d[i];
            Y[e_slot * n + i] = q[i];
          }
          x0[i] = params[o];
          const double gi = g[i];
          g0[i] = gi;
          if (H.col == 0) {
            const double di = -gi;
            d[i] = di;
            p0 = p0 + gi * di;
            p1 = p1 + di * di;
          } else {
            q[i] = gi;
            p0 = p0 + S[e_j * n + i] * gi;
          }
          break;
        }
        case kEvTlA: {
          const double qi = q[i] - e_a * Y[e_j * n + i];
          q[i] = qi;
          p0 = p0 + S[e_j2 * n + i] * qi;
          break;
        }
        case kEvTlB: {
          const double qi = q[i] - e_a * Y[e_j * n + i];
          const double r = qi * H.gamma;
          q[i] = r;
          p0 = p0 + Y[e_j * n + i] * r;
          break;
        }
        case kEvTlC: {
          const double r = q[i] + e_a * S[e_j * n + i];
          q[i] = r;
          p0 = p0 + Y[e_j2 * n + i] * r;
          break;
        }
        case kEvTlD: {
          const double r = q[i] + e_a * S[e_j * n + i];
          const double di = -r;
          d[i] = di;
          p0 = p0 + g0[i] * di;
          p1 = p1 + di * di;
          break;
        }
        default: break;
      }
    }
    const bool two_sums = ev == kEvNegG || ev == kEvTlD || (ev == kEvStore && H.col == 0);
    const double r0 = lb_wg_reduce<false>(p0, red);
    const double r1 = (ev == kEvEval || ev == kEvEval0) ? lb_wg_reduce<true>(p1, red)
                      : two_sums ? lb_wg_reduce<false>(p1, red) : 0.0;
    if (tid == 0) {
      pout[blockIdx.x] = r0;
      pout[kLbMaxBlocks + blockIdx.x] = r1;
    }
  }
  if (lead) {
    lb_copy(*reinterpret_cast<LbHdr*>(state + (par ^ 1) * kLbHdr), H);
    if (info) { info[0] = H.status; info[1] = H.nit; info[2] = H.nfev; info[3] = H.nskip; }
  }
}
