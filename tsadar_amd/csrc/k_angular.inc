// k_angular.inc -- the angular (ARTS) fit loop on the device (tsff_angular_fit): the reference's angular_optax
// (inverse/loops.py:167-275) with LossFunction._vg_angular_adjoint's value and gradient, one epoch per pass of
//   k_ang_leaves -> form factor (1-D or 2-D, saved projections) -> ATS chain -> k_ang_loss -> ATS adjoint -> form-factor adjoint
//   -> k_ang_chain -> k_ang_opt
// k_ang_loss spreads the image over up to kAngLossBlocks workgroups, whose partial sums k_ang_loss_sum adds in block order (a
// fixed partition: the loss does not depend on timing).  The other kernels are one workgroup of kThreads: their vectors are one
// plasma condition's (NP leaves, nvx or nvx^2 table values), and one workgroup makes every decision of the optimiser and of the
// early stop without a cross-workgroup order.
//
// Bit contract of k_ang_opt: the update is tsadar_amd.tree.Adam / tree.RMSProp + tree.apply_updates operation for operation in
// double, nothing fused (as k_adam.inc).  The loss and the chain rule reduce in the workgroup's order, not NumPy's: the loss and
// the gradient agree with the host loop to rounding, not bit for bit.

// Leaves -> physical parameters (ThomsonParams.physical_matrix: activation, Ti tying, fraction renormalisation) and the
// distribution function of the deck's generator:
//   DLM (1-D): fe = DLM1V(m) (distribution.dlm: linear in m between the 31 table columns, normalised to unit integral) and, for
//              the chain rule of m, dfe = (dlm(m + h) - dlm(m - h)) / (2 h), h = 1e-6 (LossFunction._vg_angular_adjoint);
//   Arbitrary2V: fe = f / sum f / dv^2 with f = fval^2 (learn_log: 10^-fval^2) (distribution.arbitrary_2v); aux[0] = sum f.
//   SphericalHarmonics (TSFF_ANG_SPH): k_sph_table after this kernel and k_sph_vjp after k_ang_chain (k_sph.inc).
//   Arbitrary1V (TSFF_ANG_ARB1V): k_arb1v_matvec and k_arb1v_point after this kernel, and again, in the other order, after
//              k_ang_chain (k_arb1v.inc); this kernel writes the physical parameters only.
__device__ __forceinline__ void ang_dlm(const double* __restrict__ tab, const double* __restrict__ maxis, int nvx, double dvx, double m,
                                        double* __restrict__ out, double* red) {
  int k = 0;   // searchsorted(M_AXIS, m, side="right") clipped to [1, 30]
  for (int i = 0; i < 31; ++i) k += maxis[i] <= m ? 1 : 0;
  k = k < 1 ? 1 : (k > 30 ? 30 : k);
  double t = (m - maxis[k - 1]) / (maxis[k] - maxis[k - 1]);
  t = fmin(fmax(t, 0.0), 1.0);
  double s = 0.0;
  for (int j = threadIdx.x; j < nvx; j += kThreads) {
    const double a = tab[(size_t)j * 31 + k - 1], b = tab[(size_t)j * 31 + k];
    const double f = a + t * (b - a);
    out[j] = f;
    s += f;
  }
  s = block_sum(s, red);
  for (int j = threadIdx.x; j < nvx; j += kThreads) out[j] = out[j] / s / dvx;
}

template <int NI>
__global__ __launch_bounds__(kThreads) void k_ang_leaves(KStatic S, const double* __restrict__ leaves, int gen, int learn_log, int nv,
                                                         const double* __restrict__ gen_data, double dvx, double dv2, int want_dm,
                                                         double* __restrict__ phys, double* __restrict__ fe, double* __restrict__ dfe,
                                                         double* __restrict__ aux) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ double ph[kNP_MAX + 1];
  if (threadIdx.x == 0) {
    Phys<NI> p;
    load_phys<NI>(leaves, S.p_scale, S.p_shift, S.p_sig, S.ti_same, true, p);
    phys_to_array<NI>(p, ph);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < S.NP; s += kThreads) phys[s] = ph[s];
  if (gen == TSFF_ANG_DLM) {
    const double* tab = gen_data;
    const double* maxis = gen_data + (size_t)nv * 31;
    const double m = ph[TSFF_P_M];
    ang_dlm(tab, maxis, nv, dvx, m, fe, red);
    if (want_dm) {   // dfe holds dlm(m - h) until the difference quotient
      const double hm = 1e-6;
      ang_dlm(tab, maxis, nv, dvx, m - hm, dfe, red);
      __syncthreads();
      double* fp = dfe + nv;   // (scratch: the second half of the dfe buffer)
      ang_dlm(tab, maxis, nv, dvx, m + hm, fp, red);
      __syncthreads();
      for (int j = threadIdx.x; j < nv; j += kThreads) dfe[j] = (fp[j] - dfe[j]) / (2.0 * hm);
    }
  } else if (gen == TSFF_ANG_ARB2V) {
    const double* fval = leaves + S.NP;
    const long n = (long)nv * nv;
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += kThreads) {
      double f = fval[i] * fval[i];
      if (learn_log) f = pow(10.0, -f);
      fe[i] = f;
      s += f;
    }
    s = block_sum(s, red);
    for (long i = threadIdx.x; i < n; i += kThreads) fe[i] = fe[i] / s / dv2;
    if (threadIdx.x == 0) aux[0] = s;
  }
}

// _angular_value_device: Et = ThryE + noise_e, err and d err / d Et per loss_method (TSFF_LOSS_*),
// value = sum err * wcol (wcol: the blue / red masks of the resolution-unit axis over rows x mask count, halved when both are
// fitted: the nanmean of the reference), Ebar = derr * wcol.  partial[blockIdx.x] = this workgroup's share of the value
// (grid-stride over the image), summed by k_ang_loss_sum.
constexpr int kAngLossBlocks = 256;
__global__ __launch_bounds__(kThreads) void k_ang_loss(const double* __restrict__ E, const double* __restrict__ noise,
                                                       const double* __restrict__ data, const double* __restrict__ wcol, int rows, int nJ,
                                                       int method, double un, double* __restrict__ Ebar, double* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  const long n = (long)rows * nJ;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const double w = wcol[i % nJ];
    const double Et = E[i] + noise[i], d = data[i], r = d - Et;
    double err, derr;
    if (method == TSFF_LOSS_L1) { err = fabs(r) / un; derr = -(double)((r > 0.0) - (r < 0.0)) / un; }
    else if (method == TSFF_LOSS_L2) { err = (r * r) / un; derr = (-2.0 * r) / un; }
    else if (method == TSFF_LOSS_LOGCOSH) { err = log(cosh(r)); derr = -tanh(r); }
    else { err = Et - d * log(Et); derr = 1.0 - d / Et; }
    acc += err * w;
    Ebar[i] = derr * w;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// loss[0] = the sum of the n <= kAngLossBlocks partials of k_ang_loss, in a fixed order (one workgroup)
__global__ __launch_bounds__(kThreads) void k_ang_loss_sum(const double* __restrict__ partial, int n, double* __restrict__ loss) {
  __shared__ double red[8];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) acc += partial[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *loss = acc;
}

// LossFunction._vg_angular_adjoint's chain rule on the device: gphys (the form-factor adjoint) + the amplitude adjoints of the
// ATS chain (ampb [rows][2], summed in row order) + the DLM order (dot(gfe, dfe)), Ti tying, activation
// (scale x sigmoid'), then d loss / d fval of Arbitrary2V (distribution.arbitrary_2v_vjp).  grad: [n_act | nv^2] (the optimiser's
// layout: the active scalar slots in the order of act, then the table).
template <int NI>
__global__ __launch_bounds__(kThreads) void k_ang_chain(KStatic S, const double* __restrict__ leaves, const double* __restrict__ gphys,
                                                        const double* __restrict__ ampb, int rows, const double* __restrict__ gfe,
                                                        const double* __restrict__ dfe, int nvx, int train_table, int learn_log, int nv,
                                                        const double* __restrict__ aux, double cvjp, double ln10,
                                                        const int* __restrict__ act, int n_act, double* __restrict__ grad) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  double dm = 0.0;
  if (dfe) {
    for (int j = threadIdx.x; j < nvx; j += kThreads) dm += gfe[j] * dfe[j];
    dm = block_sum(dm, red);
  }
  const double* fval = leaves + S.NP;
  const long n = (long)nv * nv;
  double s2 = 0.0;
  if (train_table) {
    for (long i = threadIdx.x; i < n; i += kThreads) {
      double f = fval[i] * fval[i];
      if (learn_log) f = pow(10.0, -f);
      s2 += gfe[i] * f;
    }
    s2 = block_sum(s2, red);
  }
  if (threadIdx.x == 0) {
    double g[kNP_MAX];
    for (int s = 0; s < S.NP; ++s) g[s] = gphys[s];
    if (dfe) g[TSFF_P_M] = dm;
    double a1 = 0.0, a2 = 0.0;
    for (int r = 0; r < rows; ++r) { a1 += ampb[2 * r]; a2 += ampb[2 * r + 1]; }
    g[TSFF_P_AMP1] += a1;
    g[TSFF_P_AMP2] += a2;
    for (int i = 1; i < NI; ++i)
      if (S.ti_same[i]) {
        g[TSFF_P_ION0 + TSFF_ION_TI] += g[TSFF_P_ION0 + 4 * i + TSFF_ION_TI];
        g[TSFF_P_ION0 + 4 * i + TSFF_ION_TI] = 0.0;
      }
    for (int k = 0; k < n_act; ++k) {
      const int s = act[k];
      double v = g[s] * S.p_scale[s];
      if (S.p_sig[s]) { const double sg = sigmoid(leaves[s]); v = v * (sg * (1.0 - sg)); }
      grad[k] = v;
    }
  }
  if (train_table) {
    const double tot = aux[0];
    const double q = s2 / (tot * tot);
    for (long i = threadIdx.x; i < n; i += kThreads) {
      const double fv = fval[i];
      double f = fv * fv;
      if (learn_log) f = pow(10.0, -f);
      const double fb = cvjp * (gfe[i] / tot - q);
      grad[n_act + i] = learn_log ? ((fb * (-ln10 * f)) * 2.0) * fv : (fb * 2.0) * fv;
    }
  }
}

// One optimiser step over the trained leaves (the active scalar slots of leaves[NP], then the table leaves[NP ..)) and the
// early stop of angular_optax as written (loops.py:243-266):
//   val < best and best - val < 1e-6: best = val, best leaves = the updated leaves, g_wait += 1, stop once g_wait > 5;
//   val < best otherwise:             best = val, best leaves = the updated leaves, g_wait = b_wait = 0;
//   (the reference's "elif val > best" sits under "if val < best" and never runs).
// ctl (int32): [0] status (0 running, 1 ended), [1] the epoch it ended after, [2] g_wait, [3] b_wait, [4] 1 once a best exists.
// Once ended, later epochs change nothing and log NaN.  method 0: Adam (mu = mom[0..n), nu = mom[n..2n)), 1: RMSProp (nu = mom[0..n)).
// best_hist (optional) [epochs][n_hist]: the best scalar leaves after each epoch (save_state; n_hist = NP, or NP + n_gen with the
// parameters of a trained SphericalHarmonics generator, NP + nv with the fval of a trained Arbitrary1V, behind them), untouched while no best exists.
__global__ __launch_bounds__(kThreads) void k_ang_opt(const double* __restrict__ loss, const double* __restrict__ grad,
                                                      const int* __restrict__ act, int n_act, int NP, long n_table,
                                                      double* __restrict__ leaves, double* __restrict__ mom, int method, double b1,
                                                      double omb1, double b2, double omb2, double neg_lr, double c1, double c2, double eps,
                                                      int* __restrict__ ctl, double* __restrict__ best, int epoch,
                                                      double* __restrict__ loss_hist, double* __restrict__ best_hist, int n_hist) {
#pragma clang fp contract(off)
  __shared__ int dec[2];
  const double val = *loss;
  const bool running = ctl[0] == 0;
  const double bl = best[0];
  const bool improve = running && val < bl;
  const bool small = improve && bl - val < 1e-6;
  const long n = (long)n_act + n_table;
  if (running) {
    for (long i = threadIdx.x; i < n; i += kThreads) {
      const long o = i < n_act ? (long)act[i] : NP + (i - n_act);
      const double g = grad[i];
      double upd;   // (the formulas and their bit contract: k_adam.inc)
      if (method == 0) upd = adam_update(g, mom[i], mom[n + i], b1, omb1, b2, omb2, neg_lr, c1, c2, eps);
      else upd = rmsprop_update(g, mom[i], b2, omb2, neg_lr, eps);
      const double x = leaves[o] + upd;
      leaves[o] = x;
    }
  }
  __syncthreads();
  if (improve) {   // the whole updated iterate (the reference stores eqx.combine(diff_params, static_params))
    for (long i = threadIdx.x; i < NP + n_table; i += kThreads) best[1 + i] = leaves[i];
  }
  if (threadIdx.x == 0) {
    if (loss_hist) *loss_hist = running ? val : __builtin_nan("");
    if (improve) {
      best[0] = val;
      ctl[4] = 1;
      if (small) {
        ctl[2] += 1;
        if (ctl[2] > 5) { ctl[0] = 1; ctl[1] = epoch; }
      } else {
        ctl[2] = 0;
        ctl[3] = 0;
      }
    }
    dec[0] = ctl[4];
  }
  __syncthreads();
  if (best_hist && running && dec[0])
    for (int s = threadIdx.x; s < n_hist; s += kThreads) best_hist[s] = best[1 + s];
}
