// k_chain.inc -- the instrument and loss chain around the spectrum kernels' sweeps, each rule stated once: bin amplitudes,
// theory value, per-bin loss, the adjoint of normalisation and amplitudes, and the gradient tail from the physical parameters
// to the optimiser's leaves.  Values in, values out: every caller keeps its own load placement.

// A_p, the amplitude of bin p: amps amp1 / amp2 on either side of lam for the electron feature, amps amp3 for the ion feature,
// 1 in a raw spectrum (irf.py:82-86).  lam_b: the bin's wavelength (electron feature only)
__device__ __forceinline__ double bin_amplitude(int f, bool raw, double amps, double lam_b, double p_lam, double p_amp1,
                                                double p_amp2, double p_amp3) {
  if (f == TSFF_FEATURE_ELE) return amps * (lam_b < p_lam ? p_amp1 : p_amp2);  // irf.py:126-130
  return raw ? 1.0 : amps * p_amp3;                                            // irf.py:76
}

// T_p = A_p ybin_p / M (+ noise_p) (irf.py:76,126-130; thomson_diagnostic.py:139-140) with its roundings written out -- product,
// product, sum, never a fused multiply-add -- so that a spectrum is the same bits from every kernel whatever shape the
// surrounding code gives the compiler (test_launch_plans_agree)
__device__ __forceinline__ double thry_value(double A, double y, double invM, bool has_noise, double noise) {
#pragma clang fp contract(off)
  const double t = (A * y) * invM;
  return has_noise ? t + noise : t;
}

// loss functional e(d, t) and de/dt (loss_function.py:386-418); the 1/uncert of l1/l2 is folded
// into the weights by the host (constant denominators) or applied here (theory denominator).
__device__ __forceinline__ void loss_point(int method, double d, double t, double& e, double& det) {
  const double r = d - t;
  if (method == TSFF_LOSS_L2) { e = r * r; det = -2.0 * r; }
  else if (method == TSFF_LOSS_L1) { e = fabs(r); det = r > 0.0 ? -1.0 : (r < 0.0 ? 1.0 : 0.0); }
  else if (method == TSFF_LOSS_LOGCOSH) { e = log(cosh(r)); det = -tanh(r); }
  else { e = t - d * log(t); det = 1.0 - d / t; }
}

// the fit loss of one bin (data d, theory t, fit-range mask mk): adds e to the loss sums of the ranges it lies in and returns
// dLoss/dT, the weighted de/dt
__device__ __forceinline__ double bin_loss(const KStatic& S, const KCall& K, int f, double d, double t, uint8_t mk,
                                           double& s0, double& s1) {
  double e, det;
  loss_point(S.loss_method, d, t, e, det);
  if (K.denom_mode == 2 && (S.loss_method == TSFF_LOSS_L2 || S.loss_method == TSFF_LOSS_L1)) {
    const double iden = 1.0 / (fabs(d) + 1e-10);  // loss_function.py:183 (_loss_for_hess_fn_)
    e *= iden;
    det *= iden;
  }
  double w = 0.0;
  if (mk & 1) { s0 += e; w += (f == TSFF_FEATURE_ELE ? K.wts[1] : K.wts[0]); }
  if (mk & 2) { s1 += e; w += K.wts[2]; }
  return w != 0.0 ? det * w : 0.0;  // (samples outside every fit range may hold anything, NaN included)
}

// one bin's part of the adjoint of T_p = A_p ybin_p / M: sn = sum_p u_p A_p and the amplitude adjoints a1b, a2b (amp3's in a1b
// for the ion feature), u_p = Tb_p ybin_p / M.  The amplitude adjoint rounds u_p amps before the sum, never a fused multiply-add:
// the bits of the branch-per-bin form this rule had in every kernel, whatever shape the compiler gives the selection.
__device__ __forceinline__ void norm_adjoint_bin(int f, double Tb, double y, double invM, double A, double amps, double lam_b,
                                                 double p_lam, double& sn, double& a1b, double& a2b) {
  const double u = Tb * y * invM;  // dL/dA_p
  sn += u * A;
  double& ab = (f != TSFF_FEATURE_ELE || lam_b < p_lam) ? a1b : a2b;
  {
#pragma clang fp contract(off)
    ab += u * amps;
  }
}

// ------------------------------------------------------------------------------------------
// gradient tail: physical-parameter adjoints g[NP] -> d loss / d leaves
// ------------------------------------------------------------------------------------------
// amplitudes (irf.py:76,126-130)
__device__ __forceinline__ void amp_adjoint(int f, double a1b, double a2b, double* g) {
  g[f == TSFF_FEATURE_ELE ? TSFF_P_AMP1 : TSFF_P_AMP3] += a1b;
  if (f == TSFF_FEATURE_ELE) g[TSFF_P_AMP2] += a2b;
}

// Ti tying and fraction renormalisation (ts_params.py:543-563); A is never a leaf, nor m without DLM tables (with_m)
template <int NI>
__device__ __forceinline__ void tie_renorm_adjoint(const KStatic& S, const Phys<NI>& p, bool with_m, double* g) {
#pragma unroll
  for (int s = 1; s < NI; ++s)
    if (S.ti_same[s]) {
      g[TSFF_P_ION0 + TSFF_ION_TI] += g[TSFF_P_ION0 + 4 * s + TSFF_ION_TI];
      g[TSFF_P_ION0 + 4 * s + TSFF_ION_TI] = 0.0;
    }
  double dot = 0.0;
#pragma unroll
  for (int s = 0; s < NI; ++s) dot += g[TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT] * p.fr[s];
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    const int o = TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT;
    g[o] = (g[o] - dot) / p.fsum;
    g[TSFF_P_ION0 + 4 * s + TSFF_ION_A] = 0.0;
  }
  if (!with_m) g[TSFF_P_M] = 0.0;
}

// activation (ts_params.py:329-350) and the gradient mask: d loss / d x of a slot from its physical adjoint g.  sig: the slot
// goes through a sigmoid, whose value sgf() is asked for only then; mask: the slot is a leaf
template <class SGF>
__device__ __forceinline__ double activation_adjoint(double g, double scale, bool sig, SGF sgf, bool mask) {
  double v = g * scale;
  if (sig) { const double sg = sgf(); v *= sg * (1.0 - sg); }
  return mask ? v : 0.0;
}
