// k_ats.inc -- angular (ARTS) instrument chain and its adjoint.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).

// ------------------------------------------------------------------------------------------
// Angular (ARTS) instrument chain: FitModel.electron_spectrum for spectype "angular_full"
// (generate_spectra.py:193-216), add_ATS_IRF (irf.py:5-47), reduce_ATS_to_resunit
// (thomson_diagnostic.py:78-107).  Five small kernels over [n_px x npts] images; none of them is hot.
// ------------------------------------------------------------------------------------------
// M[r][j] = filt[j] * sum_a Wt[r][a] * mean_g P[g][j][a]
__global__ void k_ats_weights(const double* __restrict__ P, const double* __restrict__ Wt, const double* __restrict__ filt,
                              int G, int npts, int NA, int npx, double* __restrict__ M) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (j >= npts) return;
  double acc = 0.0;
  for (int a = 0; a < NA; ++a) {
    const double w = Wt[(size_t)r * NA + a];
    if (w == 0.0) continue;
    double m = 0.0;
    for (int g = 0; g < G; ++g) m += P[((size_t)g * npts + j) * NA + a];
    acc += w * (m / (double)G);
  }
  M[(size_t)r * npts + j] = filt ? acc * filt[j] : acc;
}

// "same" convolution along the angular-pixel axis (dim 0) or the wavelength axis (dim 1):
// y[i] = sum_s taps[s] x[i + off + s], zero outside
__global__ void k_ats_conv(const double* __restrict__ X, const double* __restrict__ taps, int nt, int off, int along_rows,
                           int npx, int npts, double* __restrict__ Y) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (j >= npts) return;
  double acc = 0.0;
  if (along_rows) {
    for (int s = 0; s < nt; ++s) {
      const int rr = r + off + s;
      if (rr >= 0 && rr < npx) acc += taps[s] * X[(size_t)rr * npts + j];
    }
  } else {
    for (int s = 0; s < nt; ++s) {
      const int jj = j + off + s;
      if (jj >= 0 && jj < npts) acc += taps[s] * X[(size_t)r * npts + jj];
    }
  }
  Y[(size_t)r * npts + j] = acc;
}

// per angular pixel: Y[r][:] *= max_j M[r][:] / max_j Y[r][:]   (irf.py:38)
__global__ __launch_bounds__(kThreads) void k_ats_rownorm(const double* __restrict__ M, double* __restrict__ Y, int npts) {
  __shared__ double red[8];
  const int r = blockIdx.x;
  double mm = -1e300, my = -1e300;
  for (int j = threadIdx.x; j < npts; j += kThreads) {
    mm = fmax(mm, M[(size_t)r * npts + j]);
    my = fmax(my, Y[(size_t)r * npts + j]);
  }
  int dummy = 0;
  block_argmax(mm, dummy, red);
  dummy = 0;
  block_argmax(my, dummy, red);
  const double sc = mm / my;
  for (int j = threadIdx.x; j < npts; j += kThreads) Y[(size_t)r * npts + j] *= sc;
}

// resolution-unit reduction + amplitude scaling (thomson_diagnostic.py:93-106): one workgroup per output row.  phys (optional):
// lam, amp1 and amp2 are read from these physical parameters instead of the scalar arguments
__global__ __launch_bounds__(kThreads) void k_ats_resunit(const double* __restrict__ Y, const double* __restrict__ lam_nm,
                                                          int npts, int lam_step, int ang_step, int row_start,
                                                          const double* __restrict__ e_amps, double lam, double amp1, double amp2,
                                                          const double* __restrict__ phys, double* __restrict__ out) {
  __shared__ double red[8];
  if (phys) { lam = phys[TSFF_P_LAM]; amp1 = phys[TSFF_P_AMP1]; amp2 = phys[TSFF_P_AMP2]; }   // (tsff_angular_fit: on the device)
  const int R = blockIdx.x, nJ = npts / lam_step;
  const int r0 = (row_start + R) * ang_step;
  double mx = -1e300;
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double acc = 0.0;
    for (int dr = 0; dr < ang_step; ++dr)
      for (int dj = 0; dj < lam_step; ++dj) acc += Y[(size_t)(r0 + dr) * npts + J * lam_step + dj];
    acc /= (double)(ang_step * lam_step);
    out[(size_t)R * nJ + J] = acc;
    mx = fmax(mx, acc);
  }
  int dummy = 0;
  block_argmax(mx, dummy, red);
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double lb = 0.0;
    for (int dj = 0; dj < lam_step; ++dj) lb += lam_nm[J * lam_step + dj];
    lb /= (double)lam_step;
    out[(size_t)R * nJ + J] = e_amps[R] * out[(size_t)R * nJ + J] / mx * (lb < lam ? amp1 : amp2);
  }
}

// ---- adjoint of the ARTS instrument chain (reverse of the five kernels above) ----
// per angular pixel r: maxima of the unconvolved (M) and convolved (Bm, unscaled) rows and where they sit
__global__ __launch_bounds__(kThreads) void k_ats_rowstats(const double* __restrict__ M, const double* __restrict__ Bm, int npts,
                                                           double* __restrict__ stats /*[npx][4]: mM, jM, mB, jB*/) {
  __shared__ double red[8];
  const int r = blockIdx.x;
  double mm = -1e300, mb = -1e300;
  int jm = 0, jb = 0;
  for (int j = threadIdx.x; j < npts; j += kThreads) {
    const double a = M[(size_t)r * npts + j], c = Bm[(size_t)r * npts + j];
    if (a > mm) { mm = a; jm = j; }
    if (c > mb) { mb = c; jb = j; }
  }
  block_argmax(mm, jm, red);
  block_argmax(mb, jb, red);
  if (threadIdx.x == 0) { stats[4 * r] = mm; stats[4 * r + 1] = jm; stats[4 * r + 2] = mb; stats[4 * r + 3] = jb; }
}

// reverse of k_ats_resunit (+ the scaling of k_ats_rownorm): one workgroup per output row R.  Ebar [rows][nJ] ->
// Cbar[r][j] for the rows / columns of R's resolution units (C = Bm * sc_r); amp adjoints accumulated per row.
__global__ __launch_bounds__(kThreads) void k_ats_resunit_adj(const double* __restrict__ Bm, const double* __restrict__ stats,
                                                              const double* __restrict__ lam_nm, int npts, int lam_step,
                                                              int ang_step, int row_start, const double* __restrict__ e_amps,
                                                              double lam, double amp1, double amp2, const double* __restrict__ phys,
                                                              const double* __restrict__ Ebar, double* __restrict__ Cbar,
                                                              double* __restrict__ ampbar /*[rows][2]*/) {
  __shared__ double red[8];
  if (phys) { lam = phys[TSFF_P_LAM]; amp1 = phys[TSFF_P_AMP1]; amp2 = phys[TSFF_P_AMP2]; }
  __shared__ double Dl[TSFF_NBINS];
  const int R = blockIdx.x, nJ = npts / lam_step;
  const int r0 = (row_start + R) * ang_step;
  const double inv = 1.0 / (double)(ang_step * lam_step);
  double mx = -1e300;
  int js = 0;
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double acc = 0.0;
    for (int dr = 0; dr < ang_step; ++dr) {
      const double sc = stats[4 * (r0 + dr)] / stats[4 * (r0 + dr) + 2];
      for (int dj = 0; dj < lam_step; ++dj) acc += Bm[(size_t)(r0 + dr) * npts + J * lam_step + dj] * sc;
    }
    acc *= inv;
    Dl[J] = acc;
    if (acc > mx) { mx = acc; js = J; }
  }
  block_argmax(mx, js, red);
  double su = 0.0, a1 = 0.0, a2 = 0.0;
  const double ea = e_amps[R];
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double lb = 0.0;
    for (int dj = 0; dj < lam_step; ++dj) lb += lam_nm[J * lam_step + dj];
    lb /= (double)lam_step;
    const bool blue = lb < lam;
    const double eb = Ebar[(size_t)R * nJ + J];
    const double base = eb * ea * Dl[J] / mx;      // d out / d amp
    if (blue) a1 += base; else a2 += base;
    su += eb * ea * (blue ? amp1 : amp2) * Dl[J] / mx;   // sum_J u_J D_J, u_J = Ebar ea amp / mx
  }
  su = block_sum(su, red);
  a1 = block_sum(a1, red);
  a2 = block_sum(a2, red);
  if (threadIdx.x == 0) { ampbar[2 * R] = a1; ampbar[2 * R + 1] = a2; }
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double lb = 0.0;
    for (int dj = 0; dj < lam_step; ++dj) lb += lam_nm[J * lam_step + dj];
    lb /= (double)lam_step;
    double db = Ebar[(size_t)R * nJ + J] * ea * (lb < lam ? amp1 : amp2) / mx;
    if (J == js) db -= su / mx;
    db *= inv;
    for (int dr = 0; dr < ang_step; ++dr)
      for (int dj = 0; dj < lam_step; ++dj) Cbar[(size_t)(r0 + dr) * npts + J * lam_step + dj] = db;
  }
}

// reverse of k_ats_rownorm: C = Bm * sc, sc = mM / mB.  In place: Cbar -> Bmbar; Mbar gets the one-hot of d sc / d mM
__global__ __launch_bounds__(kThreads) void k_ats_rownorm_adj(const double* __restrict__ Bm, const double* __restrict__ stats,
                                                              int npts, double* __restrict__ Cbar, double* __restrict__ Mbar) {
  __shared__ double red[8];
  const int r = blockIdx.x;
  const double mM = stats[4 * r], mB = stats[4 * r + 2];
  const int jM = (int)stats[4 * r + 1], jB = (int)stats[4 * r + 3];
  double scb = 0.0;
  for (int j = threadIdx.x; j < npts; j += kThreads) scb += Cbar[(size_t)r * npts + j] * Bm[(size_t)r * npts + j];
  scb = block_sum(scb, red);
  const double sc = mM / mB;
  for (int j = threadIdx.x; j < npts; j += kThreads) {
    double v = Cbar[(size_t)r * npts + j] * sc;
    if (j == jB) v -= scb * mM / (mB * mB);
    Cbar[(size_t)r * npts + j] = v;
    Mbar[(size_t)r * npts + j] = j == jM ? scb / mB : 0.0;
  }
}

// ---- forward mode of the two row normalisations (tsff_ats_jvp; the linear stages run the forward kernels on the tangent image) ----
// tangent of k_ats_rownorm: Y = Bm sc, sc = mM / mB with the maxima where k_ats_rowstats found them (the first in index order), so
// Y' = Bm' sc + Bm sc', sc' = M'[jM] / mB - mM Bm'[jB] / mB^2.  Ys: the SCALED image Y (k_ats_rownorm has run), Bd: Bm' in, Y' out.
__global__ __launch_bounds__(kThreads) void k_ats_rownorm_jvp(const double* __restrict__ Ys, const double* __restrict__ stats,
                                                              const double* __restrict__ Md, int npts, double* __restrict__ Bd) {
  const int r = blockIdx.x;
  const double mM = stats[4 * r], mB = stats[4 * r + 2];
  const int jM = (int)stats[4 * r + 1], jB = (int)stats[4 * r + 3];
  const double sc = mM / mB;
  const double rel = Md[(size_t)r * npts + jM] / mM - Bd[(size_t)r * npts + jB] / mB;   // sc' / sc
  __syncthreads();   // (Bm'[jB] is read by every thread before its owner overwrites it)
  for (int j = threadIdx.x; j < npts; j += kThreads)
    Bd[(size_t)r * npts + j] = Bd[(size_t)r * npts + j] * sc + Ys[(size_t)r * npts + j] * rel;
}

// tangent of k_ats_resunit: out = e_amps D / mx amp with D the block means, mx = D[js] its row maximum (the first in index order) and
// amp = amp1 | amp2 by the wavelength, so out' = e_amps ((D' / mx - D mx' / mx^2) amp + D / mx amp'), mx' = D'[js].  `lam` only
// selects between the amplitudes.  One workgroup per output row; at most TSFF_NBINS resolution units per row.
__global__ __launch_bounds__(kThreads) void k_ats_resunit_jvp(const double* __restrict__ Y, const double* __restrict__ Yd,
                                                              const double* __restrict__ lam_nm, int npts, int lam_step, int ang_step,
                                                              int row_start, const double* __restrict__ e_amps, double lam, double amp1,
                                                              double amp2, double amp1_dot, double amp2_dot, double* __restrict__ out_dot) {
  __shared__ double red[8];
  __shared__ double Dl[TSFF_NBINS], Dd[TSFF_NBINS];
  const int R = blockIdx.x, nJ = npts / lam_step;
  const int r0 = (row_start + R) * ang_step;
  const double cnt = (double)(ang_step * lam_step);
  double mx = -1e300;
  int js = 0;
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double acc = 0.0, accd = 0.0;
    for (int dr = 0; dr < ang_step; ++dr)
      for (int dj = 0; dj < lam_step; ++dj) {
        acc += Y[(size_t)(r0 + dr) * npts + J * lam_step + dj];
        accd += Yd[(size_t)(r0 + dr) * npts + J * lam_step + dj];
      }
    acc /= cnt; accd /= cnt;   // (the value as k_ats_resunit forms it: the same arg-max)
    Dl[J] = acc; Dd[J] = accd;
    if (acc > mx) { mx = acc; js = J; }
  }
  block_argmax(mx, js, red);   // (its barriers publish Dl and Dd)
  const double mxd = Dd[js], ea = e_amps[R];
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double lb = 0.0;
    for (int dj = 0; dj < lam_step; ++dj) lb += lam_nm[J * lam_step + dj];
    lb /= (double)lam_step;
    const bool blue = lb < lam;
    const double u = Dl[J] / mx, ud = (Dd[J] - u * mxd) / mx;
    out_dot[(size_t)R * nJ + J] = ea * (ud * (blue ? amp1 : amp2) + u * (blue ? amp1_dot : amp2_dot));
  }
}

// ---- second-order forward mode of the two row normalisations (tsff_angular_loss_hess; the linear stages run the forward kernels on
// the second-derivative image, as they do on a tangent image) ----
// second derivative of k_ats_rownorm for a pair (a, c) of leaves: Y = B s, s = mM / mB, the maxima where k_ats_rowstats found them
// (the first in index order, positions constant).  With rho_x = s_x / s = M_x[jM] / mM - B_x[jB] / mB and
//   rho_ac = M_ac[jM] / mM - M_a[jM] M_c[jM] / mM^2 - B_ac[jB] / mB + B_a[jB] B_c[jB] / mB^2:
//   Y_ac = B_ac s + B_a s rho_c + B_c s rho_a + B s (rho_a rho_c + rho_ac).
// Ys: the SCALED image Y = B s (k_ats_rownorm has run); Ma, Mc, Mac: the weighted tangent images (before the convolutions);
// Ba, Bc: the UNSCALED convolved tangent images; Bac: B_ac in, Y_ac out.
__global__ __launch_bounds__(kThreads) void k_ats_rownorm_jvp2(const double* __restrict__ Ys, const double* __restrict__ stats,
                                                               const double* __restrict__ Ma, const double* __restrict__ Mc,
                                                               const double* __restrict__ Mac, const double* __restrict__ Ba,
                                                               const double* __restrict__ Bc, int npts, double* __restrict__ Bac) {
  const int r = blockIdx.x;
  const double mM = stats[4 * r], mB = stats[4 * r + 2];
  const int jM = (int)stats[4 * r + 1], jB = (int)stats[4 * r + 3];
  const size_t o = (size_t)r * npts;
  const double sc = mM / mB;
  const double ma = Ma[o + jM] / mM, mc = Mc[o + jM] / mM, ba = Ba[o + jB] / mB, bc = Bc[o + jB] / mB;
  const double rho_a = ma - ba, rho_c = mc - bc;
  const double rho_ac = Mac[o + jM] / mM - ma * mc - Bac[o + jB] / mB + ba * bc;
  __syncthreads();   // (B_ac[jB] is read by every thread before its owner overwrites it)
  const double k = rho_a * rho_c + rho_ac;
  for (int j = threadIdx.x; j < npts; j += kThreads)
    Bac[o + j] = Bac[o + j] * sc + Ba[o + j] * (sc * rho_c) + Bc[o + j] * (sc * rho_a) + Ys[o + j] * k;
}

// second derivative of k_ats_resunit for a pair (a, c) of leaves: out = e_amps u amp, u = D / mx with D the block means and
// mx = D[js] its row maximum (the first in index order), amp = amp1 | amp2 by the wavelength:
//   u_x  = (D_x - u mx_x) / mx,   u_ac = (D_ac - u_a mx_c - u_c mx_a - u mx_ac) / mx,
//   out_ac = e_amps (u_ac amp + u_a amp_c + u_c amp_a + u amp_ac).
// lam, amp1 and amp2 are read from the physical parameters `phys` the value image was formed with (k_ats_resunit's); the amplitudes'
// derivatives w.r.t. the NORMALISED leaves of the slots sa and sc come from the activation of the leaves on the device: amp_x is
// non-zero only when x is that amplitude's own leaf, amp_ac only for a = c = that leaf, through the sigmoid's second derivative.
// `lam` only selects the amplitude.
// Y: the scaled value image; Ya, Yc, Yac: the scaled derivative images, each NULL when identically zero (a leaf that does not reach
// the form factor).  out_a (optional): the first derivative w.r.t. leaf a, written with the diagonal pair.  One workgroup per
// output row; at most TSFF_NBINS resolution units per row.
__global__ __launch_bounds__(kThreads) void k_ats_resunit_jvp2(KStatic S, const double* __restrict__ leaves,
                                                               const double* __restrict__ phys, int sa, int sc,
                                                               const double* __restrict__ Y, const double* __restrict__ Ya,
                                                               const double* __restrict__ Yc, const double* __restrict__ Yac,
                                                               const double* __restrict__ lam_nm, int npts, int lam_step, int ang_step,
                                                               int row_start, const double* __restrict__ e_amps,
                                                               double* __restrict__ out_a, double* __restrict__ out_ac) {
  __shared__ double red[8];
  __shared__ double Dl[TSFF_NBINS], Da[TSFF_NBINS], Dc[TSFF_NBINS], Dac[TSFF_NBINS];
  const int R = blockIdx.x, nJ = npts / lam_step;
  const int r0 = (row_start + R) * ang_step;
  const double cnt = (double)(ang_step * lam_step);
  double mx = -1e300;
  int js = 0;
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double acc = 0.0, acca = 0.0, accc = 0.0, accac = 0.0;
    for (int dr = 0; dr < ang_step; ++dr)
      for (int dj = 0; dj < lam_step; ++dj) {
        const size_t i = (size_t)(r0 + dr) * npts + J * lam_step + dj;
        acc += Y[i];
        if (Ya) acca += Ya[i];
        if (Yc) accc += Yc[i];
        if (Yac) accac += Yac[i];
      }
    acc /= cnt; acca /= cnt; accc /= cnt; accac /= cnt;   // (the value as k_ats_resunit forms it: the same arg-max)
    Dl[J] = acc; Da[J] = acca; Dc[J] = accc; Dac[J] = accac;
    if (acc > mx) { mx = acc; js = J; }
  }
  block_argmax(mx, js, red);   // (its barriers publish the four block-mean rows)
  // lam and the two amplitudes: the values k_ats_resunit read (phys, staged once per call), the amplitudes' first and second
  // derivatives w.r.t. their own normalised leaf from the activation (scale x sigmoid', scale x sigmoid'')
  auto act_d = [&](int s, double& d1, double& d2) {
    if (S.p_sig[s]) {
      const double sg = sigmoid(leaves[s]), d = sg * (1.0 - sg);
      d1 = d * S.p_scale[s]; d2 = d * (1.0 - 2.0 * sg) * S.p_scale[s];
    } else {
      d1 = S.p_scale[s]; d2 = 0.0;
    }
  };
  const double lam = phys[TSFF_P_LAM], amp1 = phys[TSFF_P_AMP1], amp2 = phys[TSFF_P_AMP2];
  double a1d, a1dd, a2d, a2dd;
  act_d(TSFF_P_AMP1, a1d, a1dd);
  act_d(TSFF_P_AMP2, a2d, a2dd);
  const double mxa = Da[js], mxc = Dc[js], mxac = Dac[js], ea = e_amps[R];
  for (int J = threadIdx.x; J < nJ; J += kThreads) {
    double lb = 0.0;
    for (int dj = 0; dj < lam_step; ++dj) lb += lam_nm[J * lam_step + dj];
    lb /= (double)lam_step;
    const bool blue = lb < lam;
    const int own = blue ? TSFF_P_AMP1 : TSFF_P_AMP2;
    const double amp = blue ? amp1 : amp2, ad = blue ? a1d : a2d, add = blue ? a1dd : a2dd;
    const double amp_a = sa == own ? ad : 0.0, amp_c = sc == own ? ad : 0.0, amp_ac = (sa == own && sc == own) ? add : 0.0;
    const double u = Dl[J] / mx;
    const double ua = (Da[J] - u * mxa) / mx, uc = (Dc[J] - u * mxc) / mx;
    const double uac = (Dac[J] - ua * mxc - uc * mxa - u * mxac) / mx;
    out_ac[(size_t)R * nJ + J] = ea * (uac * amp + ua * amp_c + uc * amp_a + u * amp_ac);
    if (out_a) out_a[(size_t)R * nJ + J] = ea * (ua * amp + u * amp_a);
  }
}

// reverse of k_ats_conv: Xbar[i] (+)= sum_s taps[s] Ybar[i - off - s]
__global__ void k_ats_conv_adj(const double* __restrict__ Yb, const double* __restrict__ taps, int nt, int off, int along_rows,
                               int npx, int npts, int accumulate, double* __restrict__ Xb) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (j >= npts) return;
  double acc = 0.0;
  if (along_rows) {
    for (int s = 0; s < nt; ++s) {
      const int rr = r - off - s;
      if (rr >= 0 && rr < npx) acc += taps[s] * Yb[(size_t)rr * npts + j];
    }
  } else {
    for (int s = 0; s < nt; ++s) {
      const int jj = j - off - s;
      if (jj >= 0 && jj < npts) acc += taps[s] * Yb[(size_t)r * npts + jj];
    }
  }
  double* o = Xb + (size_t)r * npts + j;
  *o = accumulate ? *o + acc : acc;
}

// reverse of k_ats_weights: Pbar[g][j][a] = filt[j] / G * sum_r Wt[r][a] Mbar[r][j]
__global__ void k_ats_weights_adj(const double* __restrict__ Mbar, const double* __restrict__ Wt, const double* __restrict__ filt,
                                  int G, int npts, int NA, int npx, double* __restrict__ Pbar) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
  if (a >= NA) return;
  double acc = 0.0;
  for (int r = 0; r < npx; ++r) {
    const double w = Wt[(size_t)r * NA + a];
    if (w != 0.0) acc += w * Mbar[(size_t)r * npts + j];
  }
  acc *= (filt ? filt[j] : 1.0) / (double)G;
  for (int g = 0; g < G; ++g) Pbar[((size_t)g * npts + j) * NA + a] = acc;
}
