// k_sph.inc -- the SphericalHarmonics f_e generator (tsadar_amd.distribution.SphericalHarmonics.__call__) and its adjoint on
// the device: tsff_sph_table, tsff_sph_table_vjp and the TSFF_ANG_SPH generator of tsff_angular_fit.
//   theta (get_params() order): per harmonic (l, m) in sorted order -- Mora-Yahi: log_10_LT; free radial functions: flm_sign[nvr],
//   flm_mag[nvr] --, then normed_m (the order of f00 before its sigmoid).
//   forward: m = 3 sigmoid(normed_m) + 2 -> f00(vr) (get_f00: super-Gaussian, normalised over vr) -> the radial functions
//   (FLM_MY, or 10^(-10 sigmoid(M mag)) tanh(M sign) with M the Hanning smoothing matrix) -> linear interpolation onto the grid
//   points (np.interp: cell, weight and inside flag precomputed, right = 1e-16 / 1e-32) -> times Re Y_l^m (precomputed) -> floor
//   at 1e-32 -> / (sum f dv^2).
//   adjoint: fbar = (fe_bar / tot - sum(fe_bar fc) / tot^2) / dv^2 on the live points, then
//     log_10_LT : closed form, d flm / d LT = -ln 10 flm (the radial function is linear in 10^-LT);
//     normed_m  : the tangent of f00 (and of FLM_MY's coefficient) in m, exact -- digamma by recurrence + asymptotic series --,
//                 interpolated like the radial functions and contracted with fbar, times 3 sigmoid';
//     flm_sign, flm_mag: the transposed interpolation onto the radial nodes over a host-built CSR list of (point, weight) per
//                 node, one wavefront per (harmonic, node) in list order, then the tanh / 10^ / sigmoid derivatives and M^T.
// One workgroup of kThreads; every sum runs in a fixed order (thread-strided partials, wave_sum, block_sum): the results are
// bit-reproducible from run to run, and nothing is accumulated atomically.
//
// gen_data (doubles; n2 = nv^2, H harmonics): vr[nvr] | cell[n2] | wt[n2] | inside[n2] | Y[H][n2] and, for the free radial
// functions, | M[nvr][nvr] | ptr[nvr + 1] | pt[2 n2] | cw[2 n2] (CSR: the entries of node k are ptr[k] .. ptr[k + 1]; integers are
// stored as doubles).  ws (scratch): f00 | df00 | 6 arrays [H][nvr] | fbar[n2] (the adjoint only).
struct SphGen {
  int type, H, nv, nvr;
  const double *vr, *cell, *wt, *ins, *Y, *M, *ptr, *pt, *cw;
};

constexpr int kSphMaxH = 64;   // harmonics of a generator (Nl <= 9)

inline size_t sph_ws_doubles(int H, int nv, int nvr) { return (size_t)(2 + 6 * H) * nvr + (size_t)nv * nv; }

inline SphGen sph_gen(int type, int H, int nv, int nvr, const double* g) {
  const size_t n2 = (size_t)nv * nv;
  SphGen G{type, H, nv, nvr, g, g + nvr, g + nvr + n2, g + nvr + 2 * n2, g + nvr + 3 * n2, nullptr, nullptr, nullptr, nullptr};
  if (type == TSFF_SPH_ARBITRARY) {
    G.M = G.Y + (size_t)H * n2;
    G.ptr = G.M + (size_t)nvr * nvr;
    G.pt = G.ptr + nvr + 1;
    G.cw = G.pt + 2 * n2;
  }
  return G;
}

// psi(x), x > 0: psi(x) = psi(x + 1) - 1 / x up to x >= 10, then ln x - 1 / (2 x) - sum_k B_2k / (2 k x^2k) (k <= 7: the first
// term left out is 3617 / (8160 x^16) < 5e-17)
__device__ __forceinline__ double sph_digamma(double x) {
#pragma clang fp contract(off)
  double s = 0.0;
  while (x < 10.0) { s -= 1.0 / x; x += 1.0; }
  const double r = 1.0 / x, r2 = r * r;
  const double t = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 - r2 * (691.0 / 32760 - r2 * (1.0 / 12)))))));
  return s + ((log(x) - 0.5 * r) - t);
}

// scalars of the order m, by thread 0 into LDS
enum { SPH_M, SPH_DMDN, SPH_V0, SPH_A, SPH_DLNV0, SPH_VE, SPH_DLNVE, SPH_R, SPH_DLNR, SPH_NSC };

// the radial stage: f00 and the radial functions on vr (tangent: also their derivatives in m) into ws; sc: LDS [SPH_NSC],
// red: LDS [8].  Ends with a barrier: ws is readable by every thread.
__device__ __forceinline__ void sph_radial(const SphGen& G, const double* __restrict__ theta, int n_gen, bool tangent,
                                           double* __restrict__ ws, double* sc, double* red) {
#pragma clang fp contract(off)
  const int nvr = G.nvr, H = G.H;
  double* f00 = ws;
  double* df00 = ws + nvr;
  double* rad = ws + 2 * (size_t)nvr;
  double* A1 = rad + (size_t)H * nvr;   // Mora-Yahi: d rad / d m; free: tanh(M sign)
  double* A2 = A1 + (size_t)H * nvr;    // free: sigmoid(M mag)
  double* A3 = A2 + (size_t)H * nvr;    // free: 10^(-10 sigmoid)
  if (threadIdx.x == 0) {
    const double sg = sigmoid(theta[n_gen - 1]);
    const double m = sg * 3.0 + 2.0;
    const double g3 = tgamma(3.0 / m), g5 = tgamma(5.0 / m);
    const double v0 = 1.0 / sqrt(g5 / 3.0 / g3);
    sc[SPH_M] = m;
    sc[SPH_DMDN] = 3.0 * (sg * (1.0 - sg));
    sc[SPH_V0] = v0;
    sc[SPH_A] = m / (4.0 * kPi * g3) / (v0 * v0 * v0);
    sc[SPH_VE] = g5 / 3.0 / g3;
    sc[SPH_R] = tgamma(8.0 / m) / tgamma(6.0 / m);
    if (tangent) {   // d ln Gamma(a / m) / d m = psi(a / m) (-a / m^2)
      const double m2 = m * m;
      const double d3 = sph_digamma(3.0 / m) * (-3.0 / m2), d5 = sph_digamma(5.0 / m) * (-5.0 / m2);
      sc[SPH_DLNVE] = d5 - d3;
      sc[SPH_DLNV0] = -0.5 * (d5 - d3);
      sc[SPH_DLNR] = sph_digamma(8.0 / m) * (-8.0 / m2) - sph_digamma(6.0 / m) * (-6.0 / m2);
    }
  }
  __syncthreads();
  const double m = sc[SPH_M], v0 = sc[SPH_V0], dvr = G.vr[1] - G.vr[0];
  // get_f00: e = A exp(-(v / v0)^m), f00 = e / (sum(e 4 pi v^2) dvr); s = d ln e / d m up to a constant (which the normalisation
  // cancels) = -(v / v0)^m (ln(v / v0) - m d ln v0 / d m)
  double acc = 0.0;
  for (int k = threadIdx.x; k < nvr; k += kThreads) {
    const double v = G.vr[k], x = v / v0, pw = pow(x, m);
    const double e = sc[SPH_A] * exp(-pw);
    f00[k] = e;
    acc += ((e * 4.0) * kPi) * (v * v);
    if (tangent) df00[k] = -(pw * (log(x) - m * sc[SPH_DLNV0]));
  }
  const double N = block_sum(acc, red) * dvr;
  acc = 0.0;
  for (int k = threadIdx.x; k < nvr; k += kThreads) {
    const double v = G.vr[k], f = f00[k] / N;
    f00[k] = f;
    if (tangent) acc += (((f * 4.0) * kPi) * (v * v)) * df00[k];
  }
  if (tangent) {
    const double mean = block_sum(acc, red) * dvr;
    for (int k = threadIdx.x; k < nvr; k += kThreads) df00[k] = f00[k] * (df00[k] - mean);
  }
  __syncthreads();
  if (G.type == TSFF_SPH_MORA_YAHI) {   // FLM_MY.__call__ (Mora & Yahi 1982, eq. 3)
    const double ve = sc[SPH_VE], R = sc[SPH_R];
    for (int i = threadIdx.x; i < H * nvr; i += kThreads) {
      const int h = i / nvr, k = i - h * nvr;
      const double v = G.vr[k], lam_v = pow(v / ve, 4.0), vm = pow(v, m), vm2 = pow(v, m - 2.0);
      const double c1 = (m / 2.0) * vm, c2 = (((5.0 * m) / 12.0) * R) * vm2;
      const double co = ((c1 - c2) - 1.5) * lam_v, lt = pow(10.0, theta[h]);
      rad[i] = (co / lt) * f00[k];
      if (tangent) {
        const double lnv = log(v);
        const double dc1 = 0.5 * vm + c1 * lnv, dc2 = c2 / m + c2 * sc[SPH_DLNR] + c2 * lnv;
        const double dco = (dc1 - dc2) * lam_v + ((c1 - c2) - 1.5) * (lam_v * (-4.0 * sc[SPH_DLNVE]));
        A1[i] = (dco * f00[k] + co * df00[k]) / lt;
      }
    }
  } else {   // ArbitraryVr.__call__: 10^(-10 sigmoid(M mag)) tanh(M sign)
    for (int i = threadIdx.x; i < H * nvr; i += kThreads) {
      const int h = i / nvr, k = i - h * nvr;
      const double* sign = theta + (size_t)h * 2 * nvr;
      const double* mag = sign + nvr;
      const double* Mk = G.M + (size_t)k * nvr;
      double sv = 0.0, su = 0.0;
      for (int j = 0; j < nvr; ++j) { sv += Mk[j] * sign[j]; su += Mk[j] * mag[j]; }
      const double sg = 1.0 / (1.0 + exp(-su)), p10 = pow(10.0, -sg * 10.0), th = tanh(sv);
      rad[i] = p10 * th;
      A1[i] = th;
      A2[i] = sg;
      A3[i] = p10;
    }
  }
  __syncthreads();
}

// np.interp of a radial array at grid point p (inside the radial axis)
__device__ __forceinline__ double sph_lerp(const double* __restrict__ a, int i, double w) { return a[i] + w * (a[i + 1] - a[i]); }

// f(p) before the floor: interp(f00) + sum_h interp(rad_h) Y_h
__device__ __forceinline__ double sph_point(const SphGen& G, const double* __restrict__ ws, long p, long n2) {
#pragma clang fp contract(off)
  const int nvr = G.nvr, i = (int)G.cell[p];
  const double w = G.wt[p];
  const bool in = G.ins[p] != 0.0;
  const double* rad = ws + 2 * (size_t)nvr;
  double f = in ? sph_lerp(ws, i, w) : 1e-16;
  for (int h = 0; h < G.H; ++h) f = f + (in ? sph_lerp(rad + (size_t)h * nvr, i, w) : 1e-32) * G.Y[(size_t)h * n2 + p];
  return f;
}

__global__ __launch_bounds__(kThreads) void k_sph_table(SphGen G, const double* __restrict__ theta, int n_gen, double dv2,
                                                        double* __restrict__ ws, double* __restrict__ fe) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ double sc[SPH_NSC];
  sph_radial(G, theta, n_gen, false, ws, sc, red);
  const long n2 = (long)G.nv * G.nv;
  double s = 0.0;
  for (long p = threadIdx.x; p < n2; p += kThreads) {
    const double f = fmax(sph_point(G, ws, p, n2), 1e-32);
    fe[p] = f;
    s += f;
  }
  s = block_sum(s, red) * dv2;
  for (long p = threadIdx.x; p < n2; p += kThreads) fe[p] = fe[p] / s;
}

// grad[n_gen] = d loss / d theta from fe_bar = d loss / d f_e[nv][nv]
__global__ __launch_bounds__(kThreads) void k_sph_vjp(SphGen G, const double* __restrict__ theta, int n_gen, double cvjp, double ln10,
                                                      const double* __restrict__ fe_bar, double* __restrict__ ws,
                                                      double* __restrict__ grad) {
#pragma clang fp contract(off)
  __shared__ double red[8];
  __shared__ double sc[SPH_NSC];
  sph_radial(G, theta, n_gen, true, ws, sc, red);
  const int nvr = G.nvr, H = G.H;
  const long n2 = (long)G.nv * G.nv;
  const double* df00 = ws + nvr;
  const double* rad = ws + 2 * (size_t)nvr;
  double* A1 = ws + (2 + (size_t)H) * nvr;
  double* A2 = A1 + (size_t)H * nvr;
  double* A3 = A2 + (size_t)H * nvr;
  double* GS = A3 + (size_t)H * nvr;   // free radial functions: the adjoints of M sign and M mag
  double* GM = GS + (size_t)H * nvr;
  double* fbar = GM + (size_t)H * nvr;
  // the normalisation and the floor: fe = fc / (tot dv^2), fc = max(f, 1e-32)
  double tot = 0.0, dot = 0.0;
  for (long p = threadIdx.x; p < n2; p += kThreads) {
    const double f = sph_point(G, ws, p, n2), fc = fmax(f, 1e-32);
    fbar[p] = f;
    tot += fc;
    dot += fe_bar[p] * fc;
  }
  tot = block_sum(tot, red);
  dot = block_sum(dot, red);
  const double q = dot / (tot * tot);
  const bool my = G.type == TSFF_SPH_MORA_YAHI;
  double gm = 0.0, g0 = 0.0, g1 = 0.0;
  for (long p = threadIdx.x; p < n2; p += kThreads) {
    const double fb = fbar[p] > 1e-32 ? cvjp * (fe_bar[p] / tot - q) : 0.0;
    fbar[p] = fb;
    if (G.ins[p] != 0.0) {   // (outside the radial axis the interpolant is a constant)
      const int i = (int)G.cell[p];
      const double w = G.wt[p];
      double dF = sph_lerp(df00, i, w);
      if (my) {   // H == 2
        const double y0 = G.Y[p], y1 = G.Y[n2 + p];
        dF = dF + sph_lerp(A1, i, w) * y0;
        dF = dF + sph_lerp(A1 + nvr, i, w) * y1;
        g0 += (fb * y0) * sph_lerp(rad, i, w);
        g1 += (fb * y1) * sph_lerp(rad + nvr, i, w);
      }
      gm += fb * dF;
    }
  }
  gm = block_sum(gm, red);
  if (my) {
    g0 = block_sum(g0, red);
    g1 = block_sum(g1, red);
    if (threadIdx.x == 0) { grad[0] = -ln10 * g0; grad[1] = -ln10 * g1; }
  }
  if (threadIdx.x == 0) grad[n_gen - 1] = gm * sc[SPH_DMDN];
  if (my) return;
  __syncthreads();   // fbar is complete
  // transposed interpolation: one wavefront per (harmonic, node), its list in order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int task = wv; task < H * nvr; task += kThreads / 64) {
    const int h = task / nvr, k = task - h * nvr;
    const long e0 = (long)G.ptr[k], e1 = (long)G.ptr[k + 1];
    const double* Yh = G.Y + (size_t)h * n2;
    double acc = 0.0;
    for (long e = e0 + lane; e < e1; e += 64) {
      const long p = (long)G.pt[e];
      acc += (fbar[p] * Yh[p]) * G.cw[e];
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      const double th = A1[task], sg = A2[task], p10 = A3[task];
      GS[task] = (acc * p10) * (1.0 - th * th);
      GM[task] = (((acc * rad[task]) * ln10) * (-10.0)) * (sg * (1.0 - sg));
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * H * nvr; i += kThreads) {   // M^T
    const int h = i / (2 * nvr), r = i - h * 2 * nvr, j = r % nvr;
    const double* g = (r < nvr ? GS : GM) + (size_t)h * nvr;
    double s = 0.0;
    for (int k = 0; k < nvr; ++k) s += G.M[(size_t)k * nvr + j] * g[k];
    grad[i] = s;
  }
}
