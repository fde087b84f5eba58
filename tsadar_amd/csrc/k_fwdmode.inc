// k_fwdmode.inc -- what the forward-mode kernels share: the chain of one (sample, angle, gradient point), written once over the
// number type N.  Part of the single translation unit tsff_kernels.hip (included inside namespace tsff, in front of k_hessian.inc).  The kernels: k_hess_pairs (N = HD, k_hessian.inc), k_jac_sweep (TN<W>,
// k_jacobian.inc), k_ffjvp (TN<W>, k_ffjvp.inc).  DESIGN.md sections 4.4, 4.4b, 4.4c.
//
// N supplies N::of(double), the member v, the arithmetic operators with N and with double, hd_chain and hd_xm, kSecondOrder (whether
// the second-order table terms are read) and kLanes (tangent lanes that may carry a table direction of their own).
//
// Table convention (the reference's, which the torch twin follows): the piecewise-linear Z' and W lookups carry their slope and
// no curvature; the cubic Hermite ln f_e lookup carries its true second derivative; the Z' asymptote xi^-2 and exp(-xi^2) are
// differentiated exactly.

// The generic forms of 1/x, sqrt, exp and the sigmoid from hd_chain (IEEE division, library sqrt and exp); a number type with faster
// forms of its own overloads them (TN<W>)
template <class N>
__device__ __forceinline__ N hd_rcp(N x) {
  const double r = 1.0 / x.v;
  return hd_chain(x, r, -r * r, 2.0 * r * r * r);
}
template <class N>
__device__ __forceinline__ N hd_sqrt(N x) {
  const double s = sqrt(x.v);
  return hd_chain(x, s, 0.5 / s, -0.25 / (s * x.v));
}
template <class N>
__device__ __forceinline__ N hd_exp(N x) {
  const double e = exp(x.v);
  return hd_chain(x, e, e, e);
}
template <class N>
__device__ __forceinline__ N hd_sigmoid(N x) {
  const double s = sigmoid(x.v), d = s * (1.0 - s);
  return hd_chain(x, s, d, d * (1.0 - 2.0 * s));
}

// lineout scalars of one gradient point (make_lines) in the number type
template <class N, int NI>
struct LineT {
  N wpe2, wL, kL, ivTe, a_e, pref, Ud, Vd, i2wL;
  N ixi[NI], a_i[NI], cs[NI], hai[NI];
};

// ph: physical parameters [NP] (after activation, Ti tying and fraction renormalisation), as make_lines reads them
template <int NI, class N>
__device__ __forceinline__ void make_lines_hd(const N* ph, double lam_shift, int g, int G, LineT<N, NI>& L) {
  const double cg = grad_coef(g, G);
  const N ne_g = (1.0e20 * ph[TSFF_P_NE]) * (1.0 + ph[TSFF_P_NE_GRADIENT] * cg);
  const N Te_g = ph[TSFF_P_TE] * (1.0 + ph[TSFF_P_TE_GRADIENT] * cg);
  L.wL = kOmgLnum / (ph[TSFF_P_LAM] + lam_shift);
  L.i2wL = 2.0 / L.wL;
  L.wpe2 = kC0sq * ne_g;
  L.kL = hd_sqrt(L.wL * L.wL - L.wpe2) * (1.0 / kC);
  L.ivTe = 1.0 / hd_sqrt(Te_g * (1.0 / kMe));
  L.a_e = L.wpe2 * L.ivTe * L.ivTe;
  L.pref = ne_g * (kRe * kRe / (2.0 * kPi * kC));
  L.Ud = ph[TSFF_P_UD] * 1e6;
  L.Vd = ph[TSFF_P_VA] * 1e6;
  N Zbar = N::of(0.0);
#pragma unroll
  for (int s = 0; s < NI; ++s) Zbar = Zbar + ph[TSFF_P_ION0 + 4 * s + TSFF_ION_Z] * ph[TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT];
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    const int o = TSFF_P_ION0 + 4 * s;
    const N Ti = ph[o + TSFF_ION_TI], Z = ph[o + TSFF_ION_Z], fr = ph[o + TSFF_ION_FRACT];
    const double Ms = ph[o + TSFF_ION_A].v * kMp;
    const N vTi = hd_sqrt(Ti * (1.0 / Ms));
    L.ixi[s] = 1.0 / (kSqrt2 * vTi);
    L.a_i[s] = (kC0sq * kMe) * Z * Z * fr * ne_g / (Zbar * Ti);
    L.cs[s] = fr * Z * Z / (Zbar * vTi);
    L.hai[s] = -0.5 * L.a_i[s];
  }
}

template <class N>
struct BaseT {
  N ik, wd, xe, F;
};

// the tables' dependence on the DLM order m (with_m): dW/dm, d2W/dm2 on the xi2 grid and the Hermite coefficients of
// d ln f_e / dm and d2 ln f_e / dm2; m is the physical order with its two seeds
// The general case of a first-order number with tangent lanes (N::kLanes > 0, k_ffjvp): lane k < nlane carries a table direction
// of its own, Wd[k][1640] = the tangent of W and hcd[k][2 nvx] = the Hermite coefficients of the tangent of ln f_e along it, which
// the lookups add to that lane directly.  m is the special case of one direction shared by every lane through m's seeds.
template <class N>
struct MTabT {
  const double* Wm;
  const double* Wmm;     // (second order only)
  const double2* hcm;
  const double2* hcmm;   // (second order only)
  N m;
  bool on;
  int nlane = 0;         // lanes with a table direction (0: none)
  const double* Wd = nullptr;
  const double2* hcd = nullptr;
  int hstride = 0;       // double2 per lane of hcd (2 nvx)
};
__device__ __forceinline__ void cubic_at(const double2* hc, int i, double t, double idv, double& H, double& d1, double& d2) {
  const double2 c01 = hc[2 * i], c23 = hc[2 * i + 1];
  H = __builtin_fma(t, __builtin_fma(t, __builtin_fma(t, c23.y, c23.x), c01.y), c01.x);
  d1 = __builtin_fma(t, __builtin_fma(3.0 * t, c23.y, 2.0 * c23.x), c01.y) * idv;
  d2 = __builtin_fma(6.0 * t, c23.y, 2.0 * c23.x) * (idv * idv);
}

// hermite_lookup_c with the true second derivative of the cubic (-50 and no derivative outside the grid); with M.on the
// node values depend on m as well
template <class N>
__device__ __forceinline__ N hermite_hd(const Tables& T, const MTabT<N>& M, N x) {
  const double u = __builtin_fma(x.v, T.idv, T.u0);
  const double uc = fmin(fmax(u, 0.0), T.utop);
  if (u != uc) return N::of(-50.0);
  const double fl = __builtin_floor(uc);
  const double t = uc - fl;
  const int i = (int)fl;
  double H, d1, d2;
  cubic_at(T.hc, i, t, T.idv, H, d1, d2);
  if constexpr (N::kLanes > 0) {
    if (M.nlane > 0) {
      N r = hd_chain(x, H, d1, d2);
#pragma unroll
      for (int k = 0; k < N::kLanes; ++k)
        if (k < M.nlane) {
          double Hk, u1, u2;
          cubic_at(M.hcd + (size_t)k * M.hstride, i, t, T.idv, Hk, u1, u2);
          r.d[k] += Hk;
        }
      return r;
    }
  }
  if (!M.on) return hd_chain(x, H, d1, d2);
  double Hm, Hxm, unused, Hmm = 0.0, u1, u2;
  cubic_at(M.hcm, i, t, T.idv, Hm, Hxm, unused);
  if constexpr (N::kSecondOrder) cubic_at(M.hcmm, i, t, T.idv, Hmm, u1, u2);
  return hd_xm(x, M.m, H, d1, Hm, d2, Hxm, Hmm);
}

template <int NI, class N>
__device__ __forceinline__ void base_hd(double ws, double ct, const LineT<N, NI>& L, const Tables& T, const MTabT<N>& M, BaseT<N>& b) {
  const N ks = hd_sqrt(ws * ws - L.wpe2) * (1.0 / kC);
  const N k2 = ks * (ks - (2.0 * ct) * L.kL) + L.kL * L.kL;
  const N k = hd_sqrt(k2);
  b.ik = hd_rcp(k);
  b.wd = (ws - L.wL) - k * L.Vd;
  b.xe = (b.wd * b.ik - L.Ud) * L.ivTe;
  b.F = hd_exp(hermite_hd(T, M, b.xe));
}

// point_core / point_forward_sd in the number type: S (1 + 2 w / w_L)
template <int NI, class N>
__device__ __forceinline__ N point_hd(const BaseT<N>& b, const BaseT<N>& bn, bool has_next, const LineT<N, NI>& L, const Tables& T,
                                     const MTabT<N>& M) {
  const N ik2 = b.ik * b.ik;
  const N ike2 = L.a_e * ik2;
  const N vph = b.wd * b.ik;
  N opc = N::of(1.0), cim = N::of(0.0), gsum = N::of(0.0);
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    const N xi = vph * L.ixi[s];
    const N hk = L.hai[s] * ik2;
    // Z'(xi): the full table (slope, no curvature) or the asymptote xi^-2 + 0 i outside it
    constexpr double kTop = (double)(kNXi2 - 1) * (1.0 - 1.1102230246251565e-16);
    const double u = __builtin_fma(xi.v, kXi2_ih, -kXi2_0 * kXi2_ih);
    const double uc = fmin(fmax(u, 0.0), kTop);
    N zr, zi;
    if (u != uc) {
      const double r = 1.0 / xi.v, r2 = r * r;
      zr = hd_chain(xi, r2, -2.0 * r2 * r, 6.0 * r2 * r2);
      zi = N::of(0.0);
    } else {
      const double fl = __builtin_floor(uc);
      const double t = uc - fl;
      const int i = (int)fl;
      const double2 za = T.zp[i], zb = T.zp[i + 1];
      const double dr = zb.x - za.x, di = zb.y - za.y;
      zr = hd_chain(xi, __builtin_fma(t, dr, za.x), dr * kXi2_ih, 0.0);
      zi = hd_chain(xi, __builtin_fma(t, di, za.y), di * kXi2_ih, 0.0);
    }
    const N gs = hd_exp(-(xi * xi)) * kInvSqrt2Pi;
    opc = opc + hk * zr;
    cim = cim + hk * zi;
    gsum = gsum + L.cs[s] * gs;
  }
  double w, dw;
  w_lookup(T.W, b.xe.v, w, dw);
  N Wl;
  bool lanes = false;
  if constexpr (N::kLanes > 0) lanes = M.nlane > 0;
  if (lanes) {   // W(x) with a table tangent per lane, interpolated in the same cell
    Wl = hd_chain(b.xe, w, dw, 0.0);
    if constexpr (N::kLanes > 0) {
#pragma unroll
      for (int k = 0; k < N::kLanes; ++k)
        if (k < M.nlane) {
          double wk, dwk;
          w_lookup(M.Wd + (size_t)k * kNXi2, b.xe.v, wk, dwk);
          Wl.d[k] += wk;
        }
    }
  } else if (M.on) {   // W(x, m): no curvature in x; dW/dm and d2W/dm2 interpolated in the same cell, the slope of dW/dm for the mixed term
    double wm, dwm, wmm = 0.0, dwmm;
    w_lookup(M.Wm, b.xe.v, wm, dwm);
    if constexpr (N::kSecondOrder) w_lookup(M.Wmm, b.xe.v, wmm, dwmm);
    Wl = hd_xm(b.xe, M.m, w, dw, wm, 0.0, dwm, wmm);
  } else {
    Wl = hd_chain(b.xe, w, dw, 0.0);
  }
  const N D = has_next ? (bn.F - b.F) / (bn.xe - b.xe) : N::of(0.0);
  const N cer = -(ike2 * Wl);
  const N cei = (kPi * ike2) * D;
  const N er = opc + cer, ei = cei + cim;
  const N eps2 = er * er + ei * ei;
  const N ce2 = cer * cer + cei * cei;
  const N ci2 = opc * opc + cim * cim;
  const N Nn = gsum * ce2 + ci2 * b.F * L.ivTe;
  const N S = Nn * b.ik / eps2;
  return S * (1.0 + b.wd * L.i2wL);
}

// Ti tying and fraction renormalisation of the physical parameters (the tail of stage_phys)
template <int NI, class N>
__device__ __forceinline__ void tie_and_renorm(const KStatic& S, N* ph) {
  N fsum = N::of(0.0);
  for (int s = 0; s < NI; ++s) {
    const int o = TSFF_P_ION0 + 4 * s;
    if (s > 0 && S.ti_same[s]) ph[o + TSFF_ION_TI] = ph[TSFF_P_ION0 + TSFF_ION_TI];
    fsum = fsum + ph[o + TSFF_ION_FRACT];
  }
  const N ifs = hd_rcp(fsum);
  for (int s = 0; s < NI; ++s) ph[TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT] = ph[TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT] * ifs;
}
