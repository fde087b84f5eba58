// k_pairs.inc -- what the pair-sweep kernels share: k_spectrum_fused, k_forward_pairs and k_spectrum_rows walk pairs of consecutive
// samples per thread, one angle loop per pair, the right neighbour's base point taken from the next lane and the asymptotic ion terms
// per 128-sample unit.  The per-point functions of the one-sweep reverse and every step of that sweep that is the same text in two or
// three of the kernels live here, once; the angle loops themselves stay written out in each kernel (a shared skeleton cost spills).
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff, in front of k_spectrum_fused.inc).

// point_reverse with the seed PQ = w_a pref (no spectrum adjoint yet): returns S (1 + 2w/wL), whose PQ-fold is the contribution
// to x_j (before the factor ws^2), the adjoints of this point's base quantities (ba) and of the right neighbour's (xi_e, F),
// and accumulates the direct lineout-scalar adjoints into the row J.  cw = -i2wL^2 / 2 folds the adjoint of 2/wL into wL.
// The deferred factor of a_i (x -1/2) is applied after the contraction (see the kernel); pref's adjoint is x_j itself.
// point_fused_reverse is the reverse alone, of a point whose forward quantities pf the caller has (point_core, or its three steps:
// pair_step_sched); point_fused is point_core followed by it.
template <int NI, int GM, bool FAR = false>
__device__ __forceinline__ double point_fused_reverse(const PointF<NI>& pf, const Base& b, const LineS<NI>& L, const Tables& T,
                                                      double PQ, double cw, BaseAdj& ba, double& xen, double& Fn, LineS<NI>& J) {
  const double ik2 = pf.ik2, ike2 = pf.ike2, vph = pf.vph, gsum = pf.gsum, Wl = pf.Wl, dW = pf.dW, idx = pf.idx, D = pf.D;
  const double cer = pf.cer, cei = pf.cei, opc = pf.opc, cim = pf.cim, er = pf.er, ei = pf.ei, ieps2 = pf.ieps2, ce2 = pf.ce2, ci2 = pf.ci2;
  const double N = pf.N, t1 = pf.t1, S = pf.S, dop = pf.dop;
  const double* xi = pf.xi; const double* zr = pf.zr; const double* zi = pf.zi; const double* dzr = pf.dzr; const double* dzi = pf.dzi;
  const double* hk = pf.hk; const double* gs = pf.gs;
  // ---- reverse with the seed PQ ----
  const double Sb = PQ * dop;
  const double PSQ = PQ * S;
  const double fwd = S * dop;   // (x PQ by the caller: the association of k_spectrum's forward sweep, bit for bit)
  J.wL = __builtin_fma(PSQ * b.wd, cw, J.wL);
  const double Nb = Sb * t1;
  const double ikb0 = Sb * N * ieps2;
  const double e2 = -2.0 * (ikb0 * t1);
  const double NbI = Nb * L.ivTe;
  const double ci2b2 = 2.0 * (NbI * b.F);
  ba.F = NbI * ci2;
  J.ivTe += (Nb * ci2) * b.F;
  const double erb = e2 * er, eib = e2 * ei;
  double cerb = erb, ceib = eib, cimb = eib;
  if (!FAR) {   // (FAR: gsum = 0 and Im chi_i = 0 identically)
    const double ce2b2 = 2.0 * (Nb * gsum);       // 2 x adjoint of |chi_e|^2
    cerb = erb + ce2b2 * cer; ceib = eib + ce2b2 * cei;
    cimb = eib + ci2b2 * cim;
  }
  const double creb = erb + ci2b2 * opc;
  const double cp = ceib * kPi;
  const double ike2b = cp * D - cerb * Wl;
  const double Wlb = -cerb * ike2;
  ba.xe = Wlb * dW;
  if (GM == 1) {
    double Wml, dWm;
    w_lookup(T.Wm, b.xe, Wml, dWm);
    J.m += Wlb * Wml;
  }
  Fn = (cp * ike2) * idx;
  ba.F -= Fn;
  xen = -Fn * D;
  ba.xe -= xen;
  double k2acc = 0.0, vphb = 0.0;
  const double u = FAR ? 0.0 : Nb * ce2;
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    double w, xib;
    if (FAR) {   // gs = Im Z' = d Im Z' = 0
      w = creb * zr[s];
      xib = hk[s] * (creb * dzr[s]);
    } else {
      const double v = u * gs[s];
      J.cs[s] += v;
      w = creb * zr[s] + cimb * zi[s];
      xib = -2.0 * (v * xi[s] * L.cs[s]) + hk[s] * (creb * dzr[s] + cimb * dzi[s]);
    }
    const double wk = w * ik2;
    J.a_i[s] += wk;
    k2acc += wk * hk[s];
    vphb += xib * L.ixi[s];
    J.ixi[s] += xib * vph;
  }
  const double we = ike2b * ik2;
  J.a_e += we;
  ba.k2 = -k2acc - we * ike2;
  ba.wd = PSQ * L.i2wL + vphb * b.ik;
  ba.ik = ikb0 + vphb * b.wd;
  return fwd;
}
template <int NI, int GM, bool ZH, bool FAR = false>
__device__ __forceinline__ double point_fused(const Base& b, const Base& bn, bool has_next, const LineS<NI>& L, const Tables& T,
                                              double PQ, double cw, BaseAdj& ba, double& xen, double& Fn, LineS<NI>& J) {
  // ---- forward (form_factor.py:243-296) ----
  PointF<NI> pf;
  point_core<NI, ZH, FAR>(b, bn, has_next, L, T, pf);
  return point_fused_reverse<NI, GM, FAR>(pf, b, L, T, PQ, cw, ba, xen, Fn, J);
}

// The adjoint of k^2 = k_s^2 + k_L^2 - 2 k_s k_L cos(theta) flows to k_L and, through k_s(lambda), to omega_pe^2:
//   kLbar += k22 (k_L - k_s ct),   wpe2bar -= k22 (k_s - k_L ct) / (2 c^2 k_s),      k22 = 2 x adjoint of k^2.
// k_s depends on the wavelength sample only and ct = cos(theta_a) on the angle only, so a row accumulates P1 = sum_a k22 and
// P2 = sum_a k22 ct per base point (its own sample and the right neighbour) -- two instructions per base where the direct form
// took ten, a reciprocal of k_s among them -- and the two columns are assembled once per sample after the angle loop:
//   kLbar = k_L (P1a + P1b) - (k_s,j P2a + k_s,j+1 P2b),   wpe2bar = -[P1a + P1b - k_L (P2a / k_s,j + P2b / k_s,j+1)] / (2 c^2).
struct KsAcc { double p1a, p2a, p1b, p2b; };

// base_reverse (tsff_device.h) without its k_L / omega_pe^2 tail: returns k22
template <int NI, int GM, bool PAD = false>
__device__ __forceinline__ double base_reverse_fused(const Base& b, const LineS<NI>& L, const Tables& T, const BaseAdj& ba,
                                                     LineS<NI>& LB) {
  const double Hb = ba.F * b.F;  // adjoint of H = ln f_e(xi_e)
  if (GM == 1) {  // d ln f_e(xi_e)/dm: Hermite interpolant of the tangent table (zero outside the vx grid)
    Tables Tm = T;
    Tm.hc = T.hcm;
    double Hm, dHm;
    hermite_lookup_c<PAD>(Tm, b.xe, Hm, dHm);
    LB.m += (b.xe < T.vx0 || b.xe > T.vxlast) ? 0.0 : Hb * Hm;
  }
  const double xeb = ba.xe + Hb * b.dH;
  const double vph = b.wd * b.ik, k = b.k2 * b.ik;
  const double vphb = xeb * L.ivTe;
  LB.Ud -= vphb;
  LB.ivTe += xeb * (vph - L.Ud);
  const double wdb = ba.wd + vphb * b.ik;
  const double ikb = ba.ik + vphb * b.wd;
  LB.wL -= wdb;
  LB.Vd -= wdb * k;
  const double kb = wdb * L.Vd + ikb * (b.ik * b.ik);
  return 2.0 * ba.k2 - kb * b.ik;
}

// the same for a base point that receives adjoints of (xi_e, F) only: the right neighbour of a point, through the finite
// difference D = (F_{j+1} - F_j)/(xi_{e,j+1} - xi_{e,j})
template <int NI, int GM, bool PAD = false>
__device__ __forceinline__ double base_reverse_xf(const Base& b, const LineS<NI>& L, const Tables& T, double xeb_in, double Fb,
                                                  LineS<NI>& LB) {
  const double Hb = Fb * b.F;
  if (GM == 1) {
    Tables Tm = T;
    Tm.hc = T.hcm;
    double Hm, dHm;
    hermite_lookup_c<PAD>(Tm, b.xe, Hm, dHm);
    LB.m += (b.xe < T.vx0 || b.xe > T.vxlast) ? 0.0 : Hb * Hm;
  }
  const double xeb = xeb_in + Hb * b.dH;
  const double vph = b.wd * b.ik, k = b.k2 * b.ik;
  const double vphb = xeb * L.ivTe;
  LB.Ud -= vphb;
  LB.ivTe += xeb * (vph - L.Ud);
  const double wdb = vphb * b.ik;
  const double ikb = vphb * b.wd;
  LB.wL -= wdb;
  LB.Vd -= wdb * k;
  const double kb = wdb * L.Vd + ikb * (b.ik * b.ik);
  return -kb * b.ik;
}

constexpr int kPair = 2;   // consecutive samples a thread sweeps with one chain of base points

// Two selects that the inputs of a pair sweep already decide (DESIGN.md section 4.1b, profiles/r10_selects_isa.txt):
// * has_next, the test for a right neighbour in point_core: a round of the sweep covers 1024 samples and npts is a multiple of 1024,
//   so only the second sample of the LAST pair of a thread can be sample npts - 1.  Everywhere else the test is the constant true and
//   the four selects per point that it feeds fold away (pair_has_next).
// * the out-of-grid selects of the Hermite lookup: hermite_lookup_c<true> reads the out-of-grid cell instead (k_spectrum_fused and
//   k_forward_pairs, whose tables stage_commit fills with that cell).
// Both are taken by the single-species instantiations only -- the ones every bench.py line and the reference's decks run.  The
// two-species instantiations sit at 256 VGPRs with 57 - 122 registers spilled, and either form moved the spill count of several of
// them up (by up to 19 registers; tests/test_isa_lane_exchange.py pins two of them): they keep the parent's code, text for text.
template <int NI>
constexpr bool kSelectFree = NI == 1;
// has a right neighbour: sample i of pair P (of NPAIR pairs per thread) at index j of npts samples
template <int NI, int P, int NPAIR>
__device__ __forceinline__ bool pair_has_next(int i, int j, int npts) {
  return (kSelectFree<NI> && (P < NPAIR - 1 || i < kPair - 1)) || (j + 1) < npts;
}

// v of lane l (wavefront-uniform l): two scalar reads of another lane's registers, no LDS
__device__ __forceinline__ double lane_f64(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// the halos of the four phase arrays of a spectrum buffer (the samples themselves are all written at the end of the sweep); nt threads
__device__ __forceinline__ void zero_phase_halos(double* xs, int Ls, int hs, int t, int nt) {
  for (int i = t; i < 8 * hs; i += nt) { const int ph_ = i / (2 * hs), o = i - ph_ * 2 * hs; xs[ph_ * Ls + (o < hs ? o : Ls - 2 * hs + o)] = 0.0; }
  if (t < 2) xs[4 * Ls + t] = 0.0;
}

// k_s(lambda) of this lineout (angle independent, form_factor.py:218), by every wavefront for the samples its own lanes read: the
// 128-sample unit(s) of its pairs and the sample right of each (which the next wavefront writes too -- the same value)
template <int NPAIR>
__device__ __forceinline__ void ks_cache_fill(double* __restrict__ ksc, const int (&jp)[NPAIR], const double (&ws)[NPAIR][kPair + 1],
                                              double wpe2, int npts) {
#pragma unroll
  for (int p = 0; p < NPAIR; ++p)
#pragma unroll
    for (int q = 0; q <= kPair; ++q) ksc[min(jp[p] + q, npts - 1)] = ks_eval(ws[p][q], wpe2);
}

// The base point right of a 128-sample unit at one angle, which the unit's last lane takes for its missing neighbour lane: evaluated
// at the frequency wse of that sample (k_s directly: a cache entry may belong to another wavefront), component c at o[c kExBound].
template <int NI, bool PAD = false>
__device__ __forceinline__ void unit_boundary_fill(double wse, double ct, const LineS<NI>& L, const Tables& T, double* o) {
  Base be;
  base_eval<NI, PAD>(wse, ks_eval(wse, L.wpe2), ct, L, T, be);
  o[0] = be.wd; o[kExBound] = be.ik; o[2 * kExBound] = be.xe; o[3 * kExBound] = be.F; o[4 * kExBound] = be.dH;
}

// The second base point of a pair from the neighbour lane's FIRST one of this angle (bf), register to register (next_lane_f64; all 64
// lanes are here: the branches and loops around it are wavefront-uniform); the last lane takes the unit's boundary point at src
// (unit_boundary_fill).  ks2: k_s of that sample.
// (pair_step_sched asks for the boundary point ahead of the exchange: boundary_request, then neighbour_take with the values)
struct Boundary { double wd, ik, xe, F, dH; };
__device__ __forceinline__ void boundary_request(const double* src, Boundary& u) {
  u.wd = src[0]; u.ik = src[kExBound]; u.xe = src[2 * kExBound]; u.F = src[3 * kExBound]; u.dH = src[4 * kExBound];
}
template <int NI>
__device__ __forceinline__ void neighbour_take(const Base& bf, const Boundary& u, double ks2, double ct, const LineS<NI>& L, Base& b1) {
  b1.wd = next_lane_f64(bf.wd, u.wd); b1.ik = next_lane_f64(bf.ik, u.ik); b1.xe = next_lane_f64(bf.xe, u.xe);
  b1.F = next_lane_f64(bf.F, u.F); b1.dH = next_lane_f64(bf.dH, u.dH);
  b1.ks = ks2;
  b1.k2 = base_k2<NI>(ks2, ct, L);   // (base_eval's own expression: the same bits; k itself -- a separately rounded
                                     //  square root there, not k2 * ik -- only enters through wd, which is exchanged)
}
template <int NI>
__device__ __forceinline__ void neighbour_take(const Base& bf, const double* src, double ks2, double ct, const LineS<NI>& L, Base& b1) {
  b1.wd = next_lane_f64(bf.wd, src[0]); b1.ik = next_lane_f64(bf.ik, src[kExBound]); b1.xe = next_lane_f64(bf.xe, src[2 * kExBound]);
  b1.F = next_lane_f64(bf.F, src[3 * kExBound]); b1.dH = next_lane_f64(bf.dH, src[4 * kExBound]);
  b1.ks = ks2;
  b1.k2 = base_k2<NI>(ks2, ct, L);   // (base_eval's own expression: the same bits; k itself -- a separately rounded
                                     //  square root there, not k2 * ik -- only enters through wd, which is exchanged)
}

// The reverse of one point of a Jacobian row behind a forward the caller has made (pf: point_core of b0 with its right neighbour b1,
// or its three steps): the forward value into xa, the reverse with the seed wa into the row J, the k^2 adjoints of the point's own
// base b0 and of its right neighbour b1 into the row's angle sums KA.
template <int NI, int GM, bool FAR, bool PAD = false>
__device__ __forceinline__ void row_reverse(const PointF<NI>& pf, const Base& b0, const Base& b1, const LineS<NI>& L, const Tables& T,
                                            double ct, double wa, double cw, double& xa, LineS<NI>& J, KsAcc& KA) {
  BaseAdj ba;
  double xen, Fn;
  xa = __builtin_fma(wa, point_fused_reverse<NI, GM, FAR>(pf, b0, L, T, wa, cw, ba, xen, Fn, J), xa);
  const double k22a = base_reverse_fused<NI, GM, PAD>(b0, L, T, ba, J);
  const double k22b = base_reverse_xf<NI, GM, PAD>(b1, L, T, xen, Fn, J);   // (xen = Fn = 0 at the last sample)
  KA.p1a += k22a; KA.p2a = __builtin_fma(k22a, ct, KA.p2a);
  KA.p1b += k22b; KA.p2b = __builtin_fma(k22b, ct, KA.p2b);
}
// One point of a Jacobian row: forward and reverse
template <int NI, int GM, bool ZH, bool FAR, bool PAD = false>
__device__ __forceinline__ void row_step(const Base& b0, const Base& b1, bool has_next, const LineS<NI>& L, const Tables& T, double ct,
                                         double wa, double cw, double& xa, LineS<NI>& J, KsAcc& KA) {
  PointF<NI> pf;
  point_core<NI, ZH, FAR>(b0, b1, has_next, L, T, pf);
  row_reverse<NI, GM, FAR, PAD>(pf, b0, b1, L, T, ct, wa, cw, xa, J, KA);
}

// The scheduled order of one angle iteration of a pair (r13_sweep_sched, DESIGN.md section 4.1b; profiles/r13_sweep_sched_model.txt):
// the instructions and the bits of base_eval / row_step twice, in an order that puts arithmetic which needs no table between every
// table read's request and its first use.  The steps are separated by scheduling barriers: inside a step the compiler orders as it
// likes, across them it moves nothing -- left alone it sinks every read back to its use (one to five instructions ahead of it: a wait
// of an LDS round trip per lookup).
//   1  geometry of both base points, the two square roots in lock step; both Hermite cells requested;
//   2  under that wait: the first point's W pair requested (the second's too in the asymptotic form), and what needs only 1/k and
//      w - k V of the first point (point_open: the k factors, xi_i, the asymptote or the ion requests);
//   3  both Hermite finishes and exp reductions, the two 2^(j/64) entries requested (asymptotic form: the unit's boundary point too);
//   4  under that wait: the first point's ion and W finishes (point_lookups) and, in the asymptotic form, the second point's open and finishes;
//   5  both F, their polynomials in lock step; close and reverse of the first point;
//   6  general form: the boundary point and the second point's W pair requested, under that wait its open with the ion requests, under
//      theirs the lane exchange, then its finishes; both forms: close and reverse of the second point.
// The reverse is where the kernel's register demand peaks.  The two reverses in one step (which the compiler then alternates) cost 16
// spilled registers; in the general form a second point's ion cells or its W pair and the boundary point in flight across the first
// point's reverse cost 46, 27 and 2: there the second point is opened behind that reverse.
// Given to the instantiations kSweepSched names -- the single-species kernel with the lane exchange and the full Z' table, which every
// bench.py line but --dlm runs; the half-table form spilled two registers with it, the DLM and two-species forms were not tried and
// keep base_eval / row_step.
template <int NI, int GM, bool ZH, bool EX>
constexpr bool kSweepSched = NI == 1 && GM == 0 && !ZH && EX;
__device__ __forceinline__ void sched_fence() { __builtin_amdgcn_sched_barrier(0); }
template <int NI, int GM, bool ZH, bool FAR, bool PAD>
__device__ __forceinline__ void pair_step_sched(const double (&w)[kPair + 1], double ksa, double ksb, double ks2, const double* exsrc,
                                                bool has_next1, const LineS<NI>& L, const Tables& T, double ct, double wa, double cw,
                                                double& xa0, LineS<NI>& J0, KsAcc& KA0, double& xa1, LineS<NI>& J1, KsAcc& KA1) {
  Base b0, b1, b2;
  HCell h0, h1;
  base_request_pair<NI, PAD>(w[0], w[1], ksa, ksb, ct, L, T, b0, b1, h0, h1);
  sched_fence();
  WCell w0, w1;
  PointF<NI> p0, p1;
  IonCell i0[NI], i1[NI];
  w_request(T.W, b0.xe, w0);
  if (FAR) w_request(T.W, b1.xe, w1);
  point_open<NI, ZH, FAR>(b0, L, T, p0, i0);
  sched_fence();
  ExpCell e0, e1;
  Boundary ub;
  base_finish_request(T, h0, b0, e0);
  base_finish_request(T, h1, b1, e1);
  if (FAR) boundary_request(exsrc, ub);
  sched_fence();
  point_lookups<NI, ZH, FAR>(L, T, i0, w0, p0);
  if (FAR) {
    point_open<NI, ZH, FAR>(b1, L, T, p1, i1);
    point_lookups<NI, ZH, FAR>(L, T, i1, w1, p1);
  }
  sched_fence();
  fexp_finish_pair(e0, e1, b0.F, b1.F);
  point_close<NI, FAR>(b0, b1, true, L, p0);
  row_reverse<NI, GM, FAR, PAD>(p0, b0, b1, L, T, ct, wa, cw, xa0, J0, KA0);
  sched_fence();
  // the lane's FIRST base point of this angle is what its left neighbour asks for
  if (!FAR) {   // (the boundary point's wait under the ion requests, theirs under the lane exchange)
    boundary_request(exsrc, ub);
    w_request(T.W, b1.xe, w1);
    sched_fence();
    point_open<NI, ZH, FAR>(b1, L, T, p1, i1);
    sched_fence();
  }
  neighbour_take<NI>(b0, ub, ks2, ct, L, b2);
  if (!FAR) {
    sched_fence();
    point_lookups<NI, ZH, FAR>(L, T, i1, w1, p1);
  }
  point_close<NI, FAR>(b1, b2, has_next1, L, p1);
  row_reverse<NI, GM, FAR, PAD>(p1, b1, b2, L, T, ct, wa, cw, xa1, J1, KA1);
}

// the k_L and omega_pe^2 columns of a row from its angle sums (see KsAcc); ksa, ksb: k_s of the row's sample and of its right neighbour
template <int NI>
__device__ __forceinline__ void ks_columns(const KsAcc& KA, double ksa, double ksb, const LineS<NI>& L, LineS<NI>& J) {
  const double p1 = KA.p1a + KA.p1b;
  J.kL = L.kL * p1 - (ksa * KA.p2a + ksb * KA.p2b);
  J.wpe2 = -(0.5 / (kC * kC)) * (p1 - L.kL * (KA.p2a / ksa + KA.p2b / ksb));
}

// sample j of the sweep into its slot of the spectrum buffer, with the factor ws^2 (left out of the sweep) and, if filt, the notch
// filter fl of the electron feature: x_j and xbar_j carry both
__device__ __forceinline__ void store_scaled(double* slot, double x, double w, bool filt, const double* __restrict__ fl, int j) {
  *slot = x * (filt ? w * w * fl[j] : w * w);
}
