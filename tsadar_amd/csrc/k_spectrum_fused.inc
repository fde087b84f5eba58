// k_spectrum_fused.inc -- k_spectrum_fused: loss + gradient of one (lineout, feature) per workgroup in ONE sweep over the
// (wavelength, angle) points.  Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).
//
// k_spectrum (MODE 1) walks the points twice: a forward sweep for the spectrum x_j, then -- once the adjoint xbar_j of the
// spectrum is known (normalisation, binning and convolution have to be reversed first) -- a reverse sweep that RECOMPUTES
// every point to propagate xbar_j w_a into the lineout-scalar adjoints.  The reverse of a point is linear in its seed,
// so the single sweep here reverses every point with the seed w_a alone and keeps, per wavelength sample j, the row
//     J[j][k] = sum_a  d(w_a P(j, a)) / d(lineout scalar k)          (k: wpe2, wL, kL, 1/vTe, a_e, Ud, Vd | 1/xi_i, a_i, c_s | m)
// next to the forward value x_j = sum_a w_a P(j, a).  A thread keeps the four rows of its samples in registers through the
// instrument chain (which it shares with k_spectrum: phase-layout convolutions, arg-max normalisation, loss) and contracts
// them with the spectrum adjoint afterwards: grad_k = sum_j xbar_j J[j][k].  The second pass over the points, with its
// table lookups, exp() and 1/x evaluations -- 35 % of a k_spectrum step -- is gone; the price is 4 x (7 + 3 n_ion)
// accumulators per thread instead of 9 + 3 n_ion, and one more application of the (cheap, linear) base reverse per point:
// the finite difference along lambda (form_factor.py:258-259) couples x_j to the base quantities of sample j + 1, whose
// contribution must land in row j, not in row j + 1.
// Structure of the sweep (each measured, DESIGN.md section 4.1b): two PAIRS of consecutive samples per thread, each pair with
// its own loop over the angles (rows not in flight are parked outside the loop: no spills in it); the k_L / omega_pe^2
// columns from per-row angle sums (KsAcc); the asymptotic form of the ion terms for every (wavefront, pair) whose 128
// samples all lie away from the laser line (point_core<FAR>).
//
// Restrictions (launch_spectrum falls back to k_spectrum otherwise): one gradient point (the rows would need a g axis),
// points_per_pixel = 1 (phase layout), 256 threads per feature, no table adjoints (GM <= 1: the scatter into the
// distribution-function tables is not linear-separable per sample).
//
// Reference rows: a4-a15 of SURVEY.md section 8 exactly as k_spectrum (form_factor.py:182-298, generate_spectra.py:139-220,
// irf.py:50-132, loss_function.py:190-418, and reverse-mode differentiation of those, loss_function.py:108).

// point_reverse with the seed PQ = w_a pref (no spectrum adjoint yet): returns S (1 + 2w/wL), whose PQ-fold is the contribution
// to x_j (before the factor ws^2), the adjoints of this point's base quantities (ba) and of the right neighbour's (xi_e, F),
// and accumulates the direct lineout-scalar adjoints into the row J.  cw = -i2wL^2 / 2 folds the adjoint of 2/wL into wL.
// The deferred factor of a_i (x -1/2) is applied after the contraction (see the kernel); pref's adjoint is x_j itself.
template <int NI, int GM, bool ZH, bool FAR = false>
__device__ __forceinline__ double point_fused(const Base& b, const Base& bn, bool has_next, const LineS<NI>& L, const Tables& T,
                                              double PQ, double cw, BaseAdj& ba, double& xen, double& Fn, LineS<NI>& J) {
  // ---- forward (form_factor.py:243-296) ----
  PointF<NI> pf;
  point_core<NI, ZH, FAR>(b, bn, has_next, L, T, pf);
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

// The adjoint of k^2 = k_s^2 + k_L^2 - 2 k_s k_L cos(theta) flows to k_L and, through k_s(lambda), to omega_pe^2:
//   kLbar += k22 (k_L - k_s ct),   wpe2bar -= k22 (k_s - k_L ct) / (2 c^2 k_s),      k22 = 2 x adjoint of k^2.
// k_s depends on the wavelength sample only and ct = cos(theta_a) on the angle only, so a row accumulates P1 = sum_a k22 and
// P2 = sum_a k22 ct per base point (its own sample and the right neighbour) -- two instructions per base where the direct form
// took ten, a reciprocal of k_s among them -- and the two columns are assembled once per sample after the angle loop:
//   kLbar = k_L (P1a + P1b) - (k_s,j P2a + k_s,j+1 P2b),   wpe2bar = -[P1a + P1b - k_L (P2a / k_s,j + P2b / k_s,j+1)] / (2 c^2).
struct KsAcc { double p1a, p2a, p1b, p2b; };

// base_reverse (tsff_device.h) without its k_L / omega_pe^2 tail: returns k22
template <int NI, int GM>
__device__ __forceinline__ double base_reverse_fused(const Base& b, const LineS<NI>& L, const Tables& T, const BaseAdj& ba,
                                                     LineS<NI>& LB) {
  const double Hb = ba.F * b.F;  // adjoint of H = ln f_e(xi_e)
  if (GM == 1) {  // d ln f_e(xi_e)/dm: Hermite interpolant of the tangent table (zero outside the vx grid)
    Tables Tm = T;
    Tm.hc = T.hcm;
    double Hm, dHm;
    hermite_lookup_c(Tm, b.xe, Hm, dHm);
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
template <int NI, int GM>
__device__ __forceinline__ double base_reverse_xf(const Base& b, const LineS<NI>& L, const Tables& T, double xeb_in, double Fb,
                                                  LineS<NI>& LB) {
  const double Hb = Fb * b.F;
  if (GM == 1) {
    Tables Tm = T;
    Tm.hc = T.hcm;
    double Hm, dHm;
    hermite_lookup_c(Tm, b.xe, Hm, dHm);
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

// TSFF_TRACE (measurement builds only, scripts/trace_fused.py): phase time stamps of every workgroup (s_memrealtime, 100 MHz)
#ifdef TSFF_TRACE
__device__ unsigned long long* g_trace_buf = nullptr;
#define TSFF_STAMP(k) do { if (tid == 0 && g_trace_buf) g_trace_buf[(size_t)item * 16 + (k)] = wall_clock64(); } while (0)
#define TSFF_STAMP_WAVE(k) do { if (lane == 0 && g_trace_buf) g_trace_buf[(size_t)item * 16 + (k) + hw] = wall_clock64(); } while (0)
#define TSFF_STAMP_HW() do { if (tid == 0 && g_trace_buf) g_trace_buf[(size_t)item * 16] = ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) | (unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)); } while (0)
#else
#define TSFF_STAMP(k) do {} while (0)
#define TSFF_STAMP_WAVE(k) do {} while (0)
#define TSFF_STAMP_HW() do {} while (0)
#endif
// The phase-layout convolution of k_spectrum (four adjacent outputs per thread, groups of four taps read by scalar loads from the
// zero-padded tap array in constant memory, the explicit FMA chains that pin the roundings), unrolled by two so that the sliding
// window of seven spectrum values is renamed instead of moved (three 64-bit moves per 16 FMAs in the rolled form).  DIR = +1: taps
// ascending (forward), -1: descending (adjoint).  Same sums, same order, same bits as k_spectrum's loop.
// (Tried and dropped, profiles/r03k: the same loop software-pipelined with the taps read from an LDS copy -- scalar and LDS loads
//  share one counter that can only be drained completely, and the kernel has no SGPRs left to carry a group of taps across the back
//  edge -- costs more VALU instructions for its addresses than the waits it removes: conv + arg-max 5.5 / 8.0 us against 4.8 / 6.7.)
//
// r08_conv (DESIGN.md section 4.1b): the loop is software-pipelined over SETS of two tap groups.  A set is what the 32 FMAs of two groups read:
// eleven window values (22 VGPRs) and eight taps (16 SGPRs).  The rolled form requested its set at the top of an
// iteration and waited for it in front of the first FMA -- an LDS plus scalar-cache round trip exposed before every 32 FMAs, with
// nothing in flight while they issue.  Now the set of groups a + 2, a + 3 is requested while the FMAs of groups a, a + 1 issue:
//   wait (everything outstanding: exactly the current set) | request the next set | 32 FMAs on the current set
// twice per loop body, the two register sets changing roles by renaming.  Scalar loads and LDS reads share one counter and scalar
// loads return out of order, so the only exact wait is "all of it": it is written out (conv_wait) where NOTHING but the current
// set is outstanding, and the request follows it at once; the scheduling barriers keep the machine scheduler from sinking the
// requests to their uses (as it did with the boundary point of the sweep, DESIGN.md section 4.1b).
// Same sums, same order, same bits: the four accumulators are the same explicit chains over the groups 0 .. na - 1.
//
// Reading ahead.  Every request is for two groups (a, a + 1) with a even and a <= na (the first one, a = 0; in the loop body a + 4
// <= na; in the tail a + 2 <= na), so the highest group ever read is na + 1 -- two beyond the last one used.
//   taps, forward (pt = ptaps + cf_i0, ascending): highest entry cf_i0 + 4 (na + 1) + 3 = cf_i0 + 4 na + 7 < padded_taps() =
//     cf_i0 + 4 na + 8; the host array has kTapLead + n + 16 entries and cf_i0 + 4 na + 7 <= (3 - pre) + (pre + n + 3) + 7 = n + 13.
//   taps, adjoint (pt = ptaps + ca_i0, descending): lowest entry ca_i0 - 4 (na + 1) - 3 >= (n + 2 + prea) - (prea + n + 3) - 7
//     = -8 = -kTapLead: S.ptaps points kTapLead zeros INTO its allocation (tsff_api.inc), the highest entry is ca_i0 <= n + 5.
//   window: sl = ht + a0 + hs with 0 <= ht < 256 and, by the definition of S.hs, -a0 <= hs - 1 and a0 + na <= hs - 1, so
//     sl >= 1; the highest index is X2[(na + 1) + 1] = 2 Ls + sl + na + 2 <= 2 Ls + 255 + 2 hs + 1 = 3 Ls (Ls = 256 + 2 hs), and
//     X3[na + 1] <= 3 Ls + Ls - 1: inside the four phase arrays (4 Ls + 2 doubles) for every na >= 1.
// What is read beyond group na - 1 is never used.
// PIPE = false: the rolled loop (k_forward_pairs: see there).
typedef const double __attribute__((address_space(4))) cdouble_t;
struct ConvSet { double w[11], g[8]; };
// groups a, a + 1: the window values V0 .. V6 of the first, V3 .. V6 of the second and their taps.  (V0 .. V2 are the V4 .. V6 of
// the group before and could be inherited from the previous set -- but then three registers of a set are still read when the set
// is requested again, the allocator loads into temporaries and copies them behind a wait of its own in the middle of the FMAs.)
template <int DIR>
__device__ __forceinline__ void conv_request(const double* __restrict__ X0, const double* __restrict__ X1, const double* __restrict__ X2,
                                             const double* __restrict__ X3, cdouble_t* pt, int a, int at, ConvSet& s) {
  s.w[0] = X0[a]; s.w[1] = X1[a]; s.w[2] = X2[a];
  s.w[3] = X3[a]; s.w[4] = X0[a + 1]; s.w[5] = X1[a + 1]; s.w[6] = X2[a + 1];
  s.w[7] = X3[a + 1]; s.w[8] = X0[a + 2]; s.w[9] = X1[a + 2]; s.w[10] = X2[a + 2];
#pragma unroll
  for (int k = 0; k < 8; ++k) s.g[k] = pt[DIR * (4 * at + k)];
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void conv_wait() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0), vmcnt and expcnt left alone
  __builtin_amdgcn_sched_barrier(0);
}
// one tap group (H = 0, 1: which half of the set); the window slides by renaming
template <int H>
__device__ __forceinline__ void conv_group(const ConvSet& s, double (&acc)[4]) {
  const double V0 = s.w[4 * H], V1 = s.w[4 * H + 1], V2 = s.w[4 * H + 2];
  const double V3 = s.w[4 * H + 3], V4 = s.w[4 * H + 4], V5 = s.w[4 * H + 5], V6 = s.w[4 * H + 6];
  const double g0 = s.g[4 * H], g1 = s.g[4 * H + 1], g2 = s.g[4 * H + 2], g3 = s.g[4 * H + 3];
  acc[0] = __builtin_fma(g3, V3, __builtin_fma(g2, V2, __builtin_fma(g1, V1, __builtin_fma(g0, V0, acc[0]))));
  acc[1] = __builtin_fma(g3, V4, __builtin_fma(g2, V3, __builtin_fma(g1, V2, __builtin_fma(g0, V1, acc[1]))));
  acc[2] = __builtin_fma(g3, V5, __builtin_fma(g2, V4, __builtin_fma(g1, V3, __builtin_fma(g0, V2, acc[2]))));
  acc[3] = __builtin_fma(g3, V6, __builtin_fma(g2, V5, __builtin_fma(g1, V4, __builtin_fma(g0, V3, acc[3]))));
}
template <int DIR, bool PIPE = true>
__device__ __forceinline__ void conv4_phase(const double* __restrict__ xs, int Ls, int sl, cdouble_t* pt, int na, double (&acc)[4]) {
  const double* __restrict__ X0 = xs + sl, * __restrict__ X1 = X0 + Ls, * __restrict__ X2 = X1 + Ls, * __restrict__ X3 = X2 + Ls;
  if (!PIPE) {
    double V0 = X0[0], V1 = X1[0], V2 = X2[0];
#pragma unroll 2
    for (int a = 0; a < na; ++a) {
      const double V3 = X3[a], V4 = X0[a + 1], V5 = X1[a + 1], V6 = X2[a + 1];
      const double g0 = pt[4 * DIR * a], g1 = pt[4 * DIR * a + DIR], g2 = pt[4 * DIR * a + 2 * DIR], g3 = pt[4 * DIR * a + 3 * DIR];
      acc[0] = __builtin_fma(g3, V3, __builtin_fma(g2, V2, __builtin_fma(g1, V1, __builtin_fma(g0, V0, acc[0]))));
      acc[1] = __builtin_fma(g3, V4, __builtin_fma(g2, V3, __builtin_fma(g1, V2, __builtin_fma(g0, V1, acc[1]))));
      acc[2] = __builtin_fma(g3, V5, __builtin_fma(g2, V4, __builtin_fma(g1, V3, __builtin_fma(g0, V2, acc[2]))));
      acc[3] = __builtin_fma(g3, V6, __builtin_fma(g2, V5, __builtin_fma(g1, V4, __builtin_fma(g0, V3, acc[3]))));
      V0 = V4; V1 = V5; V2 = V6;
    }
    return;
  }
  ConvSet A, B;
  conv_request<DIR>(X0, X1, X2, X3, pt, 0, 0, A);
  int a = 0;
  for (; a + 4 <= na; a += 4) {   // two sets per body: A holds groups a, a + 1 on entry
    conv_wait();
    conv_request<DIR>(X0, X1, X2, X3, pt, a + 2, 2, B);
    conv_group<0>(A, acc); conv_group<1>(A, acc);
    conv_wait();
    conv_request<DIR>(X0, X1, X2, X3, pt, a + 4, 4, A);
    conv_group<0>(B, acc); conv_group<1>(B, acc);
    pt += 16 * DIR;   // (the taps through a running scalar pointer, the window through the index: the fewest address instructions)
  }
  // the last na - a = 0 .. 3 groups: A holds the first two of them (requested, not yet waited for)
  conv_wait();
  if (na - a >= 2) {
    conv_request<DIR>(X0, X1, X2, X3, pt, a + 2, 2, B);
    conv_group<0>(A, acc); conv_group<1>(A, acc);
    conv_wait();
    if (na - a == 3) conv_group<0>(B, acc);
  } else if (na - a == 1) {
    conv_group<0>(A, acc);
  }
}

constexpr int kRedSums = 32;   // offset (doubles) of the five partial block sums in the reduction scratch
// EX: the third base point of a pair -- the right neighbour of its second sample, which is the FIRST sample of the next
// thread's pair -- is not evaluated again but taken from that thread: every lane receives (w - k V, 1/k, xi_e, F, dH/dxi) of its
// neighbour lane's first base point register to register (next_lane_f64: ten DPP moves, no LDS, no wait, no barrier; k_s comes from
// the cache, k^2 is two instructions).  The last lane of a wavefront has no neighbour lane: the base points right of each
// 128-sample unit are evaluated once per (unit, angle) before the sweep and kept in LDS.  2 instead of 3 base evaluations (k, xi_e,
// Hermite lookup, exp: ~52 instructions each) per pair and angle.  Needs kExDoubles of LDS and n_angles <= 16 (launch_fused decides).
// The prologue (round 3).  The workgroup timeline (scripts/trace_fused.py, profiles/r03a_trace_fused.txt) showed what bounds the
// launch: a wavefront issues at most every second slot of its SIMD (scripts/ubench_dep.hip), two resident wavefronts per SIMD do
// not slow each other down, so a CU finishes a pair of workgroups every (sweep + everything else) -- and everything else was
// 24-30 us of pure latency (7-9 us of it the prologue: eight copy loops, each a global-load round trip, and three barriers)
// against a 34-40 us sweep.  Now: every table byte and the lineout's parameters are REQUESTED in one batch (stage_segments),
// written to LDS behind one wait, the Hermite coefficients come from the LDS copy of ln f_e, the k_s cache and the unit-boundary
// base points are filled by every wavefront for its own lanes (no workgroup barrier), and only the halos of the spectrum buffer
// are zeroed.  (Persistent workgroups looping over the items were built first: the nested loops cost the register allocator
// its balance -- 125 VGPRs spilled, scratch reloads inside the angle loops -- for 1 us more than this form saves.)
template <int NI, int GM, bool ZH, bool EX = false>
__global__ __launch_bounds__(kHalf, 2) void k_spectrum_fused(KStatic S, KCall K, int f0, int flags,
                                                             const double* __restrict__ lrec) {
  // lrec: [items][kLineRec] the lineout scalars of every (lineout, feature) item, written by k_fused_prep just before this launch
  // flags as in k_spectrum: bit 1 k_s cache in LDS, bit 2 interleaved plan (grid 2B: workgroup f B + b evaluates feature f
  // of lineout b and leaves its part of the gradient in K.gpart[f][b][:]); otherwise grid B, feature f0, grad written
  const bool use_ks = flags & 2, interleaved = flags & 4;
  const int item = blockIdx.x;
  const int f_il = interleaved ? (int)(item >= K.B) : 0;
  const int b = K.b0 + item - f_il * K.B, tid = threadIdx.x;
  // (item of the whole batch: the records of k_fused_prep / for k_fused_finish are laid out over all Btot lineouts, whatever
  //  column block this launch covers)
  const size_t gitem = (size_t)f_il * K.Btot + b;
  constexpr int TPF = kHalf, NW = TPF / 64;
  const int ht = tid, lane = tid & 63, hw = tid >> 6;
  const int f = __builtin_amdgcn_readfirstlane(interleaved ? f_il : f0);
  extern __shared__ __align__(16) unsigned char smem[];
  TSFF_STAMP_HW();
  TSFF_STAMP(1);
  const Smem m = carve(smem, S, 1, GM, use_ks, true, ZH, EX);
  constexpr int NPk = TSFF_NP(NI);
  const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
  const int npts = S.npts, NA = S.n_angles;   // npts == 1024 == 4 TPF: exactly one strip per thread
  const int hs = S.hs, Ls = npts / 4 + 2 * hs;
  double* xs = m.x;
  auto XA = [&](int j) { return (j & 3) * Ls + (j >> 2) + hs; };   // phase layout (see k_spectrum)
  Tables T;
  const double lam_shift = S.lam_shift[f];
  const double* __restrict__ omgs = S.omgs[f];
  constexpr int kPair = 2;
  const int jp[2] = {kPair * ht, npts / 2 + kPair * ht};
  double ws[2][kPair + 1];
  LineS<NI> L;
  double* __restrict__ ksc = use_ks ? m.ksc : nullptr;
  {
    // requested in this order: the lineout's parameters, every table byte, the frequency axis of the thread's samples
    TSFF_STAGE_LOCALS;
    stage_issue(TSFF_STAGE_ARGS, m, S, K, S.shared_fe ? 0 : b, ZH, f);
    // (written to LDS right away: holding the sixty staged registers across the scalar chain below makes the allocator spill
    //  them, and the DLM instantiation without the lane exchange then produced wrong spectra -- variant A of the bisection)
    stage_commit(TSFF_STAGE_ARGS, m, S, K, S.shared_fe ? 0 : b, T, ZH, f);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q <= kPair; ++q) ws[p][q] = omgs[min(jp[p] + q, npts - 1)];
    // The lineout scalars come ready-made from k_fused_prep (one thread per item, run just before this launch): activation,
    // fraction renormalisation, three square roots and eight divisions were 3 us of ONE wavefront-uniform dependency chain at the
    // head of every workgroup, repeated by all its 256 threads.  Wavefront-uniform address: scalar loads, straight into SGPRs.
    {
      lines_load<NI>(lrec + gitem * kLineRec, 1, [](double v) { return uni(v); }, L);
    }
    if (use_ks) {
      // k_s(lambda) of this lineout (angle independent, form_factor.py:218), by every wavefront for the samples its own lanes read:
      // its two 128-sample units and the sample right of each (which the next wavefront writes too -- the same value)
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q <= kPair; ++q) ksc[min(jp[p] + q, npts - 1)] = ks_eval(ws[p][q], L.wpe2);
    }
    // the halos of the four phase arrays (the samples themselves are all written at the end of the sweep)
    for (int i = ht; i < 8 * hs; i += TPF) { const int ph_ = i / (2 * hs), o = i - ph_ * 2 * hs; xs[ph_ * Ls + (o < hs ? o : Ls - 2 * hs + o)] = 0.0; }
    if (ht < 2) xs[4 * Ls + ht] = 0.0;
  }
  // Away from the laser line every point of a wavefront's pair sees |xi_i| >> 1: the ion terms are the asymptote and
  // exp(-xi_i^2) = 0 exactly (point_core<FAR>).  Decided once per (wavefront, pair) from a bound that holds for all its 128
  // samples (and the right neighbour of the last one), all angles and all species (far_range, tsff_device.h).
  // The two ends of a unit -- sample 128 hw (+ 512) and the sample right of its last one -- are the first frequency of lane 0 and
  // the third of lane 63: read from those lanes' registers, not from memory again.
  double w_lo[2], w_hi[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    w_lo[p] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(ws[p][0]), 0), __builtin_amdgcn_readlane(__double2loint(ws[p][0]), 0));
    w_hi[p] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(ws[p][kPair]), 63), __builtin_amdgcn_readlane(__double2loint(ws[p][kPair]), 63));
  }
  const bool far0 = far_range_w<NI>(w_lo[0], w_hi[0], L), far1 = far_range_w<NI>(w_lo[1], w_hi[1], L);
  // (EX) frequency of the unit-boundary base point this lane evaluates behind the barrier (lane = 16 P + a)
  const double ex_wse = ((lane >> 4) & 1) ? w_hi[1] : w_hi[0];
  __syncthreads();
  TSFF_STAMP(2);
  // Sample ownership in the sweep: thread ht owns the two PAIRS of consecutive samples {2 ht, 2 ht + 1} and
  // {npts/2 + 2 ht, npts/2 + 2 ht + 1} (rows q = 0, 1 and q = 2, 3).  Each pair has its own loop over the angles -- only its two
  // rows are touched inside the loop, so the register allocator can park the other two outside of it (all four rows in one
  // loop spilled ~34 doubles INSIDE the loop: 1.54 ms against 1.14) -- and a wavefront's pair covers 128 CONSECUTIVE samples,
  // the unit for which the asymptotic form of the ion terms is decided (below): one unit of eight contains the laser line.
  // (The convolutions own samples differently -- 4 ht .. 4 ht + 3, the phase layout; the spectrum and its adjoint change hands
  //  through LDS, where they live anyway.)
  auto JQ = [&](int q) { return jp[q >> 1] + (q & 1); };   // sample of row q
  LineS<NI> J[kStrip];
  KsAcc KA[kStrip];
  double xa[kStrip];
#pragma unroll
  for (int q = 0; q < kStrip; ++q) { zero_lines<NI>(J[q]); xa[q] = 0.0; KA[q].p1a = KA[q].p2a = KA[q].p1b = KA[q].p2b = 0.0; }
  const double cw = -0.5 * L.i2wL * L.i2wL;
  // EX: the base point right of unit u (u = 2 hw + P) at angle a: component c at exb[c kExBound + 16 u + a]
  double* exb = m.ex;
  if (EX) {   // the unit-boundary base points of this wavefront's two units, all angles at once (lane = 16 P + a)
    const int Pb = (lane >> 4) & 1, ab = lane & 15;
    if (lane < 32 && ab < NA) {
      const double wse = ex_wse;
      Base be;
      base_eval<NI>(wse, ks_eval(wse, L.wpe2), m.cosa[ab], L, T, be);   // (k_s directly: the cache entry may belong to another wavefront)
      double* o = exb + 16 * (2 * hw + Pb) + ab;
      o[0] = be.wd; o[kExBound] = be.ik; o[2 * kExBound] = be.xe; o[3 * kExBound] = be.F; o[4 * kExBound] = be.dH;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (the sweep reads other lanes' boundary points)
  }
  auto sweep = [&](auto pair_tag, auto far_tag) {
    constexpr int P = decltype(pair_tag)::value;
    constexpr bool FAR = decltype(far_tag)::value;
    const int jb = jp[P];
    const int j2 = min(jb + kPair, npts - 1);
    const double ks2 = EX ? (use_ks ? ksc[j2] : ks_eval(ws[P][kPair], L.wpe2)) : 0.0;
    double ct_n = m.cosa[0], wa_n = m.wsa[0];   // (the angle's constants are read from LDS one iteration ahead of their use)
    // (EX) the unit's boundary point, which lane 63 takes for its missing neighbour
    const double* exu = EX ? exb + 16 * (2 * hw + P) : nullptr;
    for (int a = 0; a < NA; ++a) {
      const double ct = uni(ct_n), wa = uni(wa_n * L.pref);
      { const int an = min(a + 1, NA - 1); ct_n = m.cosa[an]; wa_n = m.wsa[an]; }
      Base b0;
      base_eval<NI>(ws[P][0], use_ks ? ksc[jb] : ks_eval(ws[P][0], L.wpe2), ct, L, T, b0);
      // (EX) the lane's FIRST base point of this angle is what its left neighbour asks for: b0 itself is the second one by then
      const double f_wd = b0.wd, f_ik = b0.ik, f_xe = b0.xe, f_F = b0.F, f_dH = b0.dH;
#pragma unroll
      for (int i = 0; i < kPair; ++i) {
        constexpr int q0 = kPair * P;
        const int q = q0 + i, j = jb + i;
        const bool has_next = (j + 1) < npts;
        Base b1;
        if (EX && i == kPair - 1) {   // the neighbour lane's first base point (the unit's boundary point for the last lane), register
          // to register (next_lane_f64; all 64 lanes are here: the branches and loops around it are wavefront-uniform)
          // (The boundary point is read HERE.  Read an iteration ahead, as ct_n / wa_n are, or at the top of the iteration, its five
          //  doubles live across the pair's first point and the allocator spills 26 / 10 registers outside the loops where this form
          //  spills none; measured, DESIGN.md section 4.1b.)
          const double* src = exu + a;
          b1.wd = next_lane_f64(f_wd, src[0]); b1.ik = next_lane_f64(f_ik, src[kExBound]); b1.xe = next_lane_f64(f_xe, src[2 * kExBound]);
          b1.F = next_lane_f64(f_F, src[3 * kExBound]); b1.dH = next_lane_f64(f_dH, src[4 * kExBound]);
          b1.ks = ks2;
          b1.k2 = base_k2<NI>(ks2, ct, L);   // (base_eval's own expression: the same bits; k itself -- a separately rounded
                                             //  square root there, not k2 * ik -- only enters through wd, which is exchanged)
        } else {
          base_eval<NI>(ws[P][i + 1], use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(ws[P][i + 1], L.wpe2), ct, L, T, b1);
        }
        BaseAdj ba;
        double xen, Fn;
        xa[q] = __builtin_fma(wa, point_fused<NI, GM, ZH, FAR>(b0, b1, has_next, L, T, wa, cw, ba, xen, Fn, J[q]), xa[q]);
        const double k22a = base_reverse_fused<NI, GM>(b0, L, T, ba, J[q]);
        const double k22b = base_reverse_xf<NI, GM>(b1, L, T, xen, Fn, J[q]);   // (xen = Fn = 0 at the last sample)
        KA[q].p1a += k22a; KA[q].p2a = __builtin_fma(k22a, ct, KA[q].p2a);
        KA[q].p1b += k22b; KA[q].p2b = __builtin_fma(k22b, ct, KA[q].p2b);
        b0 = b1;
      }
    }
  };
  if (far0) sweep(std::integral_constant<int, 0>{}, std::true_type{}); else sweep(std::integral_constant<int, 0>{}, std::false_type{});
  if (far1) sweep(std::integral_constant<int, 1>{}, std::true_type{}); else sweep(std::integral_constant<int, 1>{}, std::false_type{});
  TSFF_STAMP_WAVE(9);
#pragma unroll
  for (int q = 0; q < kStrip; ++q) {   // the k_L and omega_pe^2 columns of the rows from their angle sums (see KsAcc)
    const int j = JQ(q);
    const double ksa = use_ks ? ksc[j] : ks_eval(ws[q >> 1][q & 1], L.wpe2);
    const double ksb = use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(ws[q >> 1][(q & 1) + 1], L.wpe2);
    const double p1 = KA[q].p1a + KA[q].p1b;
    J[q].kL = L.kL * p1 - (ksa * KA[q].p2a + ksb * KA[q].p2b);
    J[q].wpe2 = -(0.5 / (kC * kC)) * (p1 - L.kL * (KA[q].p2a / ksa + KA[q].p2b / ksb));
  }
  {   // the factor ws^2 (left out of the sweep) and the notch filter of the electron feature: x_j and xbar_j carry it
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
#pragma unroll
    for (int q = 0; q < kStrip; ++q) {
      const double w = ws[q >> 1][q & 1];
      xs[XA(JQ(q))] = xa[q] * (filt ? w * w * S.filt[JQ(q)] : w * w);
    }
  }
  __syncthreads();
  TSFF_STAMP(3);

  // ================= IRF convolution ("same"), bin average, normalisation (phase layout, see k_spectrum) =================
  constexpr int BPT = 4;
  typedef const double __attribute__((address_space(4))) cdouble;
  // What the chain needs from global memory is requested HERE, ahead of the convolution -- the chain is a sequence of latencies and
  // every microsecond of it is a microsecond in which this wavefront's SIMD issues at half rate: the measured data of the
  // thread's four bins (first touch: HBM), masks, bin wavelengths and the last stage's parameter transform.
  const bool raw = S.raw[f];   // no instrument response for this feature (irf.py:82-86), see k_spectrum
  const size_t row4 = (size_t)b * TSFF_NBINS + 4 * ht;
  double dpre[BPT], npre[BPT], lpre[BPT];
  uint8_t mpre[BPT];
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    dpre[r] = K.data[f][row4 + r];
    npre[r] = K.noise[f] ? K.noise[f][row4 + r] : 0.0;
    lpre[r] = f == TSFF_FEATURE_ELE ? S.lam_bin[f][4 * ht + r] : 0.0;
    mpre[r] = S.mask[f][4 * ht + r];
  }
  const double amps = raw ? 1.0 : K.amps[f][b];
  const double* __restrict__ lrp = lrec + gitem * kLineRec + 9 + 4 * NI;   // (physical lam, amp1, amp2, amp3)
  const double p_lam_v = lrp[0], p_amp1_v = lrp[1], p_amp2_v = lrp[2], p_amp3_v = lrp[3];
  double wpre[BPT];   // omega_s^2 (and the notch filter of the electron feature) of the four samples whose adjoint this thread hands over
  {
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
#pragma unroll
    for (int r = 0; r < BPT; ++r) {
      const double w = omgs[4 * ht + r];
      wpre[r] = filt ? w * w * S.filt[4 * ht + r] : w * w;
    }
  }
  double ybin[BPT] = {0.0, 0.0, 0.0, 0.0};
  conv4_phase<1>(xs, Ls, ht + S.cf_a0[f] + hs, (cdouble_t*)(S.ptaps[f] + S.cf_i0[f]), S.cf_na[f], ybin);
  double M = ybin[0];
  int pstar = 4 * ht;
#pragma unroll
  for (int r = 1; r < BPT; ++r)
    if (ybin[r] > M) { M = ybin[r]; pstar = 4 * ht + r; }
  half_argmax<NW>(M, pstar, m.red, 0, hw, lane);
  TSFF_STAMP(4);
  const double invM = raw ? 1.0 : 1.0 / M;
  const double p_lam = uni(p_lam_v), p_amp1 = uni(p_amp1_v), p_amp2 = uni(p_amp2_v), p_amp3 = uni(p_amp3_v);
  double Tb[BPT], Ap[BPT];
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = 4 * ht + r;
    const double A = bin_amplitude(f, raw, amps, lpre[r], p_lam, p_amp1, p_amp2, p_amp3);
    Ap[r] = A;
    const double t = thry_value(A, ybin[r], invM, K.noise[f] != nullptr, npre[r]);   // thomson_diagnostic.py:139-140
    if (K.thry[f]) K.thry[f][(size_t)b * TSFF_NBINS + pb] = t;
    Tb[r] = bin_loss(S, K, f, dpre[r], t, mpre[r], s0, s1);
  }

  // ================= adjoint of normalisation + binning: T_p = A_p ybin_p / M (+ noise), M attained at pstar =================
  double sn = 0.0, a1b = 0.0, a2b = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) norm_adjoint_bin(f, Tb[r], ybin[r], invM, Ap[r], amps, lpre[r], p_lam, sn, a1b, a2b);
  // The five block sums (two loss sums, three sums of the normalisation's adjoint) are NOT waited for here: every wavefront leaves
  // its partial sums in LDS and goes on; they are read behind the barrier that follows the adjoint convolution anyway.  What needed
  // them at this point -- the correction -sn / M of ybar at the arg-max bin -- is linear in ybar and is applied to the convolved
  // adjoint instead: xbar_i -= (sn / M) h[i - p* - toff].  (Round 2 waited for half_sums here: two barriers and five butterflies
  // on the critical path of the chain, of which every microsecond is a microsecond of half-rate issue on this SIMD.)
  {
    double v5[5] = {s0, s1, sn, a1b, a2b};
#pragma unroll
    for (int k = 0; k < 5; ++k) v5[k] = wave_sum(v5[k]);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) m.red[kRedSums + k * NW + hw] = v5[k];   // (behind the slots of half_argmax, which a slower wavefront may still read)
    }
  }
  // (ybar lives in the memory of x: every thread has read its x window above -- half_argmax's barriers lie in between)
#pragma unroll
  for (int r = 0; r < BPT; ++r) xs[XA(4 * ht + r)] = Tb[r] * Ap[r] * invM;
  __syncthreads();
  TSFF_STAMP(5);
  // ================= adjoint of convolution + binning (same sliding window, taps read backwards) =================
  double sx[4] = {0.0, 0.0, 0.0, 0.0};
  conv4_phase<-1>(xs, Ls, ht + S.ca_a0[f] + hs, (cdouble_t*)(S.ptaps[f] + S.ca_i0[f]), S.ca_na[f], sx);

  // ================= contraction of the rows with the spectrum adjoint: LB_k = sum_j xbar_j J[j][k] =================
  // (the adjoint of the un-scaled sample j -- it carries ws^2 and the filter -- goes from the thread that owns j in the
  //  convolutions to the thread that owns it in the sweep through the LDS buffer ybar has just been read out of)
  __syncthreads();
  TSFF_STAMP(6);
  {   // the block sums, with the association of half_sums
    const double* r = m.red + kRedSums;
    s0 = (r[0] + r[1]) + (r[2] + r[3]);
    s1 = (r[NW] + r[NW + 1]) + (r[NW + 2] + r[NW + 3]);
    sn = (r[2 * NW] + r[2 * NW + 1]) + (r[2 * NW + 2] + r[2 * NW + 3]);
    a1b = (r[3 * NW] + r[3 * NW + 1]) + (r[3 * NW + 2] + r[3 * NW + 3]);
    a2b = (r[4 * NW] + r[4 * NW + 1]) + (r[4 * NW + 2] + r[4 * NW + 3]);
  }
  if (ht == 0) {
    if (f == TSFF_FEATURE_ELE) { K.lpart[(size_t)b * 3 + 1] = s0; K.lpart[(size_t)b * 3 + 2] = s1; }
    else K.lpart[(size_t)b * 3 + 0] = s0;
  }
  if (raw) sn = a1b = a2b = 0.0;
  {
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
    const double cn = sn * invM;
    const int s_first = 4 * ht - pstar - S.toff[f], nt = S.ntaps[f];   // tap index of the thread's first sample against the arg-max bin
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * ht + r, st = s_first + r;
      const double xb = (st >= 0 && st < nt) ? __builtin_fma(-cn, m.taps[3 + st], sx[r]) : sx[r];   // (padded copy: hb[s] at 3 + s)
      xs[XA(i)] = xb * wpre[r];
    }
  }
  __syncthreads();
  constexpr int NLB = 9 + 3 * NI;
  LineS<NI> LB;
  zero_lines<NI>(LB);
#pragma unroll
  for (int q = 0; q < kStrip; ++q) {
    const double xb = xs[XA(JQ(q))];
    LB.wpe2 += xb * J[q].wpe2; LB.wL += xb * J[q].wL; LB.kL += xb * J[q].kL; LB.ivTe += xb * J[q].ivTe;
    LB.a_e += xb * J[q].a_e; LB.Ud += xb * J[q].Ud; LB.Vd += xb * J[q].Vd; LB.m += xb * J[q].m;
    LB.pref += xb * xa[q];            // d x_j / d pref = x_j / pref (the factor 1/pref below)
#pragma unroll
    for (int s = 0; s < NI; ++s) { LB.ixi[s] += xb * J[q].ixi[s]; LB.a_i[s] += xb * J[q].a_i[s]; LB.cs[s] += xb * J[q].cs[s]; }
  }
  LB.pref *= 1.0 / L.pref;
#pragma unroll
  for (int s = 0; s < NI; ++s) LB.a_i[s] *= -0.5;   // deferred factor of point_fused
  // Every wavefront leaves the sums of its 64 lanes in global memory and is done: the sum over the four wavefronts and the two
  // features, the chain rule to the physical parameters (make_lines_adjoint), Ti tying, fraction renormalisation, activation and
  // the gradient mask are the work of one thread per LINEOUT in k_fused_finish, which runs behind this kernel in place of
  // k_loss_reduce -- in round 2 they were 1.8 us of one lane's latency plus two barriers at the end of every workgroup.
  {
    double lb[kLBRec];
    lines_adj_store<NI>(LB, lb);
#pragma unroll
    for (int k = 0; k < NLB; ++k) lb[k] = wave_sum(lb[k]);
    lb[NLB] = a1b; lb[NLB + 1] = a2b;   // (block sums: the same in every wavefront's record; the finish kernel reads wavefront 0's)
    // (component-major: lbrec[(k NW + hw) nitems + item] -- k_fused_finish reads it with one item per lane)
    const size_t nitems = (size_t)K.Btot * (interleaved ? 2 : 1);
    double mine = 0.0;
#pragma unroll
    for (int k = 0; k < NLB + 2; ++k) mine = lane == k ? lb[k] : mine;
    if (lane < NLB + 2) K.lbrec[((size_t)lane * NW + hw) * nitems + gitem] = mine;
  }
  TSFF_STAMP(8);
}

// k_fused_prep: the lineout scalars of every (lineout, feature) item of a k_spectrum_fused launch -- one thread per item, the
// very code of the spectrum kernels (load_phys, make_lines: the same bits), plus the four physical parameters the instrument chain
// reads.  lrec[item][kLineRec]: the line record (lines_store) | lam, amp1, amp2, amp3.
// finrec[k][item] (component-major, read by k_fused_finish with one item per lane): the physical parameters and the sum of the
// un-normalised fractions (NP + 1), sigmoid(x) of the slots that have one (NP), and the lineout scalars once more (9 + 4 n_ion).
template <int NI>
__global__ __launch_bounds__(64) void k_fused_prep(KStatic S, const double* __restrict__ params, int B, int f0, int nload,
                                                   double* __restrict__ lrec, double* __restrict__ finrec) {
  constexpr int NPk = TSFF_NP(NI);
  const int item = blockIdx.x * 64 + threadIdx.x;
  if (item >= B * nload) return;
  const size_t nitems = (size_t)B * nload;
  const int l = item / B, b = item - l * B, f = nload == 2 ? l : f0;
  const double* __restrict__ x = params + (size_t)b * S.NP;
  double sgv[NPk];
#pragma unroll
  for (int s = 0; s < NPk; ++s) sgv[s] = S.p_sig[s] ? sigmoid(x[s]) : 0.0;
  Phys<NI> p;
  load_phys<NI>(x, S.p_scale, S.p_shift, S.p_sig, S.ti_same, true, p, sgv);
  LineS<NI> L;
  make_lines<NI>(p, S.lam_shift[f], 0, 1, L);
  {
    double ph[NPk + 1];
    phys_to_array<NI>(p, ph);
    double* __restrict__ q = finrec + item;
#pragma unroll
    for (int k = 0; k <= NPk; ++k) q[(size_t)k * nitems] = ph[k];
#pragma unroll
    for (int k = 0; k < NPk; ++k) q[(size_t)(NPk + 1 + k) * nitems] = sgv[k];
    lines_store<NI>(L, q + (size_t)(2 * NPk + 1) * nitems, nitems);
  }
  double* __restrict__ r = lrec + (size_t)item * kLineRec;
  lines_store<NI>(L, r, 1);
  r[9 + 4 * NI] = p.lam; r[10 + 4 * NI] = p.amp1; r[11 + 4 * NI] = p.amp2; r[12 + 4 * NI] = p.amp3;
}

// k_fused_finish: what remains of a fit step after k_spectrum_fused -- one thread per (lineout, feature) item, 256-thread
// workgroups.  Per item: the sums of the lineout-scalar adjoints over the four wavefronts of its workgroup (fixed order), the
// chain rule to the physical parameters (make_lines_adjoint), amplitudes, Ti tying, fraction renormalisation
// (ts_params.py:543-563), activation (ts_params.py:329-350) and the gradient mask.  With two loaded features the items of a
// lineout sit in neighbouring lanes and are added by one lane exchange.  Output either grad[B][NP] + out[3] (tsff_loss_grad) or
// the packed buffer of tsff_loss_grad_packed (see k_loss_reduce_packed: this rank's columns [b_off, b_off + B) of
// [3 | n_act x B_global], zeros elsewhere).  The loss sums are reduced by workgroup 0 exactly as in k_loss_reduce: the same bits.
// gm: the kernel's GM (1: the DLM order is a leaf).
template <int NI>
__global__ __launch_bounds__(kThreads) void k_fused_finish(KStatic S, const double* __restrict__ finrec, const double* __restrict__ lbrec,
                                                     const double* __restrict__ lpart, int B, int f0, int nload, int gm,
                                                     const uint8_t* __restrict__ gmask, double* __restrict__ grad,
                                                     double* __restrict__ loss_out, const int* __restrict__ act, int n_act,
                                                     long B_global, long b_off, double* __restrict__ packed) {
  constexpr int NPk = TSFF_NP(NI), NLB = 9 + 3 * NI, NW = kHalf / 64;
  __shared__ double red[8];
  const int lane = threadIdx.x;                        // (index inside the workgroup)
  const int per_wg = kThreads / nload;                 // lineouts per workgroup
  if (blockIdx.x == gridDim.x - 1) {
    // the LAST workgroup holds no items: it reduces the loss sums, beside the others instead of behind workgroup 0's items (the
    // loop is a chain of memory latencies: eight iterations' loads are requested at once, the additions keep k_loss_reduce's order)
    double a[3] = {0.0, 0.0, 0.0};
    constexpr int U = 8;
    for (int b0 = threadIdx.x; b0 < B; b0 += U * kThreads) {
      double v[U][3];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int bb = b0 + u * kThreads;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[u][k] = bb < B ? lpart[(size_t)bb * 3 + k] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (b0 + u * kThreads < B) { a[0] += v[u][0]; a[1] += v[u][1]; a[2] += v[u][2]; }
    }
    double* out = packed ? packed : loss_out;
    for (int k = 0; k < 3; ++k) {
      const double v = block_sum(a[k], red);
      if (threadIdx.x == 0) out[k] = v;
    }
    return;
  }
  const int b = blockIdx.x * per_wg + lane / nload, l = nload == 2 ? (lane & 1) : 0;
  // (the slot list first: behind the stores to `packed`, which may alias it for all the compiler knows, every read of it would be
  //  a fresh round trip to memory)
  int actv[NPk];
#pragma unroll
  for (int k = 0; k < NPk; ++k) actv[k] = (packed && k < n_act) ? act[k] : -1;
  const size_t nitems = (size_t)B * nload;
  double gv[NPk];
#pragma unroll
  for (int s = 0; s < NPk; ++s) gv[s] = 0.0;
  if (b < B) {
    const int f = nload == 2 ? l : f0;
    const size_t item = (size_t)l * B + b;
    // physical parameters, sigmoids and lineout scalars as k_fused_prep left them (no activation, square root or division here)
    const double* __restrict__ q = finrec + item;
    double ph[NPk + 1], sgv[NPk];
#pragma unroll
    for (int k = 0; k <= NPk; ++k) ph[k] = q[(size_t)k * nitems];
#pragma unroll
    for (int k = 0; k < NPk; ++k) sgv[k] = q[(size_t)(NPk + 1 + k) * nitems];
    Phys<NI> p;
    phys_from_lds<NI>(ph, p);
    q += (size_t)(2 * NPk + 1) * nitems;
    LineS<NI> L;
    lines_load<NI>(q, nitems, [](double v) { return v; }, L);
    double lb[NLB];
#pragma unroll
    for (int k = 0; k < NLB; ++k) {
      const double* __restrict__ r = lbrec + (size_t)k * NW * nitems + item;
      lb[k] = (r[0] + r[nitems]) + (r[2 * nitems] + r[3 * nitems]);
    }
    const double a1b = lbrec[(size_t)NLB * NW * nitems + item], a2b = lbrec[(size_t)(NLB + 1) * NW * nitems + item];
    LineS<NI> LB;
    zero_lines<NI>(LB);
    lines_adj_load<NI>(lb, true, LB);
    double g[NPk];
#pragma unroll
    for (int s = 0; s < NPk; ++s) g[s] = 0.0;
    make_lines_adjoint<NI>(p, S.lam_shift[f], 0, 1, L, LB, g);
    amp_adjoint(f, a1b, a2b, g);
    tie_renorm_adjoint<NI>(S, p, gm == 1, g);
#pragma unroll
    for (int s = 0; s < NPk; ++s) gv[s] = activation_adjoint(g[s], S.p_scale[s], S.p_sig[s], [&] { return sgv[s]; }, gmask[s]);
  }
  if (nload == 2) {   // electron-feature part + ion-feature part (k_loss_reduce's order), in the even lane
#pragma unroll
    for (int s = 0; s < NPk; ++s) {
      const double o = __shfl_xor(gv[s], 1, 64);
      gv[s] = (lane & 1) ? 0.0 : gv[s] + o;
    }
  }
  if (b < B && l == 0) {
    if (packed) {
#pragma unroll
      for (int k = 0; k < NPk; ++k) {
        double v = 0.0;
#pragma unroll
        for (int s = 0; s < NPk; ++s) v = actv[k] == s ? gv[s] : v;
        if (actv[k] >= 0) packed[3 + (size_t)k * B_global + b_off + b] = v;
      }
    } else {
#pragma unroll
      for (int s = 0; s < NPk; ++s) grad[(size_t)b * NPk + s] = gv[s];
    }
  }
  if (packed) {   // the columns of the other ranks: zero (the buffer is all-reduced in place step after step)
    const long n = (long)n_act * B_global;
    if ((long)B < B_global)
      for (long i = (long)blockIdx.x * kThreads + lane; i < n; i += (long)(gridDim.x - 1) * kThreads) {
        const long k = i / B_global, bl = i - k * B_global - b_off;
        if (bl < 0 || bl >= B) packed[3 + i] = 0.0;
      }
  }
}
