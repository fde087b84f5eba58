// k_conv.inc -- the phase-layout IRF convolution of the spectrum kernels (points_per_pixel = 1, 256 threads per feature): the sixteen
// FMAs of a tap group, once, and the software-pipelined loop around them (conv4_phase) that k_spectrum_fused and k_forward_pairs run.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff, in front of k_spectrum.inc, whose own rolled
// loops share the tap group and nothing else).

// One tap group: four adjacent outputs y[r] += sum_c g_c V[r + c] over the seven window values V0 .. V6.  The explicit FMA chains
// pin the roundings: every kernel that convolves in the phase layout adds the same products in the same order -- the same bits.
__device__ __forceinline__ void conv_taps4(double g0, double g1, double g2, double g3, double V0, double V1, double V2, double V3,
                                           double V4, double V5, double V6, double& y0, double& y1, double& y2, double& y3) {
  y0 = __builtin_fma(g3, V3, __builtin_fma(g2, V2, __builtin_fma(g1, V1, __builtin_fma(g0, V0, y0))));
  y1 = __builtin_fma(g3, V4, __builtin_fma(g2, V3, __builtin_fma(g1, V2, __builtin_fma(g0, V1, y1))));
  y2 = __builtin_fma(g3, V5, __builtin_fma(g2, V4, __builtin_fma(g1, V3, __builtin_fma(g0, V2, y2))));
  y3 = __builtin_fma(g3, V6, __builtin_fma(g2, V5, __builtin_fma(g1, V4, __builtin_fma(g0, V3, y3))));
}

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
typedef const double __attribute__((address_space(4))) cdouble_t;
typedef const double __attribute__((address_space(3))) ldouble_t;
struct ConvSet { double w[11], g[8]; };
// groups a, a + 1: the window values V0 .. V6 of the first, V3 .. V6 of the second and their taps.  (V0 .. V2 are the V4 .. V6 of
// the group before and could be inherited from the previous set -- but then three registers of a set are still read when the set
// is requested again, the allocator loads into temporaries and copies them behind a wait of its own in the middle of the FMAs.)
// r12_loops: the window through four RUNNING LDS addresses p0 .. p3 (one per phase array, at group a of the loop body) and the
// set's offset O = 0, 2, 4 from them as an immediate -- one address step per phase array and body, where the index form cost two.
// And the compiler did inherit after all: it found w[8 .. 10] of one request in w[0 .. 2] of the next (the same LDS words), kept
// those three and their ds_read2 partners -- six doubles -- across the request that reuses their registers and paid six v_mov_b64 per
// body for it.  The empty asm makes the four addresses opaque in front of every request, so that each request reads its own
// eleven values (three LDS reads more per body, no VALU instruction); the taps keep their running scalar pointer.
template <int DIR, int O>
__device__ __forceinline__ void conv_request(ldouble_t*& p0, ldouble_t*& p1, ldouble_t*& p2, ldouble_t*& p3, cdouble_t* pt, int at,
                                             ConvSet& s) {
  asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));
  s.w[0] = p0[O]; s.w[1] = p1[O]; s.w[2] = p2[O];
  s.w[3] = p3[O]; s.w[4] = p0[O + 1]; s.w[5] = p1[O + 1]; s.w[6] = p2[O + 1];
  s.w[7] = p3[O + 1]; s.w[8] = p0[O + 2]; s.w[9] = p1[O + 2]; s.w[10] = p2[O + 2];
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
  const double* w = s.w + 4 * H, * g = s.g + 4 * H;
  conv_taps4(g[0], g[1], g[2], g[3], w[0], w[1], w[2], w[3], w[4], w[5], w[6], acc[0], acc[1], acc[2], acc[3]);
}
template <int DIR>
__device__ __forceinline__ void conv4_phase(const double* __restrict__ xs, int Ls, int sl, cdouble_t* pt, int na, double (&acc)[4]) {
  ldouble_t* p0 = (ldouble_t*)xs + sl, * p1 = p0 + Ls, * p2 = p1 + Ls, * p3 = p2 + Ls;   // X0 .. X3 at group a
  ConvSet A, B;
  conv_request<DIR, 0>(p0, p1, p2, p3, pt, 0, A);
  int a = 0;
  for (; a + 4 <= na; a += 4) {   // two sets per body: A holds groups a, a + 1 on entry
    conv_wait();
    conv_request<DIR, 2>(p0, p1, p2, p3, pt, 2, B);
    conv_group<0>(A, acc); conv_group<1>(A, acc);
    conv_wait();
    conv_request<DIR, 4>(p0, p1, p2, p3, pt, 4, A);
    conv_group<0>(B, acc); conv_group<1>(B, acc);
    pt += 16 * DIR;   // (the taps through a running scalar pointer, the window through four running addresses)
    p0 += 4; p1 += 4; p2 += 4; p3 += 4;
  }
  // the last na - a = 0 .. 3 groups: A holds the first two of them (requested, not yet waited for)
  conv_wait();
  if (na - a >= 2) {
    conv_request<DIR, 2>(p0, p1, p2, p3, pt, 2, B);
    conv_group<0>(A, acc); conv_group<1>(A, acc);
    conv_wait();
    if (na - a == 3) conv_group<0>(B, acc);
  } else if (na - a == 1) {
    conv_group<0>(A, acc);
  }
}
