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
  // lrec: [items][kLineRec] the lineout scalars of every (lineout, feature) item, written by k_fused_prep just before this launch,
  // and behind them, in the same buffer, [items][n_angles][2] the angle records (cos theta_a, w_a pref) of the items
  // flags as in k_spectrum: bit 1 k_s cache in LDS, bit 2 interleaved plan (grid 2B: workgroup f B + b evaluates feature f
  // of lineout b and leaves its part of the gradient in K.gpart[f][b][:]); otherwise grid B, feature f0, grad written
  const bool use_ks = flags & kFlagKsCache, interleaved = flags & kFlagInterleaved;
  const int item = blockIdx.x;
  const int f_il = interleaved ? (int)(item >= K.B) : 0;
  const int b = K.b0 + item - f_il * K.B, tid = threadIdx.x;
  // (item of the whole batch: the records of k_fused_prep / for k_fused_finish are laid out over all Btot lineouts, whatever
  //  column block this launch covers)
  const size_t gitem = (size_t)f_il * K.Btot + b;
  constexpr int TPF = kHalf, NW = TPF / 64;
  // kLeanKs (the DLM instantiation with one species and the lane exchange): what the k_s evaluation needs does not live across the
  // angle loops.  The fallbacks `use_ks ? cache : ks_eval` before and behind the sweeps share their expressions with the k_s cache
  // fill of the prologue, and the compiler kept the fill's intermediates -- and the two frequencies no loop reads -- in registers
  // for them: 17 VGPRs more than the file has, spilled to scratch.  Now the fill works on copies the compiler cannot tell from
  // ws, and the third frequency of a pair is read again where a fallback needs it (w_third): the same values from the same
  // expressions, no scratch.  (Measured, DESIGN.md section 4.1b.)
  constexpr bool kLeanKs = GM == 1 && NI == 1 && EX;
  constexpr bool PAD = kSelectFree<NI>;   // the Hermite lookups read the out-of-grid cell that stage_commit writes (k_pairs.inc)
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
    stage_commit(TSFF_STAGE_ARGS, m, S, K, S.shared_fe ? 0 : b, T, ZH, f, PAD);
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
    if constexpr (kLeanKs) {   // (copies the compiler cannot tell from ws: the cache fill's square-root chains are its own)
      double wsc[2][kPair + 1];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q <= kPair; ++q) { wsc[p][q] = ws[p][q]; asm volatile("" : "+v"(wsc[p][q])); }
      if (use_ks) ks_cache_fill(ksc, jp, wsc, L.wpe2, npts);
    } else {
      if (use_ks) ks_cache_fill(ksc, jp, ws, L.wpe2, npts);
    }
    zero_phase_halos(xs, Ls, hs, ht, TPF);
  }
  // Away from the laser line every point of a wavefront's pair sees |xi_i| >> 1: the ion terms are the asymptote and
  // exp(-xi_i^2) = 0 exactly (point_core<FAR>).  Decided once per (wavefront, pair) from a bound that holds for all its 128
  // samples (and the right neighbour of the last one), all angles and all species (far_range, tsff_device.h).
  // The two ends of a unit -- sample 128 hw (+ 512) and the sample right of its last one -- are the first frequency of lane 0 and
  // the third of lane 63: read from those lanes' registers, not from memory again.
  double w_lo[2], w_hi[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    w_lo[p] = lane_f64(ws[p][0], 0);
    w_hi[p] = lane_f64(ws[p][kPair], 63);
  }
  // (kLeanKs) the third frequency of a pair -- no angle loop reads it: the lane exchange stands for its base point -- comes from the
  // frequency axis again where the fallbacks of the k_s cache before and behind the sweeps read it, by a load of its own each
  // time, instead of living in a register across the four angle loops
  auto w_third = [&](int p) {
    const double* o = omgs;
    int t = ht;
    asm volatile("" : "+s"(o), "+v"(t));   // (the address too is formed here, not kept from the prologue)
    return o[min(kPair * t + p * (npts / 2) + kPair, npts - 1)];
  };
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
    if (lane < 32 && ab < NA) unit_boundary_fill<NI, PAD>(ex_wse, m.cosa[ab], L, T, exb + 16 * (2 * hw + Pb) + ab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (the sweep reads other lanes' boundary points)
  }
  // (the item's angle record, behind the line records of ALL items of the batch; wavefront-uniform address, constant address space: scalar loads)
  cdouble_t* arp = (cdouble_t*)(lrec + (size_t)K.Btot * (interleaved ? 2 : 1) * kLineRec + gitem * 2 * (size_t)NA);
  auto sweep = [&](auto pair_tag, auto far_tag) {
    constexpr int P = decltype(pair_tag)::value;
    constexpr bool FAR = decltype(far_tag)::value;
    const int jb = jp[P];
    const int j2 = min(jb + kPair, npts - 1);
    double wr[kPair + 1];
    if constexpr (kLeanKs) {
#pragma unroll
      for (int q = 0; q <= kPair; ++q) wr[q] = q == kPair ? w_third(P) : ws[P][q];
    }
    const double (&wP)[kPair + 1] = [&]() -> const double (&)[kPair + 1] { if constexpr (kLeanKs) return wr; else return ws[P]; }();
    const double ks2 = EX ? (use_ks ? ksc[j2] : ks_eval(wP[kPair], L.wpe2)) : 0.0;
    // The angle's constants (cos theta_a, w_a pref) come from the item's record of k_fused_prep by ONE scalar load, straight into
    // SGPRs, one iteration ahead of their use: wavefront-uniform and independent of the sample, they were two LDS reads, a
    // multiplication and four v_readfirstlane_b32 per iteration.  The product is k_fused_prep's: the same factors, the same bits.
    cdouble_t* pn = arp;
    double ct_n = pn[0], wa_n = pn[1];
    // (EX) the unit's boundary point, which lane 63 takes for its missing neighbour
    const double* exu = EX ? exb + 16 * (2 * hw + P) : nullptr;
    // (pair_step_sched) k_s of the pair's two samples, which no angle changes: read once, not at the head of every iteration, where
    // nothing stands between the read and the square root that waits for it
    double ksa = 0.0, ksb = 0.0;
    if constexpr (kSweepSched<NI, GM, ZH, EX>) {
      ksa = use_ks ? ksc[jb] : ks_eval(ws[P][0], L.wpe2);
      ksb = use_ks ? ksc[min(jb + 1, npts - 1)] : ks_eval(ws[P][1], L.wpe2);
    }
    for (int a = 0; a < NA; ++a) {
      const double ct = ct_n, wa = wa_n;
      { pn += a + 1 < NA ? 2 : 0; ct_n = pn[0]; wa_n = pn[1]; }   // (entry min(a + 1, NA - 1))
      if constexpr (kSweepSched<NI, GM, ZH, EX>) {   // the two points of the pair in flight together (pair_step_sched, k_pairs.inc)
        constexpr int q0 = kPair * P;
        static_assert(kPair == 2, "pair_step_sched is written out for two points");
        pair_step_sched<NI, GM, ZH, FAR, PAD>(ws[P], ksa, ksb, ks2, exu + a, pair_has_next<NI, P, 2>(1, jb + 1, npts), L, T, ct, wa, cw,
                                              xa[q0], J[q0], KA[q0], xa[q0 + 1], J[q0 + 1], KA[q0 + 1]);
        continue;
      }
      Base b0;
      base_eval<NI, PAD>(wP[0], use_ks ? ksc[jb] : ks_eval(wP[0], L.wpe2), ct, L, T, b0);
      // (EX) the lane's FIRST base point of this angle is what its left neighbour asks for: b0 itself is the second one by then
      const Base b0f = b0;
#pragma unroll
      for (int i = 0; i < kPair; ++i) {
        constexpr int q0 = kPair * P;
        const int q = q0 + i, j = jb + i;
        const bool has_next = pair_has_next<NI, P, 2>(i, j, npts);
        Base b1;
        if (EX && i == kPair - 1) {   // the neighbour lane's first base point (the unit's boundary point for the last lane)
          // (The boundary point is read HERE.  Read an iteration ahead, as ct_n / wa_n are, or at the top of the iteration, its five
          //  doubles live across the pair's first point and the allocator spills 26 / 10 registers outside the loops where this form
          //  spills none; measured, DESIGN.md section 4.1b.  Tried again with the angle constants in SGPRs: still six.)
          neighbour_take<NI>(b0f, exu + a, ks2, ct, L, b1);
        } else {
          base_eval<NI, PAD>(wP[i + 1], use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(wP[i + 1], L.wpe2), ct, L, T, b1);
        }
        row_step<NI, GM, ZH, FAR, PAD>(b0, b1, has_next, L, T, ct, wa, cw, xa[q], J[q], KA[q]);
        b0 = b1;
      }
    }
  };
  if (far0) sweep(std::integral_constant<int, 0>{}, std::true_type{}); else sweep(std::integral_constant<int, 0>{}, std::false_type{});
  if (far1) sweep(std::integral_constant<int, 1>{}, std::true_type{}); else sweep(std::integral_constant<int, 1>{}, std::false_type{});
  TSFF_STAMP_WAVE(9);
  double wl[2][kPair + 1];
  if constexpr (kLeanKs) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q <= kPair; ++q) wl[p][q] = q == kPair ? w_third(p) : ws[p][q];
  }
  const double (&wq)[2][kPair + 1] = [&]() -> const double (&)[2][kPair + 1] { if constexpr (kLeanKs) return wl; else return ws; }();
#pragma unroll
  for (int q = 0; q < kStrip; ++q) {   // the k_L and omega_pe^2 columns of the rows from their angle sums (see KsAcc)
    const int j = JQ(q);
    const double ksa = use_ks ? ksc[j] : ks_eval(wq[q >> 1][q & 1], L.wpe2);
    const double ksb = use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(wq[q >> 1][(q & 1) + 1], L.wpe2);
    ks_columns<NI>(KA[q], ksa, ksb, L, J[q]);
  }
  {   // the factor ws^2 (left out of the sweep) and the notch filter of the electron feature: x_j and xbar_j carry it
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
#pragma unroll
    for (int q = 0; q < kStrip; ++q) store_scaled(xs + XA(JQ(q)), xa[q], wq[q >> 1][q & 1], filt, S.filt, JQ(q));
  }
  __syncthreads();
  TSFF_STAMP(3);

  // ================= IRF convolution ("same"), bin average, normalisation (phase layout, see k_spectrum) =================
  constexpr int BPT = 4;
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
    // (one grouped reduction, wave_sums_scatter: 9 exchanges instead of 30, wave_sum's bits; the lane that holds sum k stores it)
    const double v5[5] = {s0, s1, sn, a1b, a2b};
    const double v = wave_sums_scatter<5>(v5, lane);
    bool own;
    const int k = scatter_lane<5>(lane, own);
    if (own) m.red[kRedSums + k * NW + hw] = v;   // (behind the slots of half_argmax, which a slower wavefront may still read)
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
  // (the factors 1 / pref of LB.pref -- d x_j / d pref = x_j / pref -- and -0.5 of LB.a_i, which point_fused defers, are applied in the
  //  reduction below)
  // Every wavefront leaves the sums of its 64 lanes in global memory and is done: the sum over the four wavefronts and the two
  // features, the chain rule to the physical parameters (make_lines_adjoint), Ti tying, fraction renormalisation, activation and
  // the gradient mask are the work of one thread per LINEOUT in k_fused_finish, which runs behind this kernel in place of
  // k_loss_reduce -- in round 2 they were 1.8 us of one lane's latency plus two barriers at the end of every workgroup.
  {
    double lb[kLBRec];
    lines_adj_store<NI>(LB, lb);
    // One grouped reduction (wave_sums_scatter_scaled, tsff_device.h): the first lane of the group of four that holds sum k stores it,
    // and the 63 copies of each sum that the butterflies made and threw away are not made.  The two factors go in with it: the same
    // bits as the butterflies of the scaled values gave.
    double lbs[NLB], lbc[NLB];
    constexpr unsigned scaled = (1u << 5) | (1u << 9) | (NI > 1 ? 1u << 12 : 0u);   // (lines_adj_store: pref, a_i[s])
#pragma unroll
    for (int k = 0; k < NLB; ++k) { lbs[k] = lb[k]; lbc[k] = k == 5 ? 1.0 / L.pref : ((scaled >> k) & 1u) ? -0.5 : 1.0; }
    double mine = wave_sums_scatter_scaled<NLB, scaled>(lbs, lbc, lane);
    bool own;
    int k = scatter_lane<NLB>(lane, own);
    // (block sums: the same in every wavefront's record; the finish kernel reads wavefront 0's.  Lanes 1 and 2 hold no sum to store)
    if (lane == 1) { mine = a1b; k = NLB; }
    if (lane == 2) { mine = a2b; k = NLB + 1; }
    // (component-major: lbrec[(k NW + hw) nitems + item] -- k_fused_finish reads it with one item per lane)
    const size_t nitems = (size_t)K.Btot * (interleaved ? 2 : 1);
    if (own || lane == 1 || lane == 2) K.lbrec[((size_t)k * NW + hw) * nitems + gitem] = mine;
  }
  TSFF_STAMP(8);
}

// k_fused_prep: the lineout scalars of every (lineout, feature) item of a k_spectrum_fused launch -- one thread per item, the
// very code of the spectrum kernels (load_phys, make_lines: the same bits), plus the four physical parameters the instrument chain
// reads.  lrec[item][kLineRec]: the line record (lines_store) | lam, amp1, amp2, amp3.  arec: see below.
// finrec[k][item] (component-major, read by k_fused_finish with one item per lane): the physical parameters and the sum of the
// un-normalised fractions (NP + 1), sigmoid(x) of the slots that have one (NP), and the lineout scalars once more (9 + 4 n_ion).
// arec[item][n_angles][2] (or nullptr: the forward-only pair sweep reads none): the angle constants (cos theta_a, w_a pref) of the
// one-sweep kernel's angle loops -- the product its threads formed in every iteration, once per item.
template <int NI>
__global__ __launch_bounds__(64) void k_fused_prep(KStatic S, const double* __restrict__ params, int B, int f0, int nload,
                                                   double* __restrict__ lrec, double* __restrict__ finrec, double* __restrict__ arec) {
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
  if (arec) {
    double2* __restrict__ ar = reinterpret_cast<double2*>(arec) + (size_t)item * S.n_angles;
    for (int a = 0; a < S.n_angles; ++a) ar[a] = make_double2(S.cos_sa[a], S.w_sa[a] * L.pref);
  }
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
