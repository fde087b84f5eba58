// k_forward.inc -- k_forward_pairs: ThryE / ThryI of one (lineout, feature) item, forward only (tsff_forward; BASELINE configs[1]).
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).
//
// The sweep of k_spectrum_fused without its Jacobian rows: pairs of consecutive samples per thread, the pair's right-neighbour base
// point taken from the next lane (EXM), the asymptotic ion terms per 128-sample unit (FAR), the batched table staging and the
// lineout scalars of k_fused_prep -- and the instrument chain of k_spectrum (phase-layout convolution, arg-max normalisation,
// amplitudes, noise).  Same point functions, same order of the sums: the spectra are the bits k_spectrum and k_spectrum_fused produce.
//   NPAIR = 2: 256 threads per item, thread ht owns the pairs {2 ht, 2 ht + 1} and {512 + 2 ht, 513 + 2 ht};
//   NPAIR = 1: 512 threads per item, thread ht owns the pair {2 ht, 2 ht + 1}: the sweep -- half of an item's latency -- takes half
//     as long.  Batches of up to two items per CU (configs[1]: 256 lineouts x 2 features = 512 items on 256 CUs) run as ONE
//     dispatch round, whose duration IS one workgroup's latency, and the registers of a forward-only sweep (about 110) leave room
//     for 16 wavefronts per CU.  The instrument chain stays on the first 256 threads (four bins each: the phase layout).  In this
//     regime the lineout scalars are computed in the kernel (flags bit 3): a k_fused_prep launch in front costs more than it saves.
//   (Tried and dropped, profiles/r03o: two 256-thread workgroups per item that hand their halves over through global memory with
//    an agent-scope ticket, four per CU with the spectrum buffer overlaying the tables: the release / acquire across XCDs costs more
//    than the halved sweep saves -- 59 us against 52 at B = 256.)
// EXM: how a pair gets its right-neighbour base point: 0 evaluates it itself; 1 and 2 take it from the next lane, register to
// register (next_lane_f64, k_spectrum_fused's exchange), the unit-boundary points of the last lanes through LDS.  (1 was the exchange
// through per-lane LDS slots, 2 the one by ds_bpermute shuffles; both are this one form now.  The planner still names its
// two-workgroups-per-CU choice 1 and its wide / three-per-CU choice 2: the kernel names are what the coverage contract of the
// instantiations lists.)
// Reference rows a4-a13 of SURVEY.md section 8 (form_factor.py:182-298, generate_spectra.py:139-220, irf.py:50-132,
// thomson_diagnostic.py:109-142).  Restrictions (launch_spectrum falls back to k_spectrum): one gradient point, one point per pixel.
// LDS of a forward-only workgroup, laid out for it alone (k_spectrum's carve() reserves the adjoint's reduction scratch): with the
// half Z' table and no k_s cache (of the exchange only the 8 x 16 unit-boundary points live in LDS) a workgroup takes 52 KB --
// THREE per CU, and the sweep's 120 VGPRs leave room for four wavefronts per SIMD.
__host__ __device__ inline size_t smem_fwd_doubles(const KStatic& S, bool with_ks, bool zh, size_t exd) {   // exd: doubles of the exchange
  size_t n = 2 * (size_t)((zh ? kNZh : kNXi2) + S.nvx) + kNXi2 + 4 * (size_t)S.nvx + xbuf_doubles(S);   // zp, ht, W, hc, x
  if (with_ks) n += (size_t)S.npts + 2;
  n += S.ntaps[0] + S.ntaps[1] + 16 + 2 * (size_t)S.n_angles + (kNP_MAX + 2) + 64 + kNExpTab;           // taps, angles, phys, red, exp table
  n += exd;
  return n;
}
__device__ __forceinline__ Smem carve_fwd(unsigned char* smem, const KStatic& S, bool with_ks, bool zh, int exm) {
  Smem m;
  m.zp = reinterpret_cast<double2*>(smem);
  m.ht = m.zp + (zh ? kNZh : kNXi2);
  m.W = reinterpret_cast<double*>(m.ht + S.nvx);
  double* p = m.W + kNXi2;
  m.x = p; m.yb = p; p += xbuf_doubles(S);
  m.hc = reinterpret_cast<double2*>(p); p += 4 * (size_t)S.nvx;   // (nvx cells: nvx - 1 intervals + the out-of-grid cell, stage_commit fills both)
  m.hcm = nullptr; m.Wm = nullptr;
  m.ksc = nullptr;
  if (with_ks) { m.ksc = p; p += S.npts + 2; }
  m.taps = p; p += S.ntaps[0] + S.ntaps[1] + 16;
  m.phys = p; p += kNP_MAX + 2;
  m.cosa = p; p += S.n_angles;
  m.wsa = p; p += S.n_angles;
  m.red = p; p += 64;
  m.etab = p; p += kNExpTab;
  m.ex = exm ? p : nullptr;
  return m;
}
template <int NI, bool ZH, int EXM, int NPAIR>
__global__ __launch_bounds__(kHalf * (3 - NPAIR), 2) void k_forward_pairs(KStatic S, KCall K, int f0, int flags, const double* __restrict__ lrec) {
  constexpr bool EX = EXM != 0;
  constexpr bool PAD = kSelectFree<NI>;   // the Hermite lookups read the out-of-grid cell that stage_commit writes (k_pairs.inc)
  constexpr int NT = kHalf * (3 - NPAIR);   // threads of the workgroup
  const bool use_ks = flags & kFlagKsCache, interleaved = flags & kFlagInterleaved, own_scalars = flags & kFlagOwnScalars;
  const int item = blockIdx.x;
  const int f_il = interleaved ? (int)(item >= K.B) : 0;
  const int b = item - f_il * K.B, tid = threadIdx.x;
  constexpr int TPF = kHalf, NW = NT / 64;
  const int ht = tid, lane = tid & 63, hw = tid >> 6;
  const int f = __builtin_amdgcn_readfirstlane(interleaved ? f_il : f0);
  extern __shared__ __align__(16) unsigned char smem[];
  const Smem m = carve_fwd(smem, S, use_ks, ZH, EXM);
  const int npts = S.npts, NA = S.n_angles;   // npts == 1024
  const int hs = S.hs, Ls = npts / 4 + 2 * hs;
  double* xs = m.x;
  auto XA = [&](int j) { return (j & 3) * Ls + (j >> 2) + hs; };   // phase layout (see k_spectrum)
  Tables T;
  const double* __restrict__ omgs = S.omgs[f];
  int jp[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) jp[p] = (npts / 2) * p + kPair * ht;
  double ws[NPAIR][kPair + 1];
  LineS<NI> L;
  double* __restrict__ ksc = use_ks ? m.ksc : nullptr;
  {
    TSFF_STAGE_LOCALS;
    stage_issue(TSFF_STAGE_ARGS, m, S, K, S.shared_fe ? 0 : b, ZH, f);
    stage_commit(TSFF_STAGE_ARGS, m, S, K, S.shared_fe ? 0 : b, T, ZH, f, PAD);
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
#pragma unroll
      for (int q = 0; q <= kPair; ++q) ws[p][q] = omgs[min(jp[p] + q, npts - 1)];
    if (own_scalars) {   // (one dispatch round: parameter transform and lineout scalars here, per wavefront -- no k_fused_prep launch)
      const double xv = lane < TSFF_NP(NI) ? K.params[(size_t)b * S.NP + lane] : 0.0;
      stage_phys_wave<NI>(S, xv, m.phys, lane);
      Phys<NI> p;
      phys_from_lds<NI>(m.phys, p);
      make_lines_uniform<NI>(p, S.lam_shift[f], 0, 1, L);
    } else {   // the lineout scalars as k_fused_prep left them (wavefront-uniform address)
      lines_load<NI>(lrec + (size_t)item * kLineRec, 1, [](double v) { return uni(v); }, L);
    }
    if (use_ks) ks_cache_fill(ksc, jp, ws, L.wpe2, npts);
    zero_phase_halos(xs, Ls, hs, ht, NT);
  }
  // the two ends of a wavefront's 128-sample unit: first frequency of lane 0, third of lane 63 (see k_spectrum_fused)
  double w_hi[NPAIR];
  bool far[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) {
    w_hi[p] = lane_f64(ws[p][kPair], 63);
    far[p] = far_range_w<NI>(lane_f64(ws[p][0], 0), w_hi[p], L);
  }
  const double ex_wse = (NPAIR == 2 && ((lane >> 4) & 1)) ? w_hi[NPAIR - 1] : w_hi[0];
  __syncthreads();
  double* exb = m.ex;
  auto unit_of = [&](int P) { return NPAIR == 1 ? hw : 2 * hw + P; };   // 128-sample unit of this wavefront's pair P
  if (EX) {   // the unit-boundary base points of this wavefront's unit(s), all angles at once (lane = 16 P + a)
    const int Pb = (lane >> 4) & 1, ab = lane & 15;
    if (lane < 16 * NPAIR && ab < NA) unit_boundary_fill<NI, PAD>(ex_wse, m.cosa[ab], L, T, exb + 16 * unit_of(Pb) + ab);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  double xa[NPAIR][kPair];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) xa[p][0] = xa[p][1] = 0.0;
  auto sweep = [&](auto pair_tag, auto far_tag) {
    constexpr int P = decltype(pair_tag)::value;
    constexpr bool FAR = decltype(far_tag)::value;
    const int jb = jp[P];
    const int j2 = min(jb + kPair, npts - 1);
    const double ks2 = EX ? (use_ks ? ksc[j2] : ks_eval(ws[P][kPair], L.wpe2)) : 0.0;
    double ct_n = m.cosa[0], wa_n = m.wsa[0];
    for (int a = 0; a < NA; ++a) {
      const double ct = uni(ct_n), wa = uni(wa_n * L.pref);
      { const int an = min(a + 1, NA - 1); ct_n = m.cosa[an]; wa_n = m.wsa[an]; }
      Base b0;
      base_eval<NI, PAD>(ws[P][0], use_ks ? ksc[jb] : ks_eval(ws[P][0], L.wpe2), ct, L, T, b0);
      const Base b0f = b0;   // (the thread's FIRST base point of this angle: what its left neighbour asks for)
#pragma unroll
      for (int i = 0; i < kPair; ++i) {
        const int j = jb + i;
        const bool has_next = pair_has_next<NI, P, NPAIR>(i, j, npts);
        Base b1;
        if (EX && i == kPair - 1) {   // the next lane's first base point; the last lane takes the unit's boundary point
          // (The forward value reads xi_e and F of this point alone: the compiler drops the other three shifts and their boundary reads)
          neighbour_take<NI>(b0f, exb + 16 * unit_of(P) + a, ks2, ct, L, b1);
        } else {
          base_eval<NI, PAD>(ws[P][i + 1], use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(ws[P][i + 1], L.wpe2), ct, L, T, b1);
        }
        xa[P][i] = __builtin_fma(wa, point_forward_sd<NI, ZH, FAR>(b0, b1, has_next, L, T), xa[P][i]);
        b0 = b1;
      }
    }
  };
  if (far[0]) sweep(std::integral_constant<int, 0>{}, std::true_type{}); else sweep(std::integral_constant<int, 0>{}, std::false_type{});
  if constexpr (NPAIR == 2) {
    if (far[1]) sweep(std::integral_constant<int, 1>{}, std::true_type{}); else sweep(std::integral_constant<int, 1>{}, std::false_type{});
  }
  {   // the factor ws^2 (left out of the sweep) and the notch filter of the electron feature
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
#pragma unroll
    for (int p = 0; p < NPAIR; ++p)
#pragma unroll
      for (int i = 0; i < kPair; ++i) store_scaled(xs + XA(jp[p] + i), xa[p][i], ws[p][i], filt, S.filt, jp[p] + i);
  }
  __syncthreads();

  // ================= IRF convolution ("same"), normalisation, amplitudes, noise (as k_spectrum) =================
  constexpr int BPT = 4;
  const bool raw = S.raw[f], chain = NT == TPF || tid < TPF;   // (512-thread form: the chain runs on the first four wavefronts)
  const int hc4 = chain ? ht : 0;
  const size_t row4 = (size_t)b * TSFF_NBINS + 4 * hc4;
  double npre[BPT], lpre[BPT];
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    npre[r] = K.noise[f] ? K.noise[f][row4 + r] : 0.0;
    lpre[r] = f == TSFF_FEATURE_ELE ? S.lam_bin[f][4 * hc4 + r] : 0.0;
  }
  const double amps = raw ? 1.0 : K.amps[f][b];
  double p_lam_v, p_amp1_v, p_amp2_v, p_amp3_v;
  if (own_scalars) { p_lam_v = m.phys[TSFF_P_LAM]; p_amp1_v = m.phys[TSFF_P_AMP1]; p_amp2_v = m.phys[TSFF_P_AMP2]; p_amp3_v = m.phys[TSFF_P_AMP3]; }
  else {
    const double* __restrict__ lrp = lrec + (size_t)item * kLineRec + 9 + 4 * NI;   // (physical lam, amp1, amp2, amp3)
    p_lam_v = lrp[0]; p_amp1_v = lrp[1]; p_amp2_v = lrp[2]; p_amp3_v = lrp[3];
  }
  double ybin[BPT] = {0.0, 0.0, 0.0, 0.0};
  if (chain) conv4_phase<1>(xs, Ls, hc4 + S.cf_a0[f] + hs, (cdouble_t*)(S.ptaps[f] + S.cf_i0[f]), S.cf_na[f], ybin);
  double M = chain ? ybin[0] : -1.0e300;
  int pstar = chain ? 4 * hc4 : TSFF_NBINS;
  if (chain) {
#pragma unroll
    for (int r = 1; r < BPT; ++r)
      if (ybin[r] > M) { M = ybin[r]; pstar = 4 * hc4 + r; }
  }
  half_argmax<NW>(M, pstar, m.red, 0, hw, lane);
  if (!chain) return;
  const double invM = raw ? 1.0 : 1.0 / M;
  const double p_lam = uni(p_lam_v), p_amp1 = uni(p_amp1_v), p_amp2 = uni(p_amp2_v), p_amp3 = uni(p_amp3_v);
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const double A = bin_amplitude(f, raw, amps, lpre[r], p_lam, p_amp1, p_amp2, p_amp3);
    K.thry[f][row4 + r] = thry_value(A, ybin[r], invM, K.noise[f] != nullptr, npre[r]);   // thomson_diagnostic.py:139-140
  }
}
