// k_spectrum_rows.inc -- k_spectrum_rows: the one-sweep loss + gradient kernel for points_per_pixel > 1 (the reference's default
// decks: 5 points per pixel, 5120 wavelength samples per feature).  Part of the single translation unit tsff_kernels.hip
// (included inside namespace tsff, after k_pairs.inc whose per-point functions and sweep steps it uses).
//
// k_spectrum_fused keeps the Jacobian rows J[j][k] of a thread's four samples in registers until the adjoint xbar_j of the
// spectrum is known.  With npts = 1024 ppp samples a thread owns 4 ppp of them and the rows no longer fit: here the sweep runs
// in ppp ROUNDS of 1024 samples (the same two pairs per thread, the same 128-sample units for the asymptotic ion terms) and
// each round's rows go to a scratch array in global memory, component-major [NROW][npts] per workgroup, written as 16-byte
// pieces of consecutive lanes.  The contraction grad_k = sum_j xbar_j J[j][k] afterwards needs no ownership at all: the thread
// that produces xbar_i in the adjoint convolution reads row i (consecutive i on consecutive lanes).  The scratch is written
// once and read once -- 2 x NROW x 8 B per sample against the ~250 instructions per point of a second sweep.
// LDS: the tables of the sweep (Z', W, Hermite coefficients) and the buffers of the instrument chain (spectrum with its halo,
// per-bin adjoint) are never live together -- the spectrum values travel through the scratch too (they are the row component
// `x`) -- so the chain's buffers overlay the tables: 67 KB at 5 points per pixel where k_spectrum needs 105 KB, i.e. two
// workgroups per CU instead of one 512-thread workgroup per launch and feature.
//
// Restrictions (launch_spectrum falls back to k_spectrum otherwise): loss + gradient, one gradient point, n_ion <= 2, no table
// adjoints (GM <= 1), an instrument response on both features.
// Reference rows: as k_spectrum_fused (SURVEY.md section 8 a4-a15).

// row components in the scratch: the adjoint-carrying fields of LineS in the order of lb[] below, then the forward value
template <int NI, int GM>
struct RowsLayout {
  static constexpr int kX = 7 + 3 * NI + (GM == 1 ? 1 : 0);   // index of the forward value x_j (before ws^2 and the filter)
  static constexpr int kN = kX + 1;
};
__host__ __device__ inline int rows_components(int n_ion, int gm) { return 8 + 3 * n_ion + (gm == 1 ? 1 : 0); }

// LDS budget in doubles: persistent [taps | phys | cosa | wsa | red | etab], then the larger of the sweep's tables and the chain's buffers
__host__ __device__ inline size_t rows_persist_doubles(const KStatic& S) {
  return (size_t)S.ntaps[0] + S.ntaps[1] + (kNP_MAX + 2) + 2 * (size_t)S.n_angles + (10 * kNP_MAX + 64) + kNExpTab + 1;   // (+1: alignment pad)
}
__host__ __device__ inline size_t rows_sweep_doubles(const KStatic& S, int gm, bool zh, size_t exd) {
  return 2 * (size_t)((zh ? kNZh : kNXi2) + S.nvx) + kNXi2 + 4 * (size_t)S.nvx + (gm ? 4 * (size_t)S.nvx : 0) + exd;
}
// spectrum buffer of the chain: the linear layout with one pad double after every 4 ppp samples (the forward convolution's
// lanes are 4 ppp samples apart: the pad makes that stride odd)
__host__ __device__ inline size_t rows_xbuf_doubles(const KStatic& S) {
  const size_t n = xbuf_doubles(S);
  return ((n + n / (4 * (size_t)S.ppp) + 3) & ~(size_t)1);
}
__host__ __device__ inline size_t rows_smem_doubles(const KStatic& S, int gm, bool zh, size_t exd) {   // exd: doubles of the exchange
  const size_t a = rows_sweep_doubles(S, gm, zh, exd), c = rows_xbuf_doubles(S) + ybuf_doubles(S);
  return rows_persist_doubles(S) + (a > c ? a : c);
}

// EX: the base-point exchange between neighbouring lanes of k_spectrum_fused (its header), per round -- here still in its earlier form
// through LDS (one slot per thread and component, kExLdsDoubles in all): the register form (next_lane_f64) was built and measured
// for this kernel too and bought nothing that could be told from the noise of its bench line (bench.py --ppp 5 --batch 1024: four
// VALU instructions more and five LDS instructions fewer per angle, and this sweep waits for its angle constants at the top of every
// iteration anyway), so the kernel stays instruction for instruction what it was; DESIGN.md section 4.1b has the numbers
// FWD (round 3): tsff_forward at several points per pixel -- the same rounds with the forward value alone (point_forward_sd: the bits
// of the loss kernel's spectrum), ONE scratch component, the chain up to the store of ThryE / ThryI.  It replaces k_spectrum MODE 0's
// one 512-thread workgroup per CU for such decks (the reference's default: 5 points per pixel) and inherits the small-batch form (the
// rounds of a lineout on separate workgroups): B = 1024, ppp = 5 0.90 -> see DESIGN 4.1c; B = 16 0.23 ms was SLOWER than loss + gradient.
template <int NI, int GM, bool ZH, bool EX, bool FWD = false>
__global__ __launch_bounds__(kHalf, 2) void k_spectrum_rows(KStatic S, KCall K, int f0, int flags, const uint8_t* __restrict__ gmask,
                                                            double* __restrict__ grad, double* __restrict__ scratch,
                                                            unsigned* __restrict__ tickets) {
  // flags bit 2: interleaved plan (grid 2B: workgroup f B + b evaluates feature f of lineout b and leaves its part of the
  // gradient in K.gpart[f][b][:]); otherwise grid B, feature f0, grad written
  // flags bit 4: SPLIT (small batches: fewer workgroups than CUs) -- grid.y = ppp, workgroup (x, y) sweeps round y only and
  // the one that finishes LAST for its (lineout, feature) x runs the instrument chain and the contraction: the latency of a
  // call drops from ppp rounds + chain to one round + chain.  Hand-off through global memory between workgroups (other CUs,
  // other XCDs) as MI355X_MICROARCH.md prescribes: every storing wavefront waits for its stores, workgroup barrier, one lane's
  // agent-scope release, then an agent-scope atomic ticket; the workgroup whose ticket is the last one does one agent-scope
  // acquire behind a barrier before anybody loads a row.  The same arithmetic in the same order: the same bits.
  const bool interleaved = flags & kFlagInterleaved;
  const int f_il = interleaved ? (int)(blockIdx.x >= (unsigned)K.B) : 0;
  const int b = interleaved ? (int)blockIdx.x - f_il * K.B : (int)blockIdx.x, tid = threadIdx.x;
  constexpr int TPF = kHalf, NW = TPF / 64;
  typedef RowsLayout<NI, GM> RL;
  const int ht = tid, lane = tid & 63, hw = tid >> 6;
  const int f = __builtin_amdgcn_readfirstlane(interleaved ? f_il : f0);
  extern __shared__ __align__(16) unsigned char smem[];
  Smem m;
  {
    double* p = reinterpret_cast<double*>(smem);
    m.taps = p; p += S.ntaps[0] + S.ntaps[1];
    m.phys = p; p += kNP_MAX + 2;
    m.cosa = p; p += S.n_angles;
    m.wsa = p; p += S.n_angles;
    m.red = p; p += 10 * kNP_MAX + 64;
    m.etab = p; p += kNExpTab;
    p += ((reinterpret_cast<size_t>(p) >> 3) & 1);   // (16-byte alignment of the double2 tables)
    double* base = p;
    m.zp = reinterpret_cast<double2*>(p);
    m.ht = m.zp + (ZH ? kNZh : kNXi2);
    m.W = reinterpret_cast<double*>(m.ht + S.nvx);
    p = m.W + kNXi2;
    m.hc = reinterpret_cast<double2*>(p); p += 4 * (size_t)S.nvx;
    m.hcm = nullptr;
    if (GM) { m.hcm = reinterpret_cast<double2*>(p); p += 4 * (size_t)S.nvx; }
    m.Wm = nullptr; m.ksc = nullptr; m.ex = EX ? p : nullptr;
    m.x = base;                       // the chain's buffers overlay the tables (used after the sweep only)
    m.yb = base + rows_xbuf_doubles(S);
  }
  Tables T;
  load_tables(m, S, K, S.shared_fe ? 0 : b, true, T, ZH);
  const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
  stage_phys<NI>(S, xpar, m.phys);
  const double lam_shift = S.lam_shift[f];
  const double* __restrict__ omgs = S.omgs[f];
  const int npts = S.npts, ppp = S.ppp, NA = S.n_angles;
  double* __restrict__ rows = scratch + (size_t)blockIdx.x * (FWD ? 1 : RL::kN) * npts;
  auto RW = [&](int c, int j) -> double* { return rows + (size_t)(FWD ? 0 : c) * npts + j; };   // (FWD: the forward value is the only component)

  // ================= the sweep, ppp rounds of 1024 samples: forward value and Jacobian rows -> scratch =================
  LineS<NI> L;
  {
    Phys<NI> p;
    phys_from_lds<NI>(m.phys, p);
    make_lines_uniform<NI>(p, lam_shift, 0, 1, L);
  }
  __syncthreads();
  const double cw = -0.5 * L.i2wL * L.i2wL;
  const bool split = flags & kFlagSplit;
  const int rd_first = split ? (int)blockIdx.y : 0, rd_last = split ? (int)blockIdx.y + 1 : ppp;
  for (int rd = rd_first; rd < rd_last; ++rd) {
    // thread ht owns the pairs {2 ht, 2 ht + 1} and {512 + 2 ht, 513 + 2 ht} of the round's 1024 samples (k_spectrum_fused)
    const int jp[2] = {rd * TSFF_NBINS + kPair * ht, rd * TSFF_NBINS + TSFF_NBINS / 2 + kPair * ht};
    double ws[2][kPair + 1];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q <= kPair; ++q) ws[p][q] = omgs[min(jp[p] + q, npts - 1)];
    LineS<NI> J[kStrip];
    KsAcc KA[kStrip];
    double xa[kStrip];
#pragma unroll
    for (int q = 0; q < kStrip; ++q) { zero_lines<NI>(J[q]); xa[q] = 0.0; KA[q].p1a = KA[q].p2a = KA[q].p1b = KA[q].p2b = 0.0; }
    auto far_unit = [&](int p) {
      const int jw0 = rd * TSFF_NBINS + (p ? TSFF_NBINS / 2 : 0) + kPair * 64 * hw;
      return far_range<NI>(omgs, jw0, min(jw0 + kPair * 64, npts - 1), L);
    };
    double* exl = m.ex;
    double* exb = EX ? m.ex + kExComp * kHalf : nullptr;
    if (EX) {   // the base points right of this wavefront's two units of the round, all angles at once (lane = 16 P + a)
      __builtin_amdgcn_wave_barrier();   // (the previous round's reads of the boundary slots are done)
      const int Pb = (lane >> 4) & 1, ab = lane & 15;
      if (lane < 32 && ab < NA) {
        const int jend = min(rd * TSFF_NBINS + (Pb ? TSFF_NBINS / 2 : 0) + kPair * 64 * (hw + 1), npts - 1);
        unit_boundary_fill<NI>(omgs[jend], m.cosa[ab], L, T, exb + 16 * (2 * hw + Pb) + ab);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    auto sweep = [&](auto pair_tag, auto far_tag) {
      constexpr int P = decltype(pair_tag)::value;
      constexpr bool FAR = decltype(far_tag)::value;
      const int jb = jp[P];
      const double ks0 = ks_eval(ws[P][0], L.wpe2), ks1 = ks_eval(ws[P][1], L.wpe2), ks2 = ks_eval(ws[P][2], L.wpe2);
      for (int a = 0; a < NA; ++a) {
        const double ct = uni(m.cosa[a]), wa = uni(m.wsa[a] * L.pref);
        Base b0;
        base_eval<NI>(ws[P][0], ks0, ct, L, T, b0);
        if (EX) {
          exl[ht] = b0.wd; exl[kHalf + ht] = b0.ik; exl[2 * kHalf + ht] = b0.xe; exl[3 * kHalf + ht] = b0.F; exl[4 * kHalf + ht] = b0.dH;
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int i = 0; i < kPair; ++i) {
          constexpr int q0 = kPair * P;
          const int q = q0 + i, j = jb + i;
          // (The lookups keep their selects here: load_tables writes no out-of-grid cell.  With hermite_lookup_c<true> the forward
          //  form <1, 0, false, true, true> went from 123 to 129 VGPRs, four to three wavefronts per SIMD, and <1, 0, false, false,
          //  false> from 2 to 4 spilled registers; profiles/r10_selects_isa.txt.)
          const bool has_next = pair_has_next<NI, P, 2>(i, j, npts);
          Base b1;
          if (EX && i == kPair - 1) {   // the neighbour lane's first base point (or the unit's boundary point for the last lane)
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const double* src = lane == 63 ? exb + 16 * (2 * hw + P) + a : exl + ht + 1;
            const int cs = lane == 63 ? kExBound : kHalf;
            b1.wd = src[0]; b1.ik = src[cs]; b1.xe = src[2 * cs]; b1.F = src[3 * cs]; b1.dH = src[4 * cs];
            b1.ks = ks2;
            b1.k2 = base_k2<NI>(ks2, ct, L);
            __builtin_amdgcn_wave_barrier();   // (the next angle's stores stay behind these loads)
          } else
          base_eval<NI>(ws[P][i + 1], i == 0 ? ks1 : ks2, ct, L, T, b1);
          if constexpr (FWD) {
            xa[q] = __builtin_fma(wa, point_forward_sd<NI, ZH, FAR>(b0, b1, has_next, L, T), xa[q]);
          } else {
            row_step<NI, GM, ZH, FAR>(b0, b1, has_next, L, T, ct, wa, cw, xa[q], J[q], KA[q]);
          }
          b0 = b1;
        }
      }
    };
    if (far_unit(0)) sweep(std::integral_constant<int, 0>{}, std::true_type{}); else sweep(std::integral_constant<int, 0>{}, std::false_type{});
    if (far_unit(1)) sweep(std::integral_constant<int, 1>{}, std::true_type{}); else sweep(std::integral_constant<int, 1>{}, std::false_type{});
    if constexpr (!FWD) {
#pragma unroll
      for (int q = 0; q < kStrip; ++q)   // the k_L and omega_pe^2 columns of the rows from their angle sums (KsAcc, k_pairs.inc)
        ks_columns<NI>(KA[q], ks_eval(ws[q >> 1][q & 1], L.wpe2), ks_eval(ws[q >> 1][(q & 1) + 1], L.wpe2), L, J[q]);
    }
    // rows of the round -> scratch: per component the pair's two consecutive samples as one 16-byte store
#pragma unroll
    for (int P = 0; P < 2; ++P) {
      const int j = jp[P];
      auto put = [&](int c, double v0, double v1) { *reinterpret_cast<double2*>(RW(c, j)) = make_double2(v0, v1); };
      if constexpr (!FWD) {
        const LineS<NI>& A = J[2 * P];
        const LineS<NI>& Bq = J[2 * P + 1];
        put(0, A.wpe2, Bq.wpe2); put(1, A.wL, Bq.wL); put(2, A.kL, Bq.kL); put(3, A.ivTe, Bq.ivTe); put(4, A.a_e, Bq.a_e);
        put(5, A.Ud, Bq.Ud); put(6, A.Vd, Bq.Vd);
#pragma unroll
        for (int s = 0; s < NI; ++s) { put(7 + 3 * s, A.ixi[s], Bq.ixi[s]); put(8 + 3 * s, A.a_i[s], Bq.a_i[s]); put(9 + 3 * s, A.cs[s], Bq.cs[s]); }
        if (GM == 1) put(7 + 3 * NI, A.m, Bq.m);
      }
      put(RL::kX, xa[2 * P], xa[2 * P + 1]);
    }
  }
  if (split) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wavefront's row stores have left the CU
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned t = __hip_atomic_fetch_add(tickets + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      m.red[0] = (double)t;
    }
    __syncthreads();
    const bool last = (unsigned)m.red[0] == (unsigned)(ppp - 1);
    if (!last) return;
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(tickets + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
    }
  }
  __syncthreads();   // the tables are dead, every row is written: the chain's buffers take the tables' place

  // ================= IRF convolution ("same") + bin average (taps folded by the host), normalisation: as k_spectrum, linear layout =================
  constexpr int BPT = TSFF_NBINS / TPF;
  const int H = S.halo, Hb = S.halo_bins;
  double* xs = m.x;
  double* ybs = m.yb;
  for (int i = ht; i < (int)rows_xbuf_doubles(S); i += TPF) xs[i] = 0.0;
  for (int i = ht; i < (int)ybuf_doubles(S); i += TPF) ybs[i] = 0.0;
  __syncthreads();
  // adj4: the forward convolution's fast form (below) -- a thread owns four ADJACENT bins and x sits in the padded layout v + v / (4 ppp)
  const bool adj4 = ppp >= 2 && ppp <= 5;
  const unsigned qmagic = adj4 ? (unsigned)((0x100000000ull + 4 * ppp - 1) / (4 * ppp)) : 0u;   // v / (4 ppp) = umulhi(v, qmagic), v < 2^32 / (4 ppp)
  {
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
    for (int i = ht; i < npts; i += TPF) {   // the factor ws^2 (left out of the sweep) and the notch filter of the electron feature
      const double w = omgs[i];
      const unsigned v = (unsigned)(H + i);
      xs[v + __umulhi(v, qmagic)] = *RW(RL::kX, i) * (filt ? w * w * S.filt[i] : w * w);
    }
  }
  __syncthreads();
  const int nh = S.ntaps[f], toff = S.toff[f];
  // (constant address space: the taps are read-only for the whole launch and their index is wavefront-uniform, so the reads
  //  below are scalar loads -- no LDS traffic, no vector-memory instructions)
  cdouble_t* taps = (cdouble_t*)S.taps[f];
  auto PB = [&](int r) { return adj4 ? BPT * ht + r : ht + TPF * r; };   // r-th bin of this thread
  double ybin[BPT];
#pragma unroll
  for (int r = 0; r < BPT; ++r) ybin[r] = 0.0;
  // Fast form: the thread's bins 4 ht .. 4 ht + 3 read overlapping windows of x, ppp samples apart -- ONE LDS read of x[v] serves
  // all four with the taps s', s' - ppp, s' - 2 ppp, s' - 3 ppp (scalar loads from the zero-padded copy): 1 LDS read per 4 FMAs where
  // the bin-per-lane form below takes 4 (it was LDS-bound: the two convolutions cost 0.3 of the 1.36 ms at 5 points per pixel).
  // The lanes are 4 ppp samples apart; the pad double after every 4 ppp samples makes their stride odd (no bank conflicts), and since
  // the lane base 4 ppp ht is a multiple of 4 ppp the pad offset (c + s') / (4 ppp) is wavefront-uniform.
  auto fconv = [&](auto ppp_tag) {
    constexpr int PP = decltype(ppp_tag)::value, Q = BPT * PP;
    static_assert(BPT == 4 && 3 * PP <= kTapPad, "four adjacent bins per thread, taps padded by 3 ppp");
    cdouble_t* ptp = (cdouble_t*)(S.ptaps[f] + kTapPad);
    const double* __restrict__ xl = xs + (Q + 1) * ht;
    const int c = H + toff, n = nh + 3 * PP;
#pragma unroll 4
    for (int sp = 0; sp < n; ++sp) {
      const int w = c + sp;
      const double xv = xl[w + w / Q];
      ybin[0] = __builtin_fma(ptp[sp], xv, ybin[0]);
      ybin[1] = __builtin_fma(ptp[sp - PP], xv, ybin[1]);
      ybin[2] = __builtin_fma(ptp[sp - 2 * PP], xv, ybin[2]);
      ybin[3] = __builtin_fma(ptp[sp - 3 * PP], xv, ybin[3]);
    }
  };
  switch (adj4 ? ppp : 0) {
    case 2: fconv(std::integral_constant<int, 2>{}); break;
    case 3: fconv(std::integral_constant<int, 3>{}); break;
    case 4: fconv(std::integral_constant<int, 4>{}); break;
    case 5: fconv(std::integral_constant<int, 5>{}); break;
    default: break;
  }
  if (!adj4) {
    const double* __restrict__ x0 = xs + H + toff + ht * ppp;
    const int rs = TPF * ppp;
#pragma unroll 4
    for (int t = 0; t < nh; ++t) {  // one tap feeds all the thread's bins
      const double g = taps[t];
#pragma unroll
      for (int r = 0; r < BPT; ++r) ybin[r] += g * x0[r * rs + t];
    }
  }
  double M = ybin[0];
  int pstar = PB(0);
#pragma unroll
  for (int r = 1; r < BPT; ++r)
    if (ybin[r] > M) { M = ybin[r]; pstar = PB(r); }
  half_argmax<NW>(M, pstar, m.red, 0, hw, lane);
  const double invM = 1.0 / M;
  const double amps = K.amps[f][b];
  const double p_lam = uni(m.phys[TSFF_P_LAM]), p_amp1 = uni(m.phys[TSFF_P_AMP1]), p_amp2 = uni(m.phys[TSFF_P_AMP2]),
               p_amp3 = uni(m.phys[TSFF_P_AMP3]);
  const double* __restrict__ lamb = S.lam_bin[f];
  if constexpr (FWD) {   // tsff_forward: amplitudes, noise, store -- done
#pragma unroll
    for (int r = 0; r < BPT; ++r) {
      const int pb = PB(r);
      const double A = bin_amplitude(f, false, amps, f == TSFF_FEATURE_ELE ? lamb[pb] : 0.0, p_lam, p_amp1, p_amp2, p_amp3);
      K.thry[f][(size_t)b * TSFF_NBINS + pb] = thry_value(A, ybin[r], invM, K.noise[f] != nullptr,
                                                          K.noise[f] ? K.noise[f][(size_t)b * TSFF_NBINS + pb] : 0.0);   // thomson_diagnostic.py:139-140
    }
    return;
  }
  double Tb[BPT], Ap[BPT];
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    const double A = bin_amplitude(f, false, amps, f == TSFF_FEATURE_ELE ? lamb[pb] : 0.0, p_lam, p_amp1, p_amp2, p_amp3);
    Ap[r] = A;
    const double t = thry_value(A, ybin[r], invM, K.noise[f] != nullptr,
                                K.noise[f] ? K.noise[f][(size_t)b * TSFF_NBINS + pb] : 0.0);   // thomson_diagnostic.py:139-140
    if (K.thry[f]) K.thry[f][(size_t)b * TSFF_NBINS + pb] = t;
    Tb[r] = bin_loss(S, K, f, K.data[f][(size_t)b * TSFF_NBINS + pb], t, S.mask[f][pb], s0, s1);
  }

  // ================= adjoint of normalisation + binning: T_p = A_p ybin_p / M (+ noise), M attained at pstar =================
  double sn = 0.0, a1b = 0.0, a2b = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    norm_adjoint_bin(f, Tb[r], ybin[r], invM, Ap[r], amps, f == TSFF_FEATURE_ELE ? lamb[pb] : 0.0, p_lam, sn, a1b, a2b);
  }
  {   // the two loss sums and the three sums of the normalisation's adjoint in one reduction (half_sums)
    double v5[5] = {s0, s1, sn, a1b, a2b};
    half_sums<NW, 5>(v5, m.red, 0, hw, lane);
    s0 = v5[0]; s1 = v5[1]; sn = v5[2]; a1b = v5[3]; a2b = v5[4];
  }
  if (ht == 0) {
    if (f == TSFF_FEATURE_ELE) { K.lpart[(size_t)b * 3 + 1] = s0; K.lpart[(size_t)b * 3 + 2] = s1; }
    else K.lpart[(size_t)b * 3 + 0] = s0;
  }
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    double yb = Tb[r] * Ap[r] * invM;
    if (pb == pstar) yb -= sn * invM;
    ybs[Hb + pb] = yb;
  }
  __syncthreads();

  // ===== adjoint of convolution + binning: xbar_i = ws_i^2 filt_i sum_p ybar_p hb[i - p ppp - toff] =====
  // The ppp samples i = ppp u + r of bin u meet the same ybar_p, p = u - d, with ppp CONSECUTIVE taps hb[ppp d + r - toff]: one LDS
  // read of ybar feeds ppp FMAs whose taps are scalar loads (the per-sample form walks the taps with stride ppp and reads ybar
  // once per FMA -- and with range checks around scalar tap loads it compiled to ~100 k instructions per wavefront at 5 points per
  // pixel: the taps are zero-padded by kTapPad on both sides instead).  xbar goes to the LDS of x (dead now).
  {
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
    // tap index of (d, r): ppp d + r - toff in [0, nh); d from dlo = ceil((toff - (ppp - 1)) / ppp) to dhi = floor((nh - 1 + toff) / ppp)
    auto bins = [&](auto ppp_tag) {
      constexpr int PP = decltype(ppp_tag)::value;
      const int dlo = -((-toff + PP - 1) / PP), dhi = (nh - 1 + toff) / PP;   // (toff <= 0 < nh + toff) every d in [dlo, dhi] has a valid r
      cdouble_t* ptp = (cdouble_t*)(S.ptaps[f] + kTapPad);
#pragma unroll 1
      for (int r4 = 0; r4 < BPT; ++r4) {
        const int u = ht + TPF * r4;   // (bin-per-lane mapping whatever the forward convolution used: conflict-free reads of ybar)
        double acc[PP];
#pragma unroll
        for (int r = 0; r < PP; ++r) acc[r] = 0.0;
#pragma unroll 2
        for (int d = dlo; d <= dhi; ++d) {
          const double yv = ybs[Hb + u - d];
          const int t0 = PP * d - toff;
#pragma unroll
          for (int r = 0; r < PP; ++r) {
            acc[r] = __builtin_fma(yv, ptp[t0 + r], acc[r]);   // (zero-padded taps: no range checks)
          }
        }
#pragma unroll
        for (int r = 0; r < PP; ++r) {
          const int i = PP * u + r;
          const double w = omgs[i];
          xs[H + i] = acc[r] * (filt ? w * w * S.filt[i] : w * w);
        }
      }
    };
    __syncthreads();   // (every thread has read its x window in the forward convolution; half_sum's barriers lie in between anyway)
    switch (ppp) {
      case 2: bins(std::integral_constant<int, 2>{}); break;
      case 3: bins(std::integral_constant<int, 3>{}); break;
      case 4: bins(std::integral_constant<int, 4>{}); break;
      case 5: bins(std::integral_constant<int, 5>{}); break;
      default:
        for (int i = ht; i < npts; i += TPF) {
          const int q = i - toff;           // >= 0: toff = -dmax <= 0
          int pb = q / ppp;
          double sv = 0.0;
          for (int t = q - pb * ppp; t < nh; t += ppp, --pb) sv += taps[t] * ybs[Hb + pb];
          const double w = omgs[i];
          xs[H + i] = sv * (filt ? w * w * S.filt[i] : w * w);
        }
    }
  }
  __syncthreads();
  // ===== contraction with the rows: grad_k = sum_i xbar_i J[i][k] (row i from the scratch, consecutive i on consecutive lanes) =====
  constexpr int NPk = TSFF_NP(NI);
  constexpr int NLB = 9 + 3 * NI;
  double lb[NLB];
#pragma unroll
  for (int k = 0; k < NLB; ++k) lb[k] = 0.0;
  for (int i = ht; i < npts; i += TPF) {
    const double xb = xs[H + i];
    // lb: wpe2, wL, kL, ivTe, a_e, pref, Ud, Vd | ixi, a_i, cs per species | m   (the order of k_spectrum's reduction)
    lb[0] += xb * *RW(0, i); lb[1] += xb * *RW(1, i); lb[2] += xb * *RW(2, i); lb[3] += xb * *RW(3, i); lb[4] += xb * *RW(4, i);
    lb[5] += xb * *RW(RL::kX, i);     // d x_j / d pref = x_j / pref (the factor 1/pref below)
    lb[6] += xb * *RW(5, i); lb[7] += xb * *RW(6, i);
#pragma unroll
    for (int s = 0; s < NI; ++s) {
      lb[8 + 3 * s] += xb * *RW(7 + 3 * s, i); lb[9 + 3 * s] += xb * *RW(8 + 3 * s, i); lb[10 + 3 * s] += xb * *RW(9 + 3 * s, i);
    }
    if (GM == 1) lb[NLB - 1] += xb * *RW(7 + 3 * NI, i);
  }
  lb[5] *= 1.0 / L.pref;
#pragma unroll
  for (int s = 0; s < NI; ++s) lb[9 + 3 * s] *= -0.5;   // deferred factor of point_fused
  // (what the last stage needs from global memory is requested here, ahead of the reductions: the tail is a chain of latencies)
  const bool fin = tid < NPk;
  const double fin_x = fin ? xpar[tid] : 0.0, fin_scale = fin ? S.p_scale[tid] : 0.0;
  const bool fin_sig = fin && S.p_sig[tid], fin_mask = fin && gmask[tid];
  double* gsum = m.red + 8 * kNP_MAX;
  if (ht < NPk) gsum[ht] = 0.0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NLB; ++k) {
    const double v = wave_sum(lb[k]);
    if (lane == 0) m.red[hw * NLB + k] = v;
  }
  __syncthreads();
  if (ht == 0) {
    const double* r = m.red;
#pragma unroll
    for (int k = 0; k < NLB; ++k) lb[k] = (r[k] + r[NLB + k]) + (r[2 * NLB + k] + r[3 * NLB + k]);
    LineS<NI> LB;
    zero_lines<NI>(LB);
    lines_adj_load<NI>(lb, true, LB);
    Phys<NI> p;
    phys_from_lds<NI>(m.phys, p);
    double g[NPk];   // (registers: the LDS read-modify-writes this section used to make were a serial chain of round trips)
#pragma unroll
    for (int s = 0; s < NPk; ++s) g[s] = 0.0;
    make_lines_adjoint<NI>(p, lam_shift, 0, 1, L, LB, g);
    amp_adjoint(f, a1b, a2b, g);
    tie_renorm_adjoint<NI>(S, p, GM == 1, g);
#pragma unroll
    for (int s = 0; s < NPk; ++s) gsum[s] = g[s];
  }
  __syncthreads();
  if (tid < NPk) {
    const double v = activation_adjoint(gsum[tid], fin_scale, fin_sig, [&] { return sigmoid(fin_x); }, fin_mask);
    if (interleaved) K.gpart[((size_t)f * K.B + b) * NPk + tid] = v;  // summed over the two features by k_loss_reduce
    else grad[(size_t)b * NPk + tid] = v;
  }
}
