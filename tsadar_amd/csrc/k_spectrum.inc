// k_spectrum.inc -- k_spectrum: forward model + loss + hand-written adjoint of one (lineout, feature) per workgroup; k_loss_reduce.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).

// ------------------------------------------------------------------------------------------
// shared helpers of the spectrum kernels
// ------------------------------------------------------------------------------------------
constexpr int kHalf = 256;  // threads per feature when a k_spectrum workgroup evaluates both features (TPF)
#ifndef TSFF_QUNROLL
#define TSFF_QUNROLL 0  // unroll factor of the strip loop (points interleaved per thread); 0: chosen per instantiation
#endif
#define TSFF_PRAGMA(x) _Pragma(#x)
#define TSFF_UNROLL(n) TSFF_PRAGMA(unroll n)
#ifndef TSFF_OCC
#define TSFF_OCC 2  // wavefronts per SIMD the register allocator must leave room for (one 512-thread workgroup per CU)
#endif

struct Smem {
  double2* zp;    // [kNZh] Z' for xi >= 0, or the full [1640] table (see ion_terms)
  double2* ht;    // [nvx]
  double* W;      // [1640]
  double* x;      // [nfeat][halo + npts + halo]   model spectrum of each feature, later its adjoint
  double* yb;     // [nfeat][halo_bins + 1024 + halo_bins]   adjoint of the binned spectrum (MODE 1)
  double* taps;   // [ntaps[0] + ntaps[1]] bin-averaged IRF taps of both features
  double2* hc;    // [2*(nvx-1)] Hermite coefficients per interval
  double2* hcm;   // the same for d ln fe / dm
  double* Wm;     // [1640] dW/dm
  double* ksc;    // [nfeat][npts + 1] k_s cache of the current gradient point
  double* phys;   // [kNP_MAX + 1] physical parameters of this lineout
  double* cosa;   // [n_angles]
  double* wsa;    // [n_angles]
  double* red;    // [8 * kNP_MAX + 64]
  double* etab;   // [kNExpTab] 2^(j/64) (fexp_t)
  double* ex;     // [kExDoubles] unit-boundary points of the base-point exchange (k_spectrum_fused), or nullptr
};

// one spectrum / per-bin adjoint buffer: linear with a zero halo, or four phase arrays (sample j -> phase j & 3, slot
// j >> 2) with a halo of hs slots each -- sized for the larger of the two layouts
__host__ __device__ inline size_t xbuf_doubles(const KStatic& S) {
  const size_t lin = (size_t)S.npts + 2 * (size_t)S.halo, ph = (size_t)S.npts + 8 * (size_t)S.hs;
  return (lin > ph ? lin : ph) + 2;
}
__host__ __device__ inline size_t ybuf_doubles(const KStatic& S) {
  const size_t lin = (size_t)TSFF_NBINS + 2 * (size_t)S.halo_bins, ph = (size_t)TSFF_NBINS + 8 * (size_t)S.hs;
  return (lin > ph ? lin : ph) + 2;
}

// LDS budget (in doubles) of one k_spectrum / k_form_factor workgroup holding `nfeat` features;
// with_m: tangent tables of the DLM order; with_ks: k_s cache
// gm (the kernel's GM): 0 no extra tables; 1 tangent tables of the DLM order -- the Hermite coefficients of d ln fe / dm in
// LDS, dW/dm read from global memory (one lookup per point of the reverse sweep only; keeping its 13 KB out of LDS is what
// lets two one-feature workgroups share a CU); 2 the table ADJOINTS (LDS atomics: both regions in LDS)
// alias: the per-bin adjoint buffer shares the memory of the spectrum buffer (phase layout only, see alias_xy)
__host__ __device__ inline bool alias_xy(const KStatic& S, int tpf) { return tpf == 256 && S.ppp == 1; }
// base-point exchange of k_spectrum_fused (EX): per component (w - k V, 1/k, xi_e, F, dH/dxi) 8 units x 16 angles of unit-boundary
// base points; the exchange between lanes itself runs in registers (next_lane_f64).
// kExLdsDoubles is the footprint of the earlier form, which k_spectrum_rows keeps (its header): one LDS slot per thread and component
// in front of the boundary points, 10 KB more.  It is also what the launch planner still CHARGES the register form when it decides
// on EX, the half Z' table and the k_s cache: the decisions, and with them the instantiation every shape runs (the coverage contract
// of the instantiations pins decks to kernels at those thresholds), are what they were; the allocation is the real size.
constexpr int kExComp = 5, kExBound = 8 * 16;
constexpr int kExDoubles = kExComp * kExBound;
constexpr int kExLdsDoubles = kExComp * (kHalf + kExBound);
__host__ __device__ inline size_t smem_doubles(const KStatic& S, int nfeat, int gm, bool with_ks, bool alias = false, bool zh = true,
                                               size_t exd = 0) {   // exd: doubles of the base-point exchange (0: none)
  size_t n = 2 * (size_t)((zh ? kNZh : kNXi2) + S.nvx) + kNXi2 + 4 * (size_t)S.nvx;     // zp, ht, W, hc
  if (gm) n += 4 * (size_t)S.nvx;                                                           // hcm
  if (gm == 2) n += kNXi2;                                                                  // Wm
  n += (size_t)nfeat * xbuf_doubles(S);                                                     // spectrum buffers
  if (!alias) n += (size_t)nfeat * ybuf_doubles(S);                                         // per-bin adjoint buffers
  if (with_ks) n += (size_t)nfeat * ((size_t)S.npts + 2);                                   // k_s cache
  n += S.ntaps[0] + S.ntaps[1] + 16 + 2 * (size_t)S.n_angles + 11 * kNP_MAX + 66 + kNExpTab;     // taps (+ padding of one feature's padded copy), angles, phys, scratch, exp table
  n += exd;
  return n;
}

__device__ __forceinline__ Smem carve(unsigned char* smem, const KStatic& S, int nfeat, int gm, bool with_ks, bool alias = false,
                                   bool zh = true, bool ex = false) {
  Smem m;
  m.zp = reinterpret_cast<double2*>(smem);
  m.ht = m.zp + (zh ? kNZh : kNXi2);
  m.W = reinterpret_cast<double*>(m.ht + S.nvx);
  double* p = m.W + kNXi2;
  // one buffer per feature holds the model spectrum x and later its adjoint, another the adjoint of the binned
  // spectrum; zero halos on both sides so the convolutions need no bounds checks
  m.x = p; p += (size_t)nfeat * xbuf_doubles(S);
  if (alias) m.yb = m.x; else { m.yb = p; p += (size_t)nfeat * ybuf_doubles(S); }
  m.hc = reinterpret_cast<double2*>(p); p += 4 * (size_t)S.nvx;   // (nvx cells: nvx - 1 intervals + one more, the out-of-grid cell that stage_commit(pad) fills)
  m.hcm = nullptr; m.Wm = nullptr;
  if (gm) { m.hcm = reinterpret_cast<double2*>(p); p += 4 * (size_t)S.nvx; }
  if (gm == 2) { m.Wm = p; p += kNXi2; }
  m.ksc = nullptr;
  if (with_ks) { m.ksc = p; p += (size_t)nfeat * (S.npts + 2); }
  m.taps = p; p += S.ntaps[0] + S.ntaps[1] + 16;
  m.phys = p; p += kNP_MAX + 2;
  m.cosa = p; p += S.n_angles;
  m.wsa = p; p += S.n_angles;
  m.red = p; p += 10 * kNP_MAX + 64;   // (scratch: reductions, then the per-feature physical-parameter adjoints at 8 kNP_MAX)
  m.etab = p; p += kNExpTab;
  m.ex = ex ? p : nullptr;
  return m;
}

// parts: bit 0 the static tables (Z', IRF taps, angles, exp table), bit 1 the tables of distribution-function slot `slot`
// (W, ln f_e and its Hermite coefficients, the tangent tables of the DLM order) -- a persistent workgroup stages the first once
// and, unless every lineout shares one f_e, the second per lineout
__device__ __forceinline__ void load_tables(const Smem& m, const KStatic& S, const KCall& K, int slot, bool with_taps,
                                            Tables& T, bool zh = true, int parts = 3) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  if (parts & 1) {
    if (zh) { for (int i = tid; i < kNZh; i += nthr) m.zp[i] = S.zp[i]; }
    else { for (int i = tid; i < kNXi2; i += nthr) m.zp[i] = S.zpf[i]; }
    if (with_taps) {
      for (int i = tid; i < S.ntaps[0]; i += nthr) m.taps[i] = S.taps[0][i];
      for (int i = tid; i < S.ntaps[1]; i += nthr) m.taps[S.ntaps[0] + i] = S.taps[1][i];
    }
    for (int i = tid; i < S.n_angles; i += nthr) { m.cosa[i] = S.cos_sa[i]; m.wsa[i] = S.w_sa[i]; }
    for (int i = tid; i < kNExpTab; i += nthr) m.etab[i] = S.etab[i];
  }
  if (parts & 2) {
    for (int i = tid; i < kNXi2; i += nthr) m.W[i] = K.W[(size_t)slot * kNXi2 + i];
    for (int i = tid; i < S.nvx; i += nthr) m.ht[i] = K.ht[(size_t)slot * S.nvx + i];
    for (int i = tid; i < S.nvx - 1; i += nthr) {
      double2 c01, c23;
      hermite_coeffs(K.ht[(size_t)slot * S.nvx + i], K.ht[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
      m.hc[2 * i] = c01;
      m.hc[2 * i + 1] = c23;
    }
    if (m.hcm && K.htm) {  // tangent tables of the DLM order
      for (int i = tid; i < S.nvx - 1; i += nthr) {
        double2 c01, c23;
        hermite_coeffs(K.htm[(size_t)slot * S.nvx + i], K.htm[(size_t)slot * S.nvx + i + 1], S.dv, c01, c23);
        m.hcm[2 * i] = c01;
        m.hcm[2 * i + 1] = c23;
      }
      if (m.Wm)
        for (int i = tid; i < kNXi2; i += nthr) m.Wm[i] = K.Wm[(size_t)slot * kNXi2 + i];
    }
  }
  T.zp = m.zp; T.W = m.W; T.ht = m.ht; T.hc = m.hc; T.hcm = m.hcm; T.nvx = S.nvx;
  T.Wm = m.Wm ? m.Wm : (K.Wm ? K.Wm + (size_t)slot * kNXi2 : nullptr);   // (LDS copy, or the global table itself)
  T.Wb = nullptr; T.Hy = nullptr; T.Hs = nullptr; T.etab = m.etab;
  tables_set_grid(T, S.vx0, S.dv, S.nvx);
}

// The tables of the one-sweep kernel, staged with ONE round trip to memory: every 16-byte piece of the Z' table and of W, the exp
// table, the feature's IRF taps and the two ln f_e nodes each Hermite interval needs are requested back to back (stage_issue: up to
// kStageK + 8 loads in flight per thread) and written to LDS behind a single wait (stage_commit) -- the caller does the lineout's
// scalar work (parameter transform, lineout scalars) in between, under the loads' latency.  (load_tables walks the tables one after
// the other: eight loops, each a load -> wait -> store round trip of 1-2 us under load; the prologue took 7-9 us of a 60-70 us
// workgroup.)  Not staged: the LDS copy of ln f_e itself, which the one-sweep kernel does not read.  No barrier inside.
// entries of the zero-padded tap array the phase-layout convolutions touch (forward: ascending from cf_i0; adjoint: descending from ca_i0)
__host__ __device__ inline int padded_taps(const KStatic& S, int f) {
  const int a = S.cf_i0[f] + 4 * S.cf_na[f] + 8, b = S.ca_i0[f] + 1;   // (+ 8: conv4_phase requests two groups beyond its last one; <= ntaps + 14)
  return a > b ? a : b;
}
constexpr int kStageK = 10;   // 10 x 256 threads x 16 B = 40 KB >= the full Z' table (26 KB) + W (13 KB)
// (the staged values are separate locals of the caller -- TSFF_STAGE_LOCALS -- handed over by reference: as an array or as one
//  struct they stayed in scratch memory)
#define TSFF_STAGE_LOCALS double2 sv0, sv1, sv2, sv3, sv4, sv5, sv6, sv7, sv8, sv9, sha, shb, sma, smb; double sac, saw, set_, stp
#define TSFF_STAGE_ARGS sv0, sv1, sv2, sv3, sv4, sv5, sv6, sv7, sv8, sv9, sha, shb, sma, smb, sac, saw, set_, stp
struct StageRefs {
  double2 &v0, &v1, &v2, &v3, &v4, &v5, &v6, &v7, &v8, &v9, &ha, &hb, &ma, &mb;
  double &ang_c, &ang_w, &et, &tp;
};
#define TSFF_STAGE_PARAMS double2 &v0, double2 &v1, double2 &v2, double2 &v3, double2 &v4, double2 &v5, double2 &v6, double2 &v7, double2 &v8, \
                          double2 &v9, double2 &ha, double2 &hb, double2 &ma, double2 &mb, double &ang_c, double &ang_w, double &et, double &tp
__device__ __forceinline__ void stage_issue(TSFF_STAGE_PARAMS, const Smem& m, const KStatic& S, const KCall& K, int slot, bool zh, int f) {
  const StageRefs r{v0, v1, v2, v3, v4, v5, v6, v7, v8, v9, ha, hb, ma, mb, ang_c, ang_w, et, tp};
  const int tid = threadIdx.x, nthr = blockDim.x;
  const double2* __restrict__ s0 = zh ? S.zp : S.zpf;
  const int n0 = zh ? kNZh : kNXi2;
  const double2* __restrict__ s1 = reinterpret_cast<const double2*>(K.W + (size_t)slot * kNXi2);   // (16-byte aligned: 1640 doubles per slot)
  const int total = n0 + kNXi2 / 2;
#define TSFF_STAGE_LD(k) { const int c = (k) * nthr + tid; r.v##k = c < n0 ? s0[c] : s1[min(c, total - 1) - n0]; }
  TSFF_STAGE_LD(0) TSFF_STAGE_LD(1) TSFF_STAGE_LD(2) TSFF_STAGE_LD(3) TSFF_STAGE_LD(4)
  TSFF_STAGE_LD(5) TSFF_STAGE_LD(6) TSFF_STAGE_LD(7) TSFF_STAGE_LD(8) TSFF_STAGE_LD(9)
#undef TSFF_STAGE_LD
  static_assert(kStageK == 10, "ten load / store pairs are written out");
  // Hermite intervals: interval i needs nodes i, i + 1 of (ln f_e, slope) -- and of their m-tangents
  const int nvx = S.nvx;
  const bool hint = tid < nvx - 1, hm = hint && m.hcm && K.htm;
  r.ha = r.hb = r.ma = r.mb = make_double2(0.0, 0.0);
  if (hint) { r.ha = K.ht[(size_t)slot * nvx + tid]; r.hb = K.ht[(size_t)slot * nvx + tid + 1]; }
  if (hm) { r.ma = K.htm[(size_t)slot * nvx + tid]; r.mb = K.htm[(size_t)slot * nvx + tid + 1]; }
  r.ang_c = r.ang_w = r.et = r.tp = 0.0;
  if (tid < S.n_angles) { r.ang_c = S.cos_sa[tid]; r.ang_w = S.w_sa[tid]; }
  if (tid < kNExpTab) r.et = S.etab[tid];
  if (tid < padded_taps(S, f)) r.tp = S.ptaps[f][tid];
}
// taps: the feature's zero-padded tap array (S.ptaps[f]: hb[s] at 3 + s, points_per_pixel 1) goes to m.taps[0 .. padded_taps)
// pad: also write the out-of-grid cell of the Hermite coefficient tables (for kernels whose lookups are hermite_lookup_c<true>)
__device__ __forceinline__ void stage_commit(TSFF_STAGE_PARAMS, const Smem& m, const KStatic& S, const KCall& K, int slot, Tables& T,
                                             bool zh, int f, bool pad = false) {
  const StageRefs r{v0, v1, v2, v3, v4, v5, v6, v7, v8, v9, ha, hb, ma, mb, ang_c, ang_w, et, tp};
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int n0 = zh ? kNZh : kNXi2, total = n0 + kNXi2 / 2, nvx = S.nvx;
  double2* d0 = m.zp;
  double2* d1 = reinterpret_cast<double2*>(m.W);
#define TSFF_STAGE_ST(k) { const int c = (k) * nthr + tid; if (c < n0) d0[c] = r.v##k; else if (c < total) d1[c - n0] = r.v##k; }
  TSFF_STAGE_ST(0) TSFF_STAGE_ST(1) TSFF_STAGE_ST(2) TSFF_STAGE_ST(3) TSFF_STAGE_ST(4)
  TSFF_STAGE_ST(5) TSFF_STAGE_ST(6) TSFF_STAGE_ST(7) TSFF_STAGE_ST(8) TSFF_STAGE_ST(9)
#undef TSFF_STAGE_ST
  {   // (only with fewer than 256 threads)
    const double2* __restrict__ s0 = zh ? S.zp : S.zpf;
    const double2* __restrict__ s1 = reinterpret_cast<const double2*>(K.W + (size_t)slot * kNXi2);
    for (int c = kStageK * nthr + tid; c < total; c += nthr) {
      if (c < n0) d0[c] = s0[c]; else d1[c - n0] = s1[c - n0];
    }
  }
  for (int i = tid + nthr; i < nvx - 1; i += nthr) {   // (velocity grids beyond the workgroup size: the plain form)
    double2 c01, c23;
    hermite_coeffs(K.ht[(size_t)slot * nvx + i], K.ht[(size_t)slot * nvx + i + 1], S.dv, c01, c23);
    m.hc[2 * i] = c01; m.hc[2 * i + 1] = c23;
    if (m.hcm && K.htm) {
      hermite_coeffs(K.htm[(size_t)slot * nvx + i], K.htm[(size_t)slot * nvx + i + 1], S.dv, c01, c23);
      m.hcm[2 * i] = c01; m.hcm[2 * i + 1] = c23;
    }
  }
  if (tid < nvx - 1) {
    double2 c01, c23;
    hermite_coeffs(r.ha, r.hb, S.dv, c01, c23);
    m.hc[2 * tid] = c01; m.hc[2 * tid + 1] = c23;
    if (m.hcm && K.htm) {
      hermite_coeffs(r.ma, r.mb, S.dv, c01, c23);
      m.hcm[2 * tid] = c01; m.hcm[2 * tid + 1] = c23;
    }
  }
  if (pad) {   // (cell nvx - 1 of the 2 nvx carved)
    hermite_pad_cell(m.hc, nvx, -50.0, tid);
    if (m.hcm && K.htm) hermite_pad_cell(m.hcm, nvx, 0.0, tid);
  }
  if (m.Wm && K.Wm)
    for (int i = tid; i < kNXi2; i += nthr) m.Wm[i] = K.Wm[(size_t)slot * kNXi2 + i];
  if (tid < S.n_angles) { m.cosa[tid] = r.ang_c; m.wsa[tid] = r.ang_w; }
  if (tid < kNExpTab) m.etab[tid] = r.et;
  const int npad = padded_taps(S, f);
  if (tid < npad) m.taps[tid] = r.tp;
  for (int i = tid + nthr; i < npad; i += nthr) m.taps[i] = S.ptaps[f][i];
  T.zp = m.zp; T.W = m.W; T.ht = m.ht; T.hc = m.hc; T.hcm = m.hcm; T.nvx = S.nvx;
  T.Wm = m.Wm ? m.Wm : (K.Wm ? K.Wm + (size_t)slot * kNXi2 : nullptr);   // (LDS copy, or the global table itself)
  T.Wb = nullptr; T.Hy = nullptr; T.Hs = nullptr; T.etab = m.etab;
  tables_set_grid(T, S.vx0, S.dv, S.nvx);
}

// physical parameters of lineout `xpar` -> LDS (one activation per thread, then Ti tying and fraction
// renormalisation by one thread; ts_params.py:329-350, 543-563).  Contains workgroup barriers.
template <int NI>
__device__ __forceinline__ void stage_phys(const KStatic& S, const double* __restrict__ xpar, double* ph) {
  constexpr int NPk = TSFF_NP(NI);
  const int tid = threadIdx.x;
  if (tid < NPk) {
    const double v = xpar[tid];
    ph[tid] = (S.p_sig[tid] ? sigmoid(v) : v) * S.p_scale[tid] + S.p_shift[tid];
  }
  __syncthreads();
  if (tid == 0) {
    double fsum = 0.0;
#pragma unroll
    for (int s = 0; s < NI; ++s) {
      const int o = TSFF_P_ION0 + 4 * s;
      if (s > 0 && S.ti_same[s]) ph[o + TSFF_ION_TI] = ph[TSFF_P_ION0 + TSFF_ION_TI];
      fsum += ph[o + TSFF_ION_FRACT];
    }
#pragma unroll
    for (int s = 0; s < NI; ++s) ph[TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT] /= fsum;
    ph[NPk] = fsum;
  }
  __syncthreads();
}

// The same staging by ONE wavefront for itself, without workgroup barriers (persistent workgroups: every wavefront of the
// workgroup calls it and writes the identical values -- the result is a pure function of the lineout's parameters, so the
// concurrent stores are idempotent and a wavefront only ever reads what it has written itself).  xv: the normalised leaf of
// slot `lane` (lanes >= NP: anything).  Same operations in the same order as stage_phys: the same bits.
template <int NI>
__device__ __forceinline__ void stage_phys_wave(const KStatic& S, double xv, double* ph, int lane) {
  constexpr int NPk = TSFF_NP(NI);
  const int l = lane < NPk ? lane : 0;
  double v = (S.p_sig[l] ? sigmoid(xv) : xv) * S.p_scale[l] + S.p_shift[l];
  const double ti0 = __shfl(v, TSFF_P_ION0 + TSFF_ION_TI, 64);
  double fsum = 0.0;
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    const int o = TSFF_P_ION0 + 4 * s;
    if (s > 0 && S.ti_same[s] && lane == o + TSFF_ION_TI) v = ti0;
    fsum += __shfl(v, o + TSFF_ION_FRACT, 64);
  }
#pragma unroll
  for (int s = 0; s < NI; ++s)
    if (lane == TSFF_P_ION0 + 4 * s + TSFF_ION_FRACT) v /= fsum;
  if (lane < NPk) ph[lane] = v;
  if (lane == NPk) ph[NPk] = fsum;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// reductions over the NW wavefronts of one feature group; every thread of the WORKGROUP must call them
// (they contain workgroup barriers).  scratch: 32 doubles.
template <int NW>
__device__ __forceinline__ double half_sum(double v, double* scratch, int half, int hw, int lane) {
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) scratch[half * NW + hw] = v;
  __syncthreads();
  const double* r = scratch + half * NW;
  double s = (r[0] + r[1]) + (r[2] + r[3]);
  if (NW == 8) s += (r[4] + r[5]) + (r[6] + r[7]);
  return s;
}

// NV sums at once: the same wavefront butterflies and the same final association per value as NV calls of half_sum, behind ONE pair of
// barriers instead of NV (the chain of the one-sweep kernels is latency-bound: every barrier pair costs about a microsecond).
// scratch: NV * NW doubles.
template <int NW, int NV>
__device__ __forceinline__ void half_sums(double (&v)[NV], double* scratch, int half, int hw, int lane) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) scratch[(half * NV + k) * NW + hw] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const double* r = scratch + (half * NV + k) * NW;
    double s = (r[0] + r[1]) + (r[2] + r[3]);
    if (NW == 8) s += (r[4] + r[5]) + (r[6] + r[7]);
    v[k] = s;
  }
}

template <int NW>
__device__ __forceinline__ void half_argmax(double& v, int& idx, double* scratch, int half, int hw, int lane) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(idx, o, 64);
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
  __syncthreads();
  if (lane == 0) { scratch[half * 2 * NW + hw] = v; scratch[half * 2 * NW + NW + hw] = (double)idx; }
  __syncthreads();
  const double* r = scratch + half * 2 * NW;
  v = r[0]; idx = (int)r[NW];
#pragma unroll
  for (int k = 1; k < NW; ++k) {
    const double ov = r[k]; const int oi = (int)r[NW + k];
    if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
  }
}

// ------------------------------------------------------------------------------------------
// k_spectrum: one workgroup per lineout; threads [0,256) evaluate the first loaded feature, threads
// [256,512) the second (EPW, IAW), sharing the LDS copies of the Z', W and ln f_e tables.  A deck with
// one feature launches 256-thread workgroups.
//   MODE 0: ThryE/ThryI                              (ThomsonScatteringDiagnostic.__call__)
//   MODE 1: + masked loss sums + adjoint -> grad      (LossFunction.vg_loss)
//   MODE 2: + per-lineout sums, theory denominator, sqdev arrays (LossFunction.array_loss)
// ------------------------------------------------------------------------------------------
template <int NI, int MODE, int GM = 0, int TPF = kHalf, bool ZH = true>
__global__ __launch_bounds__(2 * kHalf, TSFF_OCC) void k_spectrum(KStatic S, KCall K, int f0, int nfeat, int flags,
                                                           const uint8_t* __restrict__ gmask, double* __restrict__ grad) {
  // flags bit 0: add to grad instead of overwriting it (second launch of a feature-split call);
  //       bit 1: k_s cache present in LDS;
  //       bit 2: interleaved plan -- grid 2B, workgroup f B + b evaluates feature f of lineout b and leaves its part of
  //              the gradient in K.gpart[f][b][:]; k_loss_reduce adds the two parts
  const bool accumulate = flags & kFlagAccumulate, use_ks = flags & kFlagKsCache, interleaved = flags & kFlagInterleaved;
  // unroll factor of the strip loops: two points in flight help the lean instantiations (-1.6 % plain, -1.9 % with the
  // tangent tables); the heavier ones (table adjoints: 2.0 -> 3.2 ms, more ion species, 512 threads) spill
  constexpr int kQU = (TSFF_QUNROLL > 0) ? TSFF_QUNROLL : ((NI == 1 && GM <= 1 && TPF == kHalf) ? 2 : 1);
  const int f_il = interleaved ? (int)(blockIdx.x >= (unsigned)K.B) : 0;  // first B workgroups: feature 0, next B: feature 1
  const int b = interleaved ? (int)blockIdx.x - f_il * K.B : (int)blockIdx.x, tid = threadIdx.x;
  // TPF threads per feature: 256 when the workgroup holds both features, 512 for a one-feature workgroup
  constexpr int NW = TPF / 64;          // wavefronts per feature
  constexpr int BPT = TSFF_NBINS / TPF;  // output bins per thread
  const int half = tid / TPF, ht = tid % TPF, lane = tid & 63, hw = ht >> 6;
  // feature of this group: wavefront-uniform, kept in an SGPR so that everything indexed by it (tap counts, axis
  // pointers, the padded taps of the convolution) is read through scalar loads
  const int f = __builtin_amdgcn_readfirstlane(interleaved ? f_il : f0 + half);
  extern __shared__ __align__(16) unsigned char smem[];
  const Smem m = carve(smem, S, nfeat, GM, use_ks, alias_xy(S, TPF), ZH);
  Tables T;
  load_tables(m, S, K, S.shared_fe ? 0 : b, true, T, ZH);

  const double* __restrict__ xpar = K.params + (size_t)b * S.NP;
  stage_phys<NI>(S, xpar, m.phys);
  const double lam_shift = S.lam_shift[f];
  const double* __restrict__ omgs = S.omgs[f];
  const int npts = S.npts, ppp = S.ppp, G = S.G, NA = S.n_angles, nstrips = S.npts / kStrip;
  const double invG = 1.0 / (double)G;
  // (pointer arithmetic on the LDS base, not a runtime-indexed pointer array: keeps ds_* addressing)
  // Layout of the spectrum buffer x (and of the per-bin adjoint buffer yb).  Linear: x[H + j] with a zero halo.  Phase
  // layout (points_per_pixel = 1, 256 threads per feature): sample j lives at x[(j & 3) Ls + (j >> 2) + hs], four
  // arrays of Ls = npts/4 + 2 hs slots.  A thread owns the four CONSECUTIVE samples 4 ht .. 4 ht + 3 (its strip of the
  // sweeps, its bins of the convolution), and every access of a wavefront is to 64 consecutive doubles of one phase
  // array (no bank conflicts), which lets the convolution slide a register window over adjacent samples (below).
  const bool ph = (TPF == kHalf) && ppp == 1;
  const int H = S.halo, Hb = S.halo_bins, hs = S.hs, Ls = npts / 4 + 2 * hs;
  // With the phase layout (ph below) the per-bin adjoint ybar lives in the memory of the spectrum x itself: x is dead once
  // the forward convolution has been read into registers, and ybar is dead once the adjoint convolution has -- 8.8 KB of
  // LDS per feature that decide whether two workgroups share a CU for the larger table sets.
  double* xs = m.x + half * xbuf_doubles(S);
  double* ybs = alias_xy(S, TPF) ? xs : m.yb + half * ybuf_doubles(S);
  auto XA = [&](int j) { return ph ? (j & 3) * Ls + (j >> 2) + hs : H + j; };     // sample j of x
  auto YA = [&](int pbin) { return ph ? (pbin & 3) * Ls + (pbin >> 2) + hs : Hb + pbin; };  // bin p of yb
  auto PB = [&](int r) { return ph ? 4 * ht + r : ht + TPF * r; };                // r-th bin of this thread
  for (int i = ht; i < (int)xbuf_doubles(S); i += TPF) xs[i] = 0.0;
  if (!alias_xy(S, TPF))
    for (int i = ht; i < (int)ybuf_doubles(S); i += TPF) ybs[i] = 0.0;
  __syncthreads();

  // ================= forward sweep over (gradient point, lambda strip, angle) =================
  // each thread owns strips of kStrip consecutive samples; the right neighbour's (xi_e, F) needed by the
  // finite difference along lambda (form_factor.py:258) is evaluated by the owner of the strip.
  double* __restrict__ ksc = use_ks ? m.ksc + half * (S.npts + 2) : nullptr;  // k_s(lambda) of the current gradient point
  for (int g = 0; g < G; ++g) {
    LineS<NI> L;
    {
      Phys<NI> p;  // re-read from LDS where needed instead of being kept live across the sweeps
      phys_from_lds<NI>(m.phys, p);
      make_lines_uniform<NI>(p, lam_shift, g, G, L);
    }
    if (use_ks) {
      if (g > 0) __syncthreads();
      for (int i = ht; i < npts; i += TPF) ksc[i] = ks_eval(omgs[i], L.wpe2);  // angle independent (form_factor.py:218)
      __syncthreads();
    }
    for (int st = ht; st < nstrips; st += TPF) {
      const int j0 = kStrip * st;
      // the frequency axis is read from global memory (L1/L2): the strip's first two samples once per
      // chunk, the others one iteration ahead of their use so the load latency hides behind a whole point
      const double ws_first = omgs[j0], ws_second = omgs[min(j0 + 1, npts - 1)];
      auto strip = [&](auto far_tag) {
        constexpr bool FAR = decltype(far_tag)::value;
        for (int a = 0; a < NA; ++a) {
          const double ct = uni(m.cosa[a]), wa = uni(m.wsa[a] * invG * L.pref);   // (pref: see point_forward_sd)
          double ws = ws_first, wnext = ws_second;
          Base b0;
          base_eval<NI>(ws, use_ks ? ksc[j0] : ks_eval(ws, L.wpe2), ct, L, T, b0);
#pragma unroll kQU
          for (int q = 0; q < kStrip; ++q) {
            const int j = j0 + q;
            const bool has_next = (j + 1) < npts;
            const double wsn = wnext;
            wnext = omgs[min(j + 2, npts - 1)];
            Base b1;
            base_eval<NI>(wsn, use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(wsn, L.wpe2), ct, L, T, b1);
            xs[XA(j)] = __builtin_fma(wa, point_forward_sd<NI, ZH, FAR>(b0, b1, has_next, L, T), xs[XA(j)]);
            b0 = b1;
            ws = wsn;
          }
        }
      };
      // wavefronts whose 256 samples all lie away from the laser line run the asymptotic form of the ion terms
      // (point_core<FAR>: same bits, ~45 instructions per point less)
      const int jw0 = kStrip * (st - lane);
      if (far_range<NI>(omgs, min(jw0, npts - 1), min(jw0 + kStrip * 64, npts - 1), L)) strip(std::true_type{});
      else strip(std::false_type{});
    }
  }
  {  // the factor ws^2 of every sample (left out of the sweep) and the notch filter of the electron feature
    const bool filt = f == TSFF_FEATURE_ELE && S.filt;
    for (int st = ht; st < nstrips; st += TPF) {
      const int j0 = kStrip * st;
#pragma unroll
      for (int q = 0; q < kStrip; ++q) {
        const double w = omgs[j0 + q];
        xs[XA(j0 + q)] *= filt ? w * w * S.filt[j0 + q] : w * w;
      }
    }
  }
  __syncthreads();

  // ================= IRF convolution ("same"), bin average, normalisation =================
  // the host folds the bin average into the taps: hb[s] = (1/ppp) sum_jj g[jj - s + nt - 1], so that
  // ybin[p] = sum_s hb[s] x[p ppp + toff + s]  (irf.py:72-74 / 114,124 in one pass; zero halo -> no bounds checks)
  const int nh = S.ntaps[f], toff = S.toff[f];
  const double* __restrict__ taps = m.taps + (f == TSFF_FEATURE_ELE ? 0 : S.ntaps[0]);
  double ybin[BPT];
#pragma unroll
  for (int r = 0; r < BPT; ++r) ybin[r] = 0.0;
  if (ph) {
    // y[4 ht + r] = sum_u g(u) x[4 ht + r + u]: the taps are walked in groups of four (u = 4 a + c); a group needs the
    // seven samples V[k] = x[4 (ht + a) + k], of which three carry over from the previous group -- four LDS reads
    // (conflict-free, one per phase array) and four scalar tap loads per sixteen FMAs, against five LDS reads per four
    // FMAs of the linear form: the convolution stops being LDS-bandwidth bound.
    // (constant address space: the padded taps are read-only for the whole launch, so the wavefront-uniform reads
    //  below become scalar loads and cost neither LDS bandwidth nor vector-memory instructions)
    cdouble_t* pt = (cdouble_t*)(S.ptaps[f] + S.cf_i0[f]);
    const double* __restrict__ X0 = xs, * __restrict__ X1 = xs + Ls, * __restrict__ X2 = xs + 2 * Ls, * __restrict__ X3 = xs + 3 * Ls;
    int sl = ht + S.cf_a0[f] + hs;
    double V0 = X0[sl], V1 = X1[sl], V2 = X2[sl];
    const int na = S.cf_na[f];
    for (int a = 0; a < na; ++a, ++sl) {
      const double V3 = X3[sl], V4 = X0[sl + 1], V5 = X1[sl + 1], V6 = X2[sl + 1];
      const double g0 = pt[4 * a], g1 = pt[4 * a + 1], g2 = pt[4 * a + 2], g3 = pt[4 * a + 3];
      // (index % BPT: the branch is dead, but must compile, in the 512-threads-per-feature instantiation)
      conv_taps4(g0, g1, g2, g3, V0, V1, V2, V3, V4, V5, V6, ybin[0], ybin[1 % BPT], ybin[2 % BPT], ybin[3 % BPT]);
      V0 = V4; V1 = V5; V2 = V6;
    }
  } else {
    const double* __restrict__ x0 = xs + H + toff + ht * ppp;
    const int rs = TPF * ppp;
#pragma unroll 4
    for (int t = 0; t < nh; ++t) {  // one tap read feeds all the thread's bins
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
  half_argmax<NW>(M, pstar, m.red, half, hw, lane);
  // raw: no instrument response for this feature (irf.py:82-86: ThryI = modlI when spect_stddev_ion == 0) -- the host
  // passes an identity tap, and the normalisation / amplitude scaling are skipped
  const bool raw = S.raw[f];
  const double invM = raw ? 1.0 : 1.0 / M;
  const double amps = raw ? 1.0 : K.amps[f][b];
  double p_lam, p_amp1, p_amp2, p_amp3;
  {
    p_lam = uni(m.phys[TSFF_P_LAM]); p_amp1 = uni(m.phys[TSFF_P_AMP1]);
    p_amp2 = uni(m.phys[TSFF_P_AMP2]); p_amp3 = uni(m.phys[TSFF_P_AMP3]);
  }
  const double* __restrict__ lamb = S.lam_bin[f];
  double Tb[BPT];  // dLoss/dT (MODE 1)
  double Ap[BPT];  // amplitude factor of bin p
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    const double A = bin_amplitude(f, raw, amps, f == TSFF_FEATURE_ELE ? lamb[pb] : 0.0, p_lam, p_amp1, p_amp2, p_amp3);
    Ap[r] = A;
    const double t = thry_value(A, ybin[r], invM, K.noise[f] != nullptr,
                                K.noise[f] ? K.noise[f][(size_t)b * TSFF_NBINS + pb] : 0.0);   // thomson_diagnostic.py:139-140
    if (K.thry[f]) K.thry[f][(size_t)b * TSFF_NBINS + pb] = t;
    Tb[r] = 0.0;
    if (MODE >= 1) {
      const double d = K.data[f][(size_t)b * TSFF_NBINS + pb];
      const uint8_t mk = S.mask[f][pb];
      if (MODE == 2) {
        double e, det;
        loss_point(S.loss_method, d, t, e, det);
        if (S.loss_method == TSFF_LOSS_L2 || S.loss_method == TSFF_LOSS_L1) e /= t;  // loss_function.py:320-321
        double sq = 0.0;
        if (mk & 1) { s0 += e; sq += e; }
        if (mk & 2) { s1 += e; sq += e; }
        if (K.sqdev[f]) K.sqdev[f][(size_t)b * TSFF_NBINS + pb] = sq;
      } else {
        Tb[r] = bin_loss(S, K, f, d, t, mk, s0, s1);
      }
    }
  }
  if (MODE == 0) return;
  s0 = half_sum<NW>(s0, m.red, half, hw, lane);
  s1 = half_sum<NW>(s1, m.red, half, hw, lane);
  if (ht == 0) {
    if (f == TSFF_FEATURE_ELE) { K.lpart[(size_t)b * 3 + 1] = s0; K.lpart[(size_t)b * 3 + 2] = s1; }
    else K.lpart[(size_t)b * 3 + 0] = s0;
  }
  if (MODE == 2) return;

  // ================= adjoint of normalisation + binning =================
  // T_p = A_p ybin_p / M (+ noise), M = max_p ybin_p attained at pstar
  double sn = 0.0, a1b = 0.0, a2b = 0.0;
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    norm_adjoint_bin(f, Tb[r], ybin[r], invM, Ap[r], amps, f == TSFF_FEATURE_ELE ? lamb[pb] : 0.0, p_lam, sn, a1b, a2b);
  }
  sn = half_sum<NW>(sn, m.red, half, hw, lane);
  a1b = half_sum<NW>(a1b, m.red, half, hw, lane);
  a2b = half_sum<NW>(a2b, m.red, half, hw, lane);
  if (raw) sn = a1b = a2b = 0.0;   // (no maximum, no amplitudes in the raw spectrum)
#pragma unroll
  for (int r = 0; r < BPT; ++r) {
    const int pb = PB(r);
    double yb = Tb[r] * Ap[r] * invM;
    if (pb == pstar) yb -= sn * invM;
    ybs[YA(pb)] = yb;
  }
  __syncthreads();
  // ================= adjoint of convolution + binning: xbar_i = filt_i sum_p ybar_p hb[i - p ppp - toff] =================
  if (ph) {
    // xbar[4 ht + r] = sum_u g'(u) ybar[4 ht + r + u], g'(u) = hb[-toff - u]: the same sliding window, taps read backwards
    cdouble_t* pt = (cdouble_t*)(S.ptaps[f] + S.ca_i0[f]);
    const double* __restrict__ Y0 = ybs, * __restrict__ Y1 = ybs + Ls, * __restrict__ Y2 = ybs + 2 * Ls, * __restrict__ Y3 = ybs + 3 * Ls;
    int sl = ht + S.ca_a0[f] + hs;
    double V0 = Y0[sl], V1 = Y1[sl], V2 = Y2[sl];
    double sx[4] = {0.0, 0.0, 0.0, 0.0};
    const int na = S.ca_na[f];
    for (int a = 0; a < na; ++a, ++sl) {
      const double V3 = Y3[sl], V4 = Y0[sl + 1], V5 = Y1[sl + 1], V6 = Y2[sl + 1];
      const double g0 = pt[-4 * a], g1 = pt[-4 * a - 1], g2 = pt[-4 * a - 2], g3 = pt[-4 * a - 3];
      conv_taps4(g0, g1, g2, g3, V0, V1, V2, V3, V4, V5, V6, sx[0], sx[1], sx[2], sx[3]);
      V0 = V4; V1 = V5; V2 = V6;
    }
    __syncthreads();   // (ybar and x share their memory: every read of ybar before the first write of xbar)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * ht + r;
      double v = sx[r] * (omgs[i] * omgs[i]);   // (the seed of the reverse sweep carries ws^2, see point_reverse)
      if (f == TSFF_FEATURE_ELE && S.filt) v *= S.filt[i];
      xs[XA(i)] = v * invG;
    }
  } else if (ppp == 1) {
    double sx[BPT];
#pragma unroll
    for (int r = 0; r < BPT; ++r) sx[r] = 0.0;
    const double* __restrict__ y0 = ybs + Hb - toff + ht;
#pragma unroll 4
    for (int t = 0; t < nh; ++t) {
      const double g = taps[t];
#pragma unroll
      for (int r = 0; r < BPT; ++r) sx[r] += g * y0[r * TPF - t];
    }
#pragma unroll
    for (int r = 0; r < BPT; ++r) {
      const int i = ht + TPF * r;
      double v = sx[r] * (omgs[i] * omgs[i]);
      if (f == TSFF_FEATURE_ELE && S.filt) v *= S.filt[i];
      xs[H + i] = v * invG;
    }
  } else {
    for (int i = ht; i < npts; i += TPF) {
      const int q = i - toff;           // >= 0: toff = -dmax <= 0
      int pb = q / ppp;
      double sv = 0.0;
      for (int t = q - pb * ppp; t < nh; t += ppp, --pb) sv += taps[t] * ybs[Hb + pb];
      sv *= omgs[i] * omgs[i];
      if (f == TSFF_FEATURE_ELE && S.filt) sv *= S.filt[i];
      xs[H + i] = sv * invG;
    }
  }
  __syncthreads();

  // ================= reverse sweep: recompute each point, accumulate lineout-scalar adjoints =================
  constexpr int NPk = TSFF_NP(NI);
  constexpr int NLB = 9 + 3 * NI;               // adjoint-carrying fields of LineS
  double* gsum = m.red + 8 * kNP_MAX;           // [2][NPk] physical-parameter adjoints of the two features
  if (ht < NPk) gsum[half * NPk + ht] = 0.0;
  const int wv = tid >> 6;
  FeAcc fa;
  fe_acc_init(fa);
  if (GM == 2) {  // table adjoints live where the tangent tables of GM == 1 would (same LDS budget)
    T.Wb = m.Wm; T.Hy = reinterpret_cast<double*>(m.hcm); T.Hs = T.Hy + S.nvx;
    for (int i = tid; i < kNXi2; i += blockDim.x) T.Wb[i] = 0.0;
    for (int i = tid; i < 2 * S.nvx; i += blockDim.x) T.Hy[i] = 0.0;
    __syncthreads();
  }
  for (int g = 0; g < G; ++g) {
    LineS<NI> L, LB;
    {
      Phys<NI> p;
      phys_from_lds<NI>(m.phys, p);
      make_lines_uniform<NI>(p, lam_shift, g, G, L);
    }
    zero_lines<NI>(LB);
    if (use_ks && G > 1) {  // (with one gradient point the cache of the forward sweep is still valid)
      __syncthreads();
      for (int i = ht; i < npts; i += TPF) ksc[i] = ks_eval(omgs[i], L.wpe2);
      __syncthreads();
    }
    for (int st = ht; st < nstrips; st += TPF) {
      const int j0 = kStrip * st;
      const double ws_first = omgs[j0], ws_second = omgs[min(j0 + 1, npts - 1)];
      auto strip = [&](auto far_tag) {
        constexpr bool FAR = decltype(far_tag)::value;
        constexpr int kQUr = (TSFF_QUNROLL > 0) ? TSFF_QUNROLL : ((NI == 1 && GM <= 1 && TPF == kHalf) ? 2 : 1);   // (= kQU)
        for (int a = 0; a < NA; ++a) {
          const double ct = uni(m.cosa[a]), wa = uni(m.wsa[a] * L.pref);
          double ws = ws_first, wnext = ws_second;
          Base b0;
          base_eval<NI>(ws, use_ks ? ksc[j0] : ks_eval(ws, L.wpe2), ct, L, T, b0);
          double cxe = 0.0, cF = 0.0;
#pragma unroll kQUr
          for (int q = 0; q < kStrip; ++q) {
            const int j = j0 + q;
            const bool has_next = (j + 1) < npts;
            const double wsn = wnext;
            wnext = omgs[min(j + 2, npts - 1)];
            Base b1;
            base_eval<NI>(wsn, use_ks ? ksc[min(j + 1, npts - 1)] : ks_eval(wsn, L.wpe2), ct, L, T, b1);
            BaseAdj ba;
            double xen, Fn;
            point_reverse<NI, GM, ZH, FAR>(b0, b1, has_next, L, T, xs[XA(j)] * wa, ba, xen, Fn, LB, fa);
            ba.xe += cxe; ba.F += cF;
            base_reverse<NI, GM>(ct, b0, L, T, ba, LB, fa);
            cxe = xen; cF = Fn;
            b0 = b1;
            ws = wsn;
          }
          if (j0 + kStrip < npts) {  // the strip's right neighbour receives the D-coupling of the last point
            BaseAdj ba;
            ba.k2 = ba.ik = ba.wd = 0.0; ba.xe = cxe; ba.F = cF;
            base_reverse<NI, GM>(ct, b0, L, T, ba, LB, fa);
          }
        }
      };
      const int jw0 = kStrip * (st - lane);   // (asymptotic ion terms for wavefronts away from the laser line, as in the forward sweep)
      if (far_range<NI>(omgs, min(jw0, npts - 1), min(jw0 + kStrip * 64, npts - 1), L)) strip(std::true_type{});
      else strip(std::false_type{});
    }
    // ---- reduce the lineout-scalar adjoints over the feature's 4 wavefronts; one thread per feature
    //      chains them to the physical parameters (make_lines_adjoint) ----
    {
      lines_adjoint_finalize<NI>(L, LB);   // deferred wavefront-uniform factors of point_reverse
      double lb[NLB];
      lines_adj_store<NI>(LB, lb);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < NLB; ++k) {
        const double v = wave_sum(lb[k]);
        if (lane == 0) m.red[wv * NLB + k] = v;
      }
      __syncthreads();
      if (ht == 0) {
        const double* r = m.red + (half * NW) * NLB;
#pragma unroll
        for (int k = 0; k < NLB; ++k) {
          double v = (r[k] + r[NLB + k]) + (r[2 * NLB + k] + r[3 * NLB + k]);
          if (NW == 8) v += (r[4 * NLB + k] + r[5 * NLB + k]) + (r[6 * NLB + k] + r[7 * NLB + k]);
          lb[k] = v;
        }
        lines_adj_load<NI>(lb, true, LB);
        Phys<NI> p;
        phys_from_lds<NI>(m.phys, p);
        double pbar[NPk];
#pragma unroll
        for (int s = 0; s < NPk; ++s) pbar[s] = 0.0;
        make_lines_adjoint<NI>(p, lam_shift, g, G, L, LB, pbar);
#pragma unroll
        for (int s = 0; s < NPk; ++s) gsum[half * NPk + s] += pbar[s];
      }
    }
  }
  if (GM == 2) {  // table adjoints of this lineout -> global (k_fe_adjoint chains them to f_e)
    fe_flush_w(fa, T.Wb);
    fe_flush_h(fa, T.Hy, T.Hs);
    __syncthreads();
    // interleaved plan: the two workgroups of a lineout leave their parts in [f][B][.] blocks, k_add_parts sums them
    const size_t pw = interleaved ? (size_t)f * K.B * kNXi2 : 0, phs = interleaved ? (size_t)f * 2 * K.B * S.nvx : 0;
    const bool acc = accumulate && !interleaved;
    for (int i = tid; i < kNXi2; i += blockDim.x) {
      double* o = K.Wb_out + pw + (size_t)b * kNXi2 + i;
      *o = acc ? *o + T.Wb[i] : T.Wb[i];
    }
    for (int i = tid; i < S.nvx; i += blockDim.x) {
      double* oy = K.Hy_out + phs + (size_t)b * S.nvx + i;
      double* os = K.Hs_out + phs + (size_t)b * S.nvx + i;
      *oy = acc ? *oy + T.Hy[i] : T.Hy[i];
      *os = acc ? *os + T.Hs[i] : T.Hs[i];
    }
  }
  // amplitudes (irf.py:76,126-130)
  if (ht == 0) amp_adjoint(f, a1b, a2b, gsum + half * NPk);
  __syncthreads();
  // ---- feature sum and the chain rule to the normalised leaves (Ti tying, fraction renormalisation,
  //      activation; ts_params.py:329-350, 543-563) ----
  if (tid == 0) {
    if (nfeat > 1)
      for (int s = 0; s < NPk; ++s) gsum[s] += gsum[NPk + s];
    Phys<NI> p;
    phys_from_lds<NI>(m.phys, p);
    tie_renorm_adjoint<NI>(S, p, GM == 1, gsum);
  }
  __syncthreads();
  if (tid < NPk) {
    const double xv = xpar[tid];
    const double v = activation_adjoint(gsum[tid], S.p_scale[tid], S.p_sig[tid], [&] { return sigmoid(xv); }, gmask[tid]);
    if (interleaved) K.gpart[((size_t)f * K.B + b) * NPk + tid] = v;  // summed over the two features by k_loss_reduce
    else grad[(size_t)b * NPk + tid] = accumulate ? grad[(size_t)b * NPk + tid] + v : v;
  }
}

// a[i] += b[i] (per-feature parts of the table adjoints, interleaved plan)
__global__ __launch_bounds__(kThreads) void k_add_parts(double* __restrict__ a, const double* __restrict__ b, long n) {
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) a[i] += b[i];
}

// deterministic reduction of lpart[B][3] -> out[3] by workgroup 0 in a fixed order; with gpart (interleaved plan) every
// workgroup also adds the two per-feature gradient parts: grad[i] = gpart[0][i] + gpart[1][i], i < n
__global__ __launch_bounds__(kThreads) void k_loss_reduce(const double* __restrict__ lpart, int B, double* __restrict__ out,
                                                          const double* __restrict__ gpart, long n, double* __restrict__ grad) {
  __shared__ double red[8];
  if (gpart) {
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) grad[i] = gpart[i] + gpart[n + i];
  }
  if (blockIdx.x != 0) return;
  double a[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += kThreads) {
    a[0] += lpart[(size_t)b * 3 + 0]; a[1] += lpart[(size_t)b * 3 + 1]; a[2] += lpart[(size_t)b * 3 + 2];
  }
  for (int k = 0; k < 3; ++k) {
    const double v = block_sum(a[k], red);
    if (threadIdx.x == 0) out[k] = v;
  }
}

// tsff_loss_grad_packed: the gradient in the layout the optimiser consumes (the flat vector of ravel_pytree, loops.py:40-54:
// trainable leaves outermost, lineouts of the GLOBAL batch innermost) written straight into the buffer of the step's one
// all-reduce: packed = [S_iaw, S_blue, S_red | g[k][b_global]], k < n_act.  This rank fills the columns
// [b_off, b_off + B) from its per-lineout gradient (grad[B][NP], or the sum of the two per-feature parts of the interleaved
// plan) and writes ZERO everywhere else, so the buffer can be all-reduced in place step after step without a memset.
// The loss sums are reduced by workgroup 0 in a fixed order, as in k_loss_reduce.
__global__ __launch_bounds__(kThreads) void k_loss_reduce_packed(const double* __restrict__ lpart, int B, const double* __restrict__ gpart,
                                                                 const double* __restrict__ grad, int NP, const int* __restrict__ act,
                                                                 int n_act, long B_global, long b_off, double* __restrict__ packed) {
  __shared__ double red[8];
  const long n = (long)n_act * B_global, nbnp = (long)B * NP;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const long k = i / B_global, bl = i - k * B_global - b_off;
    double v = 0.0;
    if (bl >= 0 && bl < B) {
      const long o = bl * NP + act[k];
      v = gpart ? gpart[o] + gpart[nbnp + o] : grad[o];
    }
    packed[3 + i] = v;
  }
  if (blockIdx.x != 0) return;
  double a[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < B; b += kThreads) {
    a[0] += lpart[(size_t)b * 3 + 0]; a[1] += lpart[(size_t)b * 3 + 1]; a[2] += lpart[(size_t)b * 3 + 2];
  }
  for (int k = 0; k < 3; ++k) {
    const double v = block_sum(a[k], red);
    if (threadIdx.x == 0) packed[k] = v;
  }
}

// tsff_pack_fe_rows: the packed buffer of a free-form f_e step, [S_iaw, S_blue, S_red | rows x B_global] with the rows of the
// optimiser's ravel order -- the n_act scalar leaves (from grad[B][NP]) followed by the nvx values of d loss / d f_e (from
// grad_fe[B][nvx]) -- this rank's columns [b_off, b_off + B) filled, every other column zero (cf. k_loss_reduce_packed).  A
// 32 x 32 LDS tile transposes [lineout][row] into [row][lineout] so that both sides move whole cache lines.
__global__ __launch_bounds__(kThreads) void k_pack_fe_rows(const double* __restrict__ terms, const double* __restrict__ grad, int NP,
                                                           const double* __restrict__ grad_fe, int nvx, int B, const int* __restrict__ act,
                                                           int n_act, long B_global, long b_off, double* __restrict__ packed) {
  __shared__ double tile[32][33];
  const int nrows = n_act + nvx, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8 threads
  const long ntb = (B_global + 31) / 32, ntr = (nrows + 31) / 32;
  if (blockIdx.x == 0 && threadIdx.x < 3) packed[threadIdx.x] = terms[threadIdx.x];
  for (long t = blockIdx.x; t < ntb * ntr; t += gridDim.x) {
    const long tb = t % ntb, tr = t / ntb;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // read: rows fastest (contiguous in grad_fe)
      const long bl = tb * 32 + ty + 8 * k - b_off;
      const int r = (int)(tr * 32) + tx;
      double v = 0.0;
      if (bl >= 0 && bl < B && r < nrows) v = r < n_act ? grad[bl * NP + act[r]] : grad_fe[bl * nvx + (r - n_act)];
      tile[ty + 8 * k][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // write: lineouts fastest
      const long bg = tb * 32 + tx;
      const int r = (int)(tr * 32) + ty + 8 * k;
      if (bg < B_global && r < nrows) packed[3 + (long)r * B_global + bg] = tile[tx][ty + 8 * k];
    }
  }
}
