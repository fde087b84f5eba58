// tsff_api.inc -- host side of libtsff.so: the C ABI declared in include/tsff.h.
// Included at the end of tsff_kernels.hip (single translation unit, no -fgpu-rdc needed).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace tsff {

static thread_local std::string g_create_error;
constexpr size_t kLdsLimit = 160 * 1024;  // LDS per CU (and per workgroup) on gfx950

enum PlanBit : int {   // the bits of TSFF_OPT_LAUNCH_PLAN (tsff.h; 16 and 128 are not in use and are refused)
  kPlanNoInterleave = 1,   // never interleave the features (both in one workgroup / split as the budget allows), no split forms
  kPlanTwoSweep = 2,       // never the one-sweep kernel (nor the rows kernel)
  kPlanNeverThree = 4,     // never three forward workgroups per CU
  kPlanNoExchange = 8,     // no base-point exchange
  kPlanGemm128 = 32,       // the 128 x 128 tiling of the W-table GEMM
  kPlanOnePerCU = 64,      // one workgroup per CU (measurements)
  kPlanNoPairs = 256,      // never the pair-sweep forward kernel
};
constexpr int kPlanBits = kPlanNoInterleave | kPlanTwoSweep | kPlanNeverThree | kPlanNoExchange | kPlanGemm128 | kPlanOnePerCU | kPlanNoPairs;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t ensure(size_t n) {
    if (n <= bytes) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// what the projection records of a saving 2-D forward were made from: the adjoint may use them for exactly that (use_saved)
struct ProjRecords {
  long begin = -1, end = -1;
  int nv = 0, feature = -1, B = 0;
  const void *phys = nullptr, *fe = nullptr;
  double ud = 0.0, va = 0.0;
  void invalidate() { begin = end = -1; }
  bool covers(long b, long e, int nv_, int feature_) const { return begin == b && end == e && nv == nv_ && feature == feature_; }
  bool made_from(const void* phys_, const void* fe_, double ud_, double va_, int B_) const {
    return phys == phys_ && fe == fe_ && ud == ud_ && va == va_ && B == B_;
  }
};

}  // namespace tsff

struct tsff_handle {
  tsff::KStatic S{};
  int device = 0;
  int n_ion = 1;
  int fe_mode = 0;
  hipStream_t stream = nullptr;
  // tsff_set_stream: ev_switch orders the next stream behind the work earlier calls left on the previous one; `enqueued`: a call
  // has run since the last switch; `capturing`: the current call's stream is being captured into a graph (set by DevGuard)
  hipEvent_t ev_switch = nullptr;
  bool enqueued = false, capturing = false;
  std::string err;
  std::string launched;   // tsff_last_launch: the kernels the current entry point enqueued, ';'-separated
  // static device arrays
  tsff::DevBuf etab;
  tsff::DevBuf omgs[2], lam_bin[2], filt, cos_sa, sa_rad, w_sa, zp, zpf, xi1, xi2, taps[2], ptaps[2], mask[2], p_scale, p_shift, p_sig,
      dlm, gmask, lg;
  // tables (slot 0 = shared fe); htm/Wm: tangents w.r.t. the DLM order; X/cst: inputs of k_wgemm
  tsff::DevBuf ht, W, fe_tmp, htm, Wm, X, cst;
  size_t smem_vectors = 0;
  int kw_lo = 0, kw_hi = TSFF_NXI1;   // K window of k_wgemm: X rows are exactly zero outside (see there)
  int denom_mode = 0;  // TSFF_OPT_DENOM_MODE
  int plan = 0;        // TSFF_OPT_LAUNCH_PLAN
  // The pipelined DLM plan (TSFF_OPT_DLM_BLOCKS, OFF by default): the per-lineout tables of column block i + 1 of the batch
  // (k_fe_vectors + the FP64-MFMA GEMM) are built on a second stream while the one-sweep kernel (FP64 VALU) works on block i.
  // Measured a LOSS on gfx950 (1.82 -> 1.97 / 2.05 / 2.26 ms per step with 2 / 4 / 8 blocks, profiles/r03l_dlm_blocks.txt): the FP64
  // matrix instruction runs at exactly the vector FMA rate (64 cycles per v_mfma_f64_16x16x4) and a wavefront issuing it back to
  // back leaves the other wavefront of its SIMD one VALU slot in ~190 cycles (scripts/ubench_coissue.hip,
  // profiles/r03l_ubench_coissue.txt) -- the "two pipes" are one FP64 datapath, so the kernels can only share the device in
  // space, and every block pays its own fill and drain.  Kept as an option for devices where the matrix pipe is separate.
  // aux: the second stream (created on first use, non-blocking, higher priority); ev_fork: main -> aux at the start of a call;
  // blk_ev[i]: tables of block i ready.
  int dlm_blocks = 0;                 // 0 / 1: off (one stream), n: n column blocks
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr;
  std::vector<hipEvent_t> blk_ev;
  int pipe_nblk = 0, pipe_nb = 0;     // blocks in flight on aux for the current call (0: none), lineouts per block
  // angular (ARTS) instrument chain
  tsff::DevBuf Wb, Hys, Yt;  // table adjoints of the f_e gradient
  tsff::DevBuf gpart;        // per-feature gradient parts of the interleaved launch plan
  tsff::DevBuf lbrec;        // per (item, wavefront) lineout-scalar adjoints of k_spectrum_fused (k_fused_finish)
  tsff::DevBuf lrec, finrec; // per item lineout scalars of k_fused_prep (for the one-sweep kernel / for k_fused_finish); lrec holds, behind
                             // the kLineRec doubles of every item, the angle records of the one-sweep kernel (2 n_angles doubles per item)
  tsff::DevBuf fpad;         // padded copies of 2-D tables that do not fit LDS
  tsff::DevBuf rows;         // Jacobian rows of k_spectrum_rows (points_per_pixel > 1)
  tsff::DevBuf tickets;      // per (lineout, feature) arrival counters of its split form (small batches)
  tsff::DevBuf proj;         // projection records of tsff_form_factor_2d_save (proj2d_doubles per point)
  tsff::DevBuf fbar_parts;   // per-workgroup partial tiles of the table adjoint
  tsff::ProjRecords proj_rec;
  uint64_t proj_token = 0, proj_counter = 0;   // generation token of the records (0: none); see tsff_form_factor_2d_save
  tsff::DevBuf lbparts;      // per-worker partials of the lineout-scalar adjoints (summed in a fixed order by k_lbacc_reduce)
  tsff::DevBuf lbacc, f1bar, fbar_pad;  // adjoint of the 2-D path: lineout-scalar adjoints, f1bar per point, padded table adjoint
  mutable int ncu_cached = 0;
  int ncu2d() const {
    if (ncu_cached <= 0) {
      int n = 256;
      (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device);
      ncu_cached = n > 0 ? n : 256;
    }
    return ncu_cached;
  }
  std::vector<uint8_t> gmask_host;  // last gradient mask uploaded (re-sent only when it changes)
  tsff::DevBuf act, gradws;         // tsff_loss_grad_packed: active slots on the device, per-lineout gradient workspace
  // tsff_adam_fit / tsff_lbfgs_fit: the packed buffer of their steps.  One for both, as gradws and act are shared: a handle runs
  // one call at a time (handles are not thread-safe, tsff.h) and a stream switch is ordered behind the previous stream by ev_switch
  tsff::DevBuf fit_packed;
  tsff::DevBuf adam_best;                // tsff_adam_fit: the ping-pong pair of best losses
  tsff::DevBuf ang_ws;                   // tsff_angular_fit: parameters, tables, image, seed and adjoints of one epoch
  tsff::DevBuf sph_ws;                   // tsff_sph_table(_vjp): the radial functions and the point adjoint (k_sph.inc)
  tsff::DevBuf arb1v_ws;                 // tsff_arb1v_table(_vjp): u = S fval and its adjoint (k_arb1v.inc)
  std::vector<int32_t> act_host;
  tsff::DevBuf hws, hout;          // tsff_loss_hess: hyper-dual spectra of the persistent workgroups, per-task sums
  tsff::DevBuf htmm, Xmm, cstmm, Wmm, Wmm_unused;   // tsff_loss_hess with the DLM order m: second m-derivative tables
  tsff::DevBuf jrows;              // tsff_spectrum_jacobian / tsff_loss_gauss_newton: per persistent workgroup the row form's spectrum and
                                   // tangents ((1 + n_active) x npts doubles) and the Gauss-Newton call's Jacobian rows (n_active x 1024)
  tsff::DevBuf jv_htd, jv_X, jv_cst, jv_Wd;   // tsff_form_factor_jvp: the table tangents of a block of directions (k_fe_direction + k_wgemm<2>)
  tsff::DevBuf ff2j_tab, ff2j_pad, ff2j_P, ff2j_flags;   // tsff_form_factor_2d_jvp: the projections of a group's tangent tables, the padded tangent
                                          // table (L1/L2 path), the value when the caller asks for none, which directions have a table tangent
  tsff::DevBuf ats_E;              // tsff_ats_jvp: the third tangent image (ats_C, ats_D and this one hold M', A', B')
  tsff::DevBuf ahess_ws;           // tsff_angular_loss_hess: the physical parameters, P and its derivative images, the per-leaf ARTS images, E / E1 / E2
  tsff::DevBuf lm_ws;              // tsff_lm_fit: the gradient [B][n_active] and Gauss-Newton matrix [B][n_active][n_active] of an evaluation
  size_t smem_adjoint = 0;
  tsff::DevBuf ats_w, ats_ta, ats_tl, ats_lam, ats_M, ats_A, ats_B, ats_C, ats_D, ats_stats;
  int ats_npx = 0, ats_nta = 0, ats_offa = 0, ats_ntl = 0, ats_offl = 0, ats_lam_step = 1, ats_ang_step = 1,
      ats_row_start = 0, ats_row_end = 0;
  // per-call workspace
  tsff::DevBuf lpart;
  int reserved_B = 0;
  std::vector<double> lamE_bin, lamI_bin;
  std::vector<double> omgs_host[2];
  size_t smem_spectrum = 0, smem_prepare = 0, smem_ff = 0;
  // timing ring: one HIP event pair per main-kernel launch, recorded on the handle's stream
  bool timing = false;
  std::vector<hipEvent_t> ev0, ev1;
  size_t ev_count = 0;  // launches recorded since tsff_enable_timing
};

namespace tsff {

static int fail(tsff_handle* h, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (h) h->err = buf; else g_create_error = buf;
  return code;
}

// every entry point runs with the handle's device current (a handle is bound to the device that was current at
// tsff_create) and restores the caller's device on return
// (and starts the launch record of tsff_last_launch: the string keeps its capacity, so recording allocates nothing once a call's
// names have fitted)
// An entry point's guard also notes whether its stream is being captured into a graph, and on the way out joins the DLM tables
// still in flight on the second stream (join_pipe), whichever return path the call took -- nothing is left unordered behind the
// handle's stream.  call = false (tsff_set_stream, tsff_destroy): the device only.
static int join_pipe(tsff_handle* h);
struct DevGuard {
  int prev = -1;
  tsff_handle* call = nullptr;
  explicit DevGuard(tsff_handle* h, bool is_call = true) {
    if (!h) return;
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != h->device && hipSetDevice(h->device) == hipSuccess) prev = cur;
    if (!is_call) return;
    call = h;
    h->launched.clear();
    h->enqueued = true;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    h->capturing = hipStreamIsCapturing(h->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
  }
  ~DevGuard() {
    if (call) (void)join_pipe(call);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

// tsff_last_launch: every kernel launch goes through TSFF_LAUNCH / TSFF_LAUNCH0 / TSFF_LAUNCH_FN, which append the kernel's name
// spelled like its demangled device symbol (every template argument included, defaults too) to h->launched
static void note_arg(std::string& s, bool v) { s += v ? "true" : "false"; }
static void note_arg(std::string& s, int v) {
  char b[16];
  snprintf(b, sizeof b, "%d", v);
  s += b;
}
template <class... A>
static const char* note_launch(tsff_handle* h, const char* kernel, A... targs) {   // (returns the name it appended)
  std::string& s = h->launched;
  if (!s.empty()) s += ';';
  const size_t at = s.size();
  s += kernel;
  if constexpr (sizeof...(A) > 0) {
    int i = 0;
    s += '<';
    ((s += i++ ? ", " : "", note_arg(s, targs)), ...);
    s += '>';
  }
  return s.c_str() + at;
}
#define TSFF_UNPAREN(...) __VA_ARGS__
// TSFF_LAUNCH(h, k_name, (template arguments), grid, block, smem, stream, kernel arguments...)
#define TSFF_LAUNCH(h, K, TARGS, ...)                              \
  do {                                                             \
    note_launch((h), #K, TSFF_UNPAREN TARGS);                      \
    hipLaunchKernelGGL((K<TSFF_UNPAREN TARGS>), __VA_ARGS__);      \
  } while (0)
#define TSFF_LAUNCH0(h, K, ...)                                    \
  do {                                                             \
    note_launch((h), #K);                                          \
    hipLaunchKernelGGL(K, __VA_ARGS__);                            \
  } while (0)

#define TSFF_HIP(h, call)                                                                         \
  do {                                                                                            \
    hipError_t e__ = (call);                                                                      \
    if (e__ != hipSuccess) return fail((h), -5, "%s failed: %s", #call, hipGetErrorString(e__)); \
  } while (0)

// a per-handle device buffer that must hold N bytes: grown (hipFree + hipMalloc) only outside graph capture -- a call on a
// capturing stream that would have to grow one is refused with -2 before it enqueues anything (see tsff_reserve)
#define TSFF_ENSURE(h, BUF, N)                                                                                            \
  do {                                                                                                                    \
    const size_t n__ = (N);                                                                                               \
    if (n__ > (BUF).bytes) {                                                                                              \
      if ((h)->capturing) return fail((h), -2, "graph capture: %s needs %zu bytes (tsff_reserve the batch first)", #BUF, n__); \
      TSFF_HIP(h, (BUF).ensure(n__));                                                                                     \
    }                                                                                                                     \
  } while (0)

// TSFF_LAUNCH_FN(h, selector's pointer, ("k_name", template arguments as run-time values), grid, block, smem, stream, kernel
// arguments...): the launch of a family whose instantiations a selector names (below).  A null pointer -- the caller asked for
// a form that does not ship -- is an internal error
#define TSFF_LAUNCH_FN(h, FN, NAME, ...)                                                                        \
  do {                                                                                                          \
    const auto fn__ = (FN);                                                                                     \
    const char* name__ = note_launch((h), TSFF_UNPAREN NAME);                                                   \
    if (!fn__) return fail((h), -5, "internal error: %s is not a shipped instantiation", name__);               \
    hipLaunchKernelGGL(fn__, __VA_ARGS__);                                                                      \
  } while (0)

// runtime value -> template argument: f(std::integral_constant<int, n>) for n in [1, MAX] (nothing otherwise), f(bool_constant)
template <int MAX, class F>
static auto with_ion(int n, F&& f) {
  using R = decltype(f(std::integral_constant<int, 1>{}));
  if constexpr (MAX > 1)
    if (n < MAX) return with_ion<MAX - 1>(n, f);
  if (n == MAX) return f(std::integral_constant<int, MAX>{});
  return R();
}
template <class F>
static auto with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <class F>
static auto with_bools(bool a, bool b, F&& f) { return with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { return f(A, B); }); }); }
template <int V> using IntC = std::integral_constant<int, V>;
// TSFF_LAUNCH_ION(h, MAX, k_name, grid, ...): k_name<n_ion> for the handle's ion count (1 .. MAX; nothing otherwise)
#define TSFF_LAUNCH_ION(h, MAX, K, ...) with_ion<MAX>((h)->n_ion, [&](auto N) { TSFF_LAUNCH(h, K, (N.value), __VA_ARGS__); })

// timing ring: one event pair per main-kernel launch (tsff_enable_timing), recorded on the handle's stream
static size_t timing_slot(const tsff_handle* h) { return h->ev0.empty() ? 0 : h->ev_count % h->ev0.size(); }
static int timing_begin(tsff_handle* h) {
  if (h->timing) TSFF_HIP(h, hipEventRecord(h->ev0[timing_slot(h)], h->stream));
  return 0;
}
static int timing_end(tsff_handle* h) {
  if (h->timing) {
    TSFF_HIP(h, hipEventRecord(h->ev1[timing_slot(h)], h->stream));
    h->ev_count++;
  }
  return 0;
}

// the gradient mask on the device; re-sent (synchronously: pageable source) only when it changes -- refused inside graph capture
static int upload_mask(tsff_handle* h, const uint8_t* grad_mask) {
  if (h->gmask_host.size() == (size_t)h->S.NP && std::memcmp(h->gmask_host.data(), grad_mask, h->S.NP) == 0) return 0;
  if (h->capturing) return fail(h, -2, "graph capture: the gradient mask differs from the last eager call's (a change is uploaded synchronously)");
  h->gmask_host.assign(grad_mask, grad_mask + h->S.NP);
  TSFF_HIP(h, hipStreamSynchronize(h->stream));
  TSFF_HIP(h, hipMemcpy(h->gmask.p, h->gmask_host.data(), h->S.NP, hipMemcpyHostToDevice));
  return 0;
}

// the active slots of the packed outputs on the device; re-sent only when the list changes
static int upload_slots(tsff_handle* h, const int32_t* act, int n) {
  if (h->act_host.size() == (size_t)n && std::memcmp(h->act_host.data(), act, n * sizeof(int32_t)) == 0) return 0;
  if (h->capturing)
    return fail(h, -2, "graph capture: the active slot list differs from the last eager call's (a change is uploaded synchronously)");
  h->act_host.assign(act, act + n);
  TSFF_ENSURE(h, h->act, kNP_MAX * sizeof(int32_t));
  // (pageable source that the next call may reassign: a synchronous copy of <= NP indices, once per change of the slot list)
  TSFF_HIP(h, hipStreamSynchronize(h->stream));
  TSFF_HIP(h, hipMemcpy(h->act.p, h->act_host.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
  return 0;
}

template <class T>
static hipError_t upload(DevBuf& b, const T* src, size_t n) {
  hipError_t e = b.ensure(n * sizeof(T) ? n * sizeof(T) : 8);
  if (e != hipSuccess) return e;
  if (n) return hipMemcpy(b.p, src, n * sizeof(T), hipMemcpyHostToDevice);
  return hipSuccess;
}

// ---- What ships.  One selector per kernel family: the run-time values of its template arguments -> the instantiation's
// pointer (all instantiations of a family have one function type), nullptr for a combination that does not ship.  A selector is
// the only place that names its family's instantiations (one more name, one more kernel in the library): the launches ask it for
// the pointer (TSFF_LAUNCH_FN), tsff_create walks its domain to raise the LDS limit (raise_lds_limits).

// the two-sweep kernel: (MODE, GM) in {(0, 0), (1, 0), (1, 1), (1, 2), (2, 0)} x (TPF, ZH) in {(256, false), (256, true), (512, true)} --
// 512 threads per feature ships with the half Z' table only
static auto spectrum_kernel(int n_ion, int mode, int gm, int tpf, bool zh) {
  using SpectrumFn = decltype(&k_spectrum<1, 0>);
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) -> SpectrumFn {
    auto tz = [&](auto MODE, auto GM) -> SpectrumFn {
      if (tpf == kHalf) return zh ? &k_spectrum<N.value, MODE.value, GM.value, kHalf, true> : &k_spectrum<N.value, MODE.value, GM.value, kHalf, false>;
      return tpf == 2 * kHalf && zh ? &k_spectrum<N.value, MODE.value, GM.value, 2 * kHalf, true> : nullptr;
    };
    if (mode == 1) return gm == 0 ? tz(IntC<1>(), IntC<0>()) : gm == 1 ? tz(IntC<1>(), IntC<1>()) : gm == 2 ? tz(IntC<1>(), IntC<2>()) : nullptr;
    if (gm != 0) return nullptr;
    return mode == 0 ? tz(IntC<0>(), IntC<0>()) : mode == 2 ? tz(IntC<2>(), IntC<0>()) : nullptr;
  });
}

// the one-sweep kernel: GM 0 / 1 x ZH x EX, n_ion <= kFusedMaxIon
static auto fused_kernel(int n_ion, int gm, bool zh, bool ex) {
  using FusedFn = decltype(&k_spectrum_fused<1, 0, false>);
  return with_ion<kFusedMaxIon>(n_ion, [&](auto N) -> FusedFn {
    return with_bools(zh, ex, [&](auto ZH, auto EX) -> FusedFn {
      return gm == 0 ? &k_spectrum_fused<N.value, 0, ZH.value, EX.value> : gm == 1 ? &k_spectrum_fused<N.value, 1, ZH.value, EX.value> : nullptr;
    });
  });
}

// the forward pair sweep: the nine (ZH, EXM, NPAIR) forms (., 0, 1), (., 2, 1), (., 0, 2), (., 1, 2) and (true, 2, 2).  EXM: 0 no exchange,
// 1 and 2 the lane exchange (one form since it runs in registers; the planner's two-per-CU and wide / three-per-CU choices keep
// their numbers, k_forward.inc)
static auto pairs_kernel(int n_ion, bool zh, int exm, int npair) {
  using PairsFn = decltype(&k_forward_pairs<1, false, 0, 1>);
  return with_ion<kFusedMaxIon>(n_ion, [&](auto N) -> PairsFn {
    auto z = [&](auto EXM, auto NPAIR) -> PairsFn {
      return zh ? &k_forward_pairs<N.value, true, EXM.value, NPAIR.value> : &k_forward_pairs<N.value, false, EXM.value, NPAIR.value>;
    };
    if (npair == 1) return exm == 0 ? z(IntC<0>(), IntC<1>()) : exm == 2 ? z(IntC<2>(), IntC<1>()) : nullptr;
    if (npair != 2) return nullptr;
    if (exm == 2) return zh ? &k_forward_pairs<N.value, true, 2, 2> : nullptr;
    return exm == 0 ? z(IntC<0>(), IntC<2>()) : exm == 1 ? z(IntC<1>(), IntC<2>()) : nullptr;
  });
}

// the rows kernel (points_per_pixel > 1): loss + gradient (FWD false) GM 0 / 1 x ZH x EX; forward only (FWD true) with GM 0
static auto rows_kernel(int n_ion, int gm, bool zh, bool ex, bool fwd) {
  using RowsFn = decltype(&k_spectrum_rows<1, 0, false, false>);
  return with_ion<kFusedMaxIon>(n_ion, [&](auto N) -> RowsFn {
    return with_bools(zh, ex, [&](auto ZH, auto EX) -> RowsFn {
      if (fwd) return gm == 0 ? &k_spectrum_rows<N.value, 0, ZH.value, EX.value, true> : nullptr;
      return gm == 0 ? &k_spectrum_rows<N.value, 0, ZH.value, EX.value, false> : gm == 1 ? &k_spectrum_rows<N.value, 1, ZH.value, EX.value, false> : nullptr;
    });
  });
}

// the other families with more than 64 KB of dynamic LDS (the form-factor adjoint: GM 2 with the f_e adjoint; the 2-D kernels: the
// point groups follow from where the table lives)
static auto form_factor_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_form_factor<N.value>; }); }
static auto fe_prepare_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_fe_prepare<N.value>; }); }
static auto fe_vectors_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_fe_vectors<N.value>; }); }
static auto hess_pairs_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_hess_pairs<N.value>; }); }
// the Jacobian sweep: groups of W = 3 tangents, or of 1 (a single leaf; a spectrum too long for the LDS with three); rows: the row
// form of the sweep (W = 3, n_ion <= kFusedMaxIon: the reverse of the pair-sweep kernels)
static auto jac_kernel(int n_ion, int width, bool rows) {
  using JacFn = decltype(&k_jac_sweep<1, 1, false>);
  if (rows)
    return width != 3 ? JacFn(nullptr) : with_ion<kFusedMaxIon>(n_ion, [&](auto N) -> JacFn { return &k_jac_sweep<N.value, 3, true>; });
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) -> JacFn {
    return width == 3 ? &k_jac_sweep<N.value, 3, false> : width == 1 ? &k_jac_sweep<N.value, 1, false> : nullptr;
  });
}
static auto form_factor_adj_kernel(int n_ion, bool grad_fe) {
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) { return grad_fe ? &k_form_factor_adj<N.value, 2> : &k_form_factor_adj<N.value, 0>; });
}
// the forward mode of the 1-D form factor: groups of three directions
static auto ffjvp_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_ffjvp<N.value, 3>; }); }
// its second-order forward mode (tsff_angular_loss_hess)
static auto ffhess_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_ffhess<N.value>; }); }
static auto form_factor_2d_kernel(int n_ion, bool lds, bool save) {
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) {
    return with_bools(lds, save, [&](auto LDS, auto SAVE) { return &k_form_factor_2d<N.value, LDS.value, LDS.value ? TSFF_2D_GROUPS_LDS : TSFF_2D_GROUPS_L2, SAVE.value>; });
  });
}
static auto form_factor_2d_adj_kernel(int n_ion, bool lds) {
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) { return lds ? &k_form_factor_2d_adj<N.value, true, TSFF_2D_GROUPS_LDS> : &k_form_factor_2d_adj<N.value, false, TSFF_2D_GROUPS_L2>; });
}

// the forward mode of the 2-D form factor: the projection of a tangent table (the forward's workgroup), the tail in groups of three
constexpr int kFf2dJvpW = 3;
static auto ff2d_project_kernel(int n_ion, bool lds) {
  return with_ion<TSFF_MAX_ION>(n_ion, [&](auto N) { return lds ? &k_ff2d_project<N.value, true, TSFF_2D_GROUPS_LDS> : &k_ff2d_project<N.value, false, TSFF_2D_GROUPS_L2>; });
}
static auto ff2d_jvp_kernel(int n_ion) { return with_ion<TSFF_MAX_ION>(n_ion, [](auto N) { return &k_ff2d_jvp<N.value, kFf2dJvpW>; }); }

// More dynamic LDS than the default limit: raised once, at tsff_create, on every instantiation the selectors ship for the
// handle's ion count and on the single kernels that need it; no launch sets it
// (the attribute is process-wide, not per handle, and is never lowered: the families sized by the velocity grid get the CU's
// whole LDS too, so that creating a handle with a smaller grid never lowers the limit another handle's launches rely on)
static hipError_t raise_lds_limits(int n_ion) {
  hipError_t e = hipSuccess;
  auto raise = [&](auto fn, size_t bytes = kLdsLimit) {
    if (fn && e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  };
  for (int zh = 0; zh < 2; ++zh) {
    for (int mode = 0; mode <= 2; ++mode)
      for (int gm = 0; gm <= 2; ++gm)
        for (int tpf = kHalf; tpf <= 2 * kHalf; tpf += kHalf) raise(spectrum_kernel(n_ion, mode, gm, tpf, zh));
    for (int exm = 0; exm <= 2; ++exm)
      for (int npair = 1; npair <= 2; ++npair) raise(pairs_kernel(n_ion, zh, exm, npair));
    for (int ex = 0; ex < 2; ++ex)
      for (int gm = 0; gm <= 1; ++gm) {
        raise(fused_kernel(n_ion, gm, zh, ex));
        for (int fwd = 0; fwd < 2; ++fwd) raise(rows_kernel(n_ion, gm, zh, ex, fwd));
      }
  }
  for (int a = 0; a < 2; ++a) {
    raise(form_factor_adj_kernel(n_ion, a));
    raise(form_factor_2d_adj_kernel(n_ion, a));
    for (int save = 0; save < 2; ++save) raise(form_factor_2d_kernel(n_ion, a, save));
  }
  raise(form_factor_kernel(n_ion));
  raise(fe_prepare_kernel(n_ion));
  raise(fe_vectors_kernel(n_ion));
  raise(hess_pairs_kernel(n_ion));
  raise(jac_kernel(n_ion, 1, false));
  raise(jac_kernel(n_ion, 3, false));
  raise(jac_kernel(n_ion, 3, true));
  raise(ffjvp_kernel(n_ion));
  raise(ffhess_kernel(n_ion));
  for (int a = 0; a < 2; ++a) raise(ff2d_project_kernel(n_ion, a));
  raise(&k_fe_direction);
  raise(&k_fe_adjoint);
  raise(&k_ff2d_table_adj);
  raise(&k_wgemm_w, kWgemmWSmem);
  return e;
}

constexpr size_t kRowsScratchMax = (size_t)16 << 30;   // the row scratch of k_spectrum_rows (larger: the two-sweep kernel)

// bytes of the scratch buffers of the spectrum plans (nitems: one-feature workgroups, lineouts x loaded features): plan_spectrum
// sizes what a plan needs, ensure_workspace the largest a plan can need
static size_t lbrec_bytes(size_t nitems) { return nitems * (kHalf / 64) * kLBRec * sizeof(double); }
static size_t lrec_bytes(const KStatic& S, size_t nitems, bool angles) {   // (line records | the one-sweep kernel's angle records)
  return nitems * (kLineRec + (angles ? 2 * (size_t)S.n_angles : 0)) * sizeof(double);
}
static size_t finrec_bytes(const tsff_handle& h, size_t nitems) { return nitems * (2 * (size_t)h.S.NP + 1 + 9 + 4 * (size_t)h.n_ion) * sizeof(double); }
static size_t gpart_bytes(const KStatic& S, int B) { return (size_t)2 * B * S.NP * sizeof(double); }
static size_t gradws_bytes(const KStatic& S, int B) { return (size_t)B * S.NP * sizeof(double); }

static int ensure_workspace(tsff_handle* h, int B, bool with_rows = false) {
  if (with_rows && h->S.ppp > 1 && h->S.G == 1 && h->n_ion <= 2) {
    // the row scratch of k_spectrum_rows (points_per_pixel > 1; the widest layout: DLM tangent component included), so that a
    // handle reserved through tsff_reserve allocates nothing in tsff_loss_grad (graph capture)
    const size_t need = (size_t)B * ((h->S.load[0] ? 1 : 0) + (h->S.load[1] ? 1 : 0)) * (9 + 3 * (size_t)h->n_ion) * h->S.npts * sizeof(double);
    if (need <= kRowsScratchMax) TSFF_ENSURE(h, h->rows, need);
  }
  if (B <= h->reserved_B) return 0;
  if (h->capturing) return fail(h, -2, "graph capture: the workspace holds %d lineouts, the call has %d (tsff_reserve the batch first)", h->reserved_B, B);
  const int slots = h->fe_mode == TSFF_FE_SHARED ? 1 : B;
  TSFF_ENSURE(h, h->lpart, (size_t)B * 3 * sizeof(double));
  // the kernels overwrite the slots of the loaded features; the slots of a feature that is not loaded stay zero
  TSFF_HIP(h, hipMemsetAsync(h->lpart.p, 0, (size_t)B * 3 * sizeof(double), h->stream));
  // the records of the one-sweep and pair-sweep kernels, the per-feature gradient parts of the interleaved plans, the packed
  // call's gradient workspace and slot list, and the arrival counters of the rows kernel's split form (zeroed once: the last
  // arrival resets its counter) at their largest over the plans plan_spectrum can pick for B lineouts -- so that a call on a
  // reserved handle allocates nothing (graph capture)
  const size_t nitems = (size_t)B * ((h->S.load[0] ? 1 : 0) + (h->S.load[1] ? 1 : 0));
  TSFF_ENSURE(h, h->lbrec, lbrec_bytes(nitems));
  TSFF_ENSURE(h, h->lrec, lrec_bytes(h->S, nitems, true));
  TSFF_ENSURE(h, h->finrec, finrec_bytes(*h, nitems));
  TSFF_ENSURE(h, h->gpart, gpart_bytes(h->S, B));
  TSFF_ENSURE(h, h->gradws, gradws_bytes(h->S, B));
  TSFF_ENSURE(h, h->act, kNP_MAX * sizeof(int32_t));
  if (h->tickets.bytes < 1024 * sizeof(unsigned)) {
    TSFF_ENSURE(h, h->tickets, 1024 * sizeof(unsigned));
    TSFF_HIP(h, hipMemsetAsync(h->tickets.p, 0, h->tickets.bytes, h->stream));
  }
  if (h->fe_mode != TSFF_FE_SHARED) {
    // growing the table buffers would drop the shared slot; non-shared modes rebuild them per call
    TSFF_ENSURE(h, h->ht, (size_t)slots * h->S.nvx * sizeof(double2));
    TSFF_ENSURE(h, h->W, (size_t)slots * kNXi2 * sizeof(double));
    TSFF_ENSURE(h, h->fe_tmp, (size_t)slots * h->S.nvx * sizeof(double));
    TSFF_ENSURE(h, h->htm, (size_t)slots * h->S.nvx * sizeof(double2));
    TSFF_ENSURE(h, h->Wm, (size_t)slots * kNXi2 * sizeof(double));
    TSFF_ENSURE(h, h->X, (size_t)slots * 4 * kNXi1 * sizeof(double));
    TSFF_ENSURE(h, h->cst, (size_t)slots * 2 * sizeof(double));
  }
  h->reserved_B = B;
  return 0;
}

// launch k_fe_prepare for `slots` distribution functions
static int launch_prepare(tsff_handle* h, const double* fe_dev, int mode, const double* params, int slots,
                          double2* ht, double* W, double* fe_out) {
  const int qsplit = slots >= 64 ? 1 : (slots >= 8 ? 4 : 16);
  dim3 grid(slots, qsplit), block(kThreads);
  TSFF_LAUNCH_FN(h, fe_prepare_kernel(h->n_ion), ("k_fe_prepare", h->n_ion), grid, block, h->smem_prepare, h->stream, h->S, fe_dev, mode,
                 params, ht, W, fe_out);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// the second stream and the events of the pipelined DLM plan
static int ensure_pipe(tsff_handle* h, int nblk) {
  if (!h->aux) {
    int lo = 0, hi = 0;
    TSFF_HIP(h, hipDeviceGetStreamPriorityRange(&lo, &hi));   // (hi = the numerically smallest = the highest priority)
    TSFF_HIP(h, hipStreamCreateWithPriority(&h->aux, hipStreamNonBlocking, hi));
    TSFF_HIP(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  }
  while ((int)h->blk_ev.size() < nblk) {
    hipEvent_t e;
    TSFF_HIP(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->blk_ev.push_back(e);
  }
  return 0;
}
// every consumer other than the per-block launches of launch_fused: wait for the last block (aux is in order)
static int join_pipe(tsff_handle* h) {
  if (h->pipe_nblk > 1) TSFF_HIP(h, hipStreamWaitEvent(h->stream, h->blk_ev[h->pipe_nblk - 1], 0));
  h->pipe_nblk = 0;
  return 0;
}

// k_fe_vectors + the W-table GEMM for lineouts [b0, b0 + nb) on stream st
static int launch_tables_block(tsff_handle* h, const double* params, const double* fe, int b0, int nb, hipStream_t st) {
  const size_t nvx = h->S.nvx;
  const double* fe_b = fe ? fe + (size_t)b0 * nvx : nullptr;
  const double* par_b = params + (size_t)b0 * h->S.NP;
  double2* ht_b = h->ht.as<double2>() + (size_t)b0 * nvx; double2* htm_b = h->htm.as<double2>() + (size_t)b0 * nvx;
  double* X_b = h->X.as<double>() + (size_t)b0 * 4 * kNXi1; double* cst_b = h->cst.as<double>() + (size_t)b0 * 2;
  double* W_b = h->W.as<double>() + (size_t)b0 * kNXi2; double* Wm_b = h->Wm.as<double>() + (size_t)b0 * kNXi2;
  dim3 grid(nb), block(kThreads);
  TSFF_LAUNCH_FN(h, fe_vectors_kernel(h->n_ion), ("k_fe_vectors", h->n_ion), grid, block, h->smem_vectors, st, h->S, fe_b, h->fe_mode, par_b,
                 ht_b, htm_b, X_b, cst_b);
  TSFF_HIP(h, hipGetLastError());
  const int nc = h->fe_mode == TSFF_FE_DLM ? 4 : 2;  // explicit f_e tables carry no tangent vectors
  const int nM = (nb + kGM / nc - 1) / (kGM / nc), nQ = (kNXi2 + kGN - 1) / kGN;
  dim3 ggrid(8 * ((nM + 7) / 8) * nQ);
  if (nc == 4 && !(h->plan & kPlanGemm128)) {   // 128 x 144 tiles: no partial last round (k_wgemm_w); plan bit 5: the 128 x 128 form
    dim3 wgrid(8 * ((nM + 7) / 8) * ((kNXi2 + kGNw - 1) / kGNw));
    TSFF_LAUNCH0(h, k_wgemm_w, wgrid, block, kWgemmWSmem, st, h->S.lg, X_b, cst_b, h->S.xi2, nb, W_b, Wm_b, h->kw_lo, h->kw_hi);
  } else if (nc == 4)
    TSFF_LAUNCH(h, k_wgemm, (4), ggrid, block, 0, st, h->S.lg, X_b, cst_b, h->S.xi2, nb, W_b, Wm_b, h->kw_lo, h->kw_hi);
  else
    TSFF_LAUNCH(h, k_wgemm, (2), ggrid, block, 0, st, h->S.lg, X_b, cst_b, h->S.xi2, nb, W_b, Wm_b, h->kw_lo, h->kw_hi);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// per-call table preparation; fills K.ht / K.W.  pipe: the caller can consume the tables per column block (loss + gradient with
// the DLM order as a leaf: launch_fused) -- the blocks are then built on the second stream, one event each (every other consumer
// joins through join_pipe).
static int prepare_tables(tsff_handle* h, const double* params, const double* fe, int B, KCall& K, bool pipe = false) {
  h->pipe_nblk = 0;
  if (h->fe_mode == TSFF_FE_SHARED) {
    K.ht = h->ht.as<double2>();
    K.W = h->W.as<double>();
    return 0;
  }
  // per-lineout tables: vectors (A, s, dA/dm, ds/dm) per lineout, then W = c + Lg (A + xi2 s) for the whole batch
  // blocks of a multiple of 256 lineouts (the GEMM spreads groups of eight 32-lineout tiles over the XCDs); off unless asked for
  int nblk = 1;
  if (pipe && h->fe_mode == TSFF_FE_DLM && h->dlm_blocks > 1) nblk = h->dlm_blocks;
  int nb = B;
  if (nblk > 1) {
    nb = (((B + nblk - 1) / nblk) + 255) / 256 * 256;
    nblk = (B + nb - 1) / nb;
  }
  if (nblk > 1) {
    int rc = ensure_pipe(h, nblk);
    if (rc) return rc;
    TSFF_HIP(h, hipEventRecord(h->ev_fork, h->stream));
    TSFF_HIP(h, hipStreamWaitEvent(h->aux, h->ev_fork, 0));
    for (int i = 0; i < nblk; ++i) {
      const int b0 = i * nb;
      rc = launch_tables_block(h, params, fe, b0, std::min(nb, B - b0), h->aux);
      if (rc) return rc;
      TSFF_HIP(h, hipEventRecord(h->blk_ev[i], h->aux));
    }
    h->pipe_nblk = nblk; h->pipe_nb = nb;
  } else {
    int rc = launch_tables_block(h, params, fe, 0, B, h->stream);
    if (rc) return rc;
  }
  K.ht = h->ht.as<double2>();
  K.W = h->W.as<double>();
  K.htm = h->htm.as<double2>();
  K.Wm = h->Wm.as<double>();
  return 0;
}

// Launch plan of k_spectrum.  Two loaded features:
//   interleaved (default when two one-feature workgroups fit the LDS of a CU): ONE launch of 2B 256-thread workgroups,
//     workgroup 2b + f evaluates feature f of lineout b; two workgroups per CU overlap each other's barriers, table
//     staging and tails (measured 10 % faster than the fused plan); the gradient parts are added atomically;
//   fused: both features in one 512-thread workgroup (one workgroup per CU) -- used when the LDS footprint does not
//     allow two workgroups per CU (table-adjoint mode with large velocity grids, points_per_pixel > 1);
//   split: one 512-thread launch per feature, the second accumulating into grad (LDS budget exceeded: points_per_pixel 5).
// MODE 1 runs the one-sweep kernel k_spectrum_fused instead wherever its restrictions hold (see plan_spectrum).
// One loaded feature: 256-thread workgroups when two fit a CU, else 512.  The k_s cache is used when it still fits.
// The dispatch: MODE (0 forward, 1 loss + gradient, 2 array loss) and GM (0 plasma parameters, 1 + the DLM order, 2 + the table
// adjoints) are run-time arguments.  plan_spectrum decides the form and its template arguments as fields of the plan (the
// TSFF_OPT_LAUNCH_PLAN bits: PlanBit); launch_spectrum asks the form's selector for that instantiation and launches the pointer.
enum class SpectrumForm { rows, pairs, one_sweep, two_sweep };

struct SpectrumPlan {
  SpectrumForm form = SpectrumForm::two_sweep;
  // zh: the half Z' table; ex: the base-point exchange; ks: the k_s cache; three: three workgroups per CU; wide: two workgroups
  // per item (pair sweep); split: one workgroup per (lineout, feature, round); interleaved: both features' workgroups in one launch
  bool zh = false, ex = false, ks = false, three = false, wide = false, split = false, interleaved = false;
  int nfeat = 1, tpf = kHalf;   // features per workgroup, threads per feature
  size_t smem = 0;
  dim3 grid, block;
  size_t rows = 0, tickets = 0, gpart = 0, lbrec = 0, lrec = 0, finrec = 0;   // bytes of the buffers the form needs (0: none)
};

// the launch plan of one launch_spectrum call: decisions only, nothing allocated or launched (MODE, GM: spelled like the template
// arguments they select)
static SpectrumPlan plan_spectrum(const tsff_handle& h, const int MODE, const int GM, int B, int nload) {
  const KStatic& S = h.S;
  const size_t nitems = (size_t)B * nload;   // one-feature workgroups
  const size_t finrec = finrec_bytes(h, nitems);
  // points_per_pixel > 1, loss + gradient: the one-sweep kernel with its rows in a global scratch array (k_spectrum_rows.inc) -- one
  // launch of 256-thread one-feature workgroups, two per CU (the full Z' table if that still fits, else the half table); the scratch
  // is capped at kRowsScratchMax (larger batches fall back to the two-sweep kernel).  Forward only: the forward form of the rounds
  // kernel (FWD) -- two 256-thread workgroups per CU and, for small batches, the rounds of a lineout on separate workgroups --
  // instead of k_spectrum MODE 0's one 512-thread workgroup per CU
  if ((MODE == 1 && GM <= 1) || (MODE == 0 && GM == 0)) {
    if (S.G == 1 && S.ppp > 1 && h.n_ion <= kFusedMaxIon && !(h.plan & kPlanTwoSweep) && !S.raw[0] && !S.raw[1] && nload >= 1) {
      const bool FWD = MODE == 0;
      SpectrumPlan p;
      p.form = SpectrumForm::rows;
      // (the exchange's 15 KB -- this kernel keeps the form through LDS -- live in the sweep's part of the LDS: free whenever the
      //  chain's buffers are the larger part)
      const size_t exd = kExLdsDoubles;
      p.ex = S.n_angles <= 16 && !(h.plan & kPlanNoExchange) && 2 * sizeof(double) * rows_smem_doubles(S, GM, true, exd) <= kLdsLimit;
      p.zh = 2 * sizeof(double) * rows_smem_doubles(S, GM, false, p.ex ? exd : 0) > kLdsLimit;
      p.smem = sizeof(double) * rows_smem_doubles(S, GM, p.zh, p.ex ? exd : 0);
      p.interleaved = nload == 2;
      p.rows = nitems * (FWD ? 1 : rows_components(h.n_ion, GM)) * (size_t)S.npts * sizeof(double);   // (forward: the value only)
      if (2 * p.smem <= kLdsLimit && (FWD || p.rows <= kRowsScratchMax)) {
        // small batches: one workgroup per (lineout, feature, ROUND), the last one of a (lineout, feature) runs the chain
        p.split = nitems * 2 <= (size_t)h.ncu2d() && !(h.plan & kPlanNoInterleave);
        p.tickets = p.split ? nitems * sizeof(unsigned) : 0;
        if (!FWD && p.interleaved) p.gpart = gpart_bytes(S, B);
        p.grid = p.split ? dim3((unsigned)nitems, (unsigned)S.ppp) : dim3((unsigned)nitems);
        p.block = dim3(kHalf);
        return p;
      }
    }
  }
  // forward only (tsff_forward), one gradient point, one point per pixel: the pair-sweep kernel (k_forward.inc) -- two workgroups
  // per item while the whole batch fits one dispatch round of two items per CU (configs[1]), else one; plan bit 8 (256): never
  if (MODE == 0 && GM == 0) {
    if (S.G == 1 && S.ppp == 1 && h.n_ion <= kFusedMaxIon && !(h.plan & kPlanNoPairs) && nload >= 1) {
      SpectrumPlan p;
      p.form = SpectrumForm::pairs;
      p.ex = S.n_angles <= 16 && !(h.plan & kPlanNoExchange);
      p.interleaved = nload == 2;
      // 512 threads per item (one pair per thread) while the batch fits one round of two items per CU
      p.wide = nitems <= 2 * (size_t)h.ncu2d() && !(h.plan & kPlanNoInterleave);
      // LDS of the forward workgroup (smem_fwd_doubles): two per CU (the full Z' table and the k_s cache as they fit), or -- batches
      // of more than two items per CU -- THREE per CU with the half Z' table and no k_s cache (plan bit 2 (4): never).  EXM 1 and 2
      // cost the same LDS: the exchange itself is in registers, only the unit-boundary points live in LDS
      const size_t exd = p.ex ? kExDoubles : 0, exd2 = p.ex ? kExLdsDoubles : 0;   // (two per CU: decided at kExLdsDoubles, k_spectrum.inc)
      const bool zh2 = 2 * sizeof(double) * smem_fwd_doubles(S, false, false, exd2) > kLdsLimit;
      const bool ks2 = 2 * sizeof(double) * smem_fwd_doubles(S, true, zh2, exd2) <= kLdsLimit;
      const size_t smem3 = sizeof(double) * smem_fwd_doubles(S, false, true, exd);
      p.three = !p.wide && !(h.plan & kPlanNeverThree) && nitems > 2 * (size_t)h.ncu2d() && 3 * smem3 <= kLdsLimit;
      p.zh = p.three || zh2;
      p.ks = !p.three && ks2;
      p.smem = p.three ? smem3 : sizeof(double) * smem_fwd_doubles(S, ks2, zh2, exd);
      if (p.three || 2 * sizeof(double) * smem_fwd_doubles(S, ks2, zh2, p.wide ? exd : exd2) <= kLdsLimit) {
        if (!p.wide) { p.lrec = lrec_bytes(S, nitems, false); p.finrec = finrec; }
        p.grid = dim3((unsigned)nitems);
        p.block = dim3(p.wide ? 2 * kHalf : kHalf);
        return p;
      }
    }
  }
  SpectrumPlan p;
  // the one-sweep kernel (k_spectrum_fused.inc) wherever its restrictions hold: loss + gradient, one gradient point, one point
  // per pixel, 256-thread one-feature workgroups, no table adjoints; with the base-point exchange (EX: lane to lane in registers,
  // 5 KB of LDS for the unit-boundary points, n_angles <= 16) when two such workgroups still fit a CU (the half Z' table makes room)
  const bool fused_ok = MODE == 1 && GM <= 1 && S.G == 1 && S.ppp == 1 && h.n_ion <= kFusedMaxIon && !(h.plan & kPlanTwoSweep);
  p.ex = fused_ok && S.n_angles <= 16 && !(h.plan & kPlanNoExchange) && 2 * sizeof(double) * smem_doubles(S, 1, GM, false, true, true, kExLdsDoubles) <= kLdsLimit;
  // forward-only calls need 139 VGPRs: THREE one-feature workgroups fit a CU's registers, and its LDS too with the half Z' table
  // and without the k_s cache -- 3 wavefronts per SIMD hide the lookups' latency better than 2 (plan bit 2 (4): never); only when
  // there are more workgroups than two per CU (a grid that fits at two per CU gains nothing and pays for the half table)
  p.three = MODE == 0 && !(h.plan & kPlanNeverThree) && (long)nitems > 2L * h.ncu2d() &&
            3 * sizeof(double) * smem_doubles(S, 1, GM, false, alias_xy(S, 256), true) <= kLdsLimit;
  // zh: Z' table held for xi >= 0 only, 13 KB less LDS for about 1 % more instructions -- used only when the full table would
  // cost the two-workgroups-per-CU plan
  p.zh = p.three || 2 * sizeof(double) * smem_doubles(S, 1, GM, false, alias_xy(S, 256), false, p.ex ? kExLdsDoubles : 0) > kLdsLimit;
  // (tpf: threads per feature of the instantiation the size is for -- 256-thread-per-feature workgroups with points_per_pixel 1
  //  keep the per-bin adjoint in the memory of the spectrum, alias_xy)
  // (exc: what the exchange is charged -- kExLdsDoubles for the decisions, kExDoubles for the allocation; k_spectrum.inc)
  auto bytes = [&](int nf, bool ks, int tpf, size_t exc = kExLdsDoubles) {
    return sizeof(double) * smem_doubles(S, nf, GM, ks, alias_xy(S, tpf), p.zh, (p.ex && nf == 1 && tpf == 256) ? exc : 0);
  };
  const bool two_per_cu = 2 * bytes(1, false, 256) <= kLdsLimit;   // two one-feature workgroups per CU
  p.interleaved = nload == 2 && two_per_cu && !(h.plan & kPlanNoInterleave);
  p.nfeat = nload;
  if (p.interleaved || bytes(p.nfeat, false, 256) > kLdsLimit) p.nfeat = 1;
  const bool small_wg = p.nfeat == 1 && two_per_cu;   // 256-thread one-feature workgroups
  p.tpf = (p.nfeat == 2 || small_wg) ? kHalf : 2 * kHalf;
  const size_t budget = small_wg ? kLdsLimit / (p.three ? 3 : 2) : kLdsLimit;
  p.ks = bytes(p.nfeat, true, p.tpf) <= budget;
  p.smem = bytes(p.nfeat, p.ks, p.tpf, kExDoubles);
  if ((h.plan & kPlanOnePerCU) && p.smem <= kLdsLimit / 2) p.smem = kLdsLimit / 2 + 1024;   // (experiments: one workgroup per CU)
  // (the one-sweep kernel: also no second accumulating launch)
  const int nlaunch = p.interleaved ? 1 : nload / p.nfeat;
  if (fused_ok && small_wg && nlaunch == 1) {   // it leaves per-wavefront records; k_fused_finish turns them into the gradient
    p.form = SpectrumForm::one_sweep;
    p.lbrec = lbrec_bytes(nitems);
    p.lrec = lrec_bytes(S, nitems, true);
    p.finrec = finrec;
  } else if (p.interleaved && MODE == 1) {
    p.gpart = gpart_bytes(S, B);
  }
  p.grid = dim3(p.interleaved ? 2 * B : B);
  p.block = dim3(small_wg ? kHalf : 2 * kHalf);
  return p;
}

// the one-sweep kernel k_spectrum_fused (GM: 0 plasma parameters, 1 + the DLM order): the lineout scalars of every item, one
// thread each (k_fused_prep), then one launch over the whole batch, or -- the pipelined DLM plan -- one per column block, each
// behind the event of its tables
static int launch_fused(tsff_handle* h, int gm, const KCall& K, const SpectrumPlan& p, int f0, int flags, int nload) {
  const double* lrec = h->lrec.as<double>();
  TSFF_LAUNCH_ION(h, kFusedMaxIon, k_fused_prep, dim3((p.grid.x + 63) / 64), dim3(64), 0, h->stream, h->S, K.params, K.B, f0, nload,
                  h->lrec.as<double>(), h->finrec.as<double>(), h->lrec.as<double>() + (size_t)K.B * nload * kLineRec);   // (the angle records: behind the line records of all K.B * nload items)
  const int nblk = h->pipe_nblk > 1 ? h->pipe_nblk : 1;
  for (int i = 0; i < nblk; ++i) {
    KCall Kb = K;
    dim3 g = p.grid;
    if (nblk > 1) {
      Kb.b0 = i * h->pipe_nb; Kb.B = std::min(h->pipe_nb, K.B - Kb.b0);
      g = dim3((unsigned)(Kb.B * nload));
      (void)hipStreamWaitEvent(h->stream, h->blk_ev[i], 0);
    }
    TSFF_LAUNCH_FN(h, fused_kernel(h->n_ion, gm, p.zh, p.ex), ("k_spectrum_fused", h->n_ion, gm, p.zh, p.ex), g, p.block, p.smem, h->stream,
                   h->S, Kb, f0, flags, lrec);
  }
  h->pipe_nblk = 0;
  return 0;
}

// the plan launch_spectrum(mode, gm) runs for B lineouts, its LDS budget checked and every scratch buffer of it sized (the
// arrival counters zeroed when they grow) -- before a call enqueues anything, so that a refusal leaves nothing behind
static int size_plan(tsff_handle* h, int mode, int gm, int B, SpectrumPlan& p) {
  const int nload = (h->S.load[0] ? 1 : 0) + (h->S.load[1] ? 1 : 0);
  p = plan_spectrum(*h, mode, gm, B, nload);
  if (p.smem > kLdsLimit) return fail(h, TSFF_ERR_LDS, "LDS budget exceeded (%zu B): reduce npts or the IRF cutoff", p.smem);
  if (p.rows) TSFF_ENSURE(h, h->rows, p.rows);
  if (p.tickets && h->tickets.bytes < p.tickets) {
    TSFF_ENSURE(h, h->tickets, std::max<size_t>(p.tickets, 1024 * sizeof(unsigned)));
    TSFF_HIP(h, hipMemsetAsync(h->tickets.p, 0, h->tickets.bytes, h->stream));
  }
  if (p.gpart) TSFF_ENSURE(h, h->gpart, p.gpart);
  if (p.lbrec) TSFF_ENSURE(h, h->lbrec, p.lbrec);
  if (p.lrec) TSFF_ENSURE(h, h->lrec, p.lrec);
  if (p.finrec) TSFF_ENSURE(h, h->finrec, p.finrec);
  return 0;
}

// the launches of a plan size_plan(mode, gm) made for K.B lineouts: the KCall's pointers into the plan's buffers (K.gpart when
// p.gpart, K.lbrec for the one-sweep form), the pipe, the timing ring, the kernels.  Allocates and refuses nothing; a form that
// does not ship for (mode, gm) -- the planner never picks one -- gets no pointer from its selector: -5.
static int launch_spectrum(tsff_handle* h, int mode, int gm, KCall& K, const SpectrumPlan& p, const uint8_t* gmask = nullptr, double* grad = nullptr) {
  const int nload = (h->S.load[0] ? 1 : 0) + (h->S.load[1] ? 1 : 0), n = h->n_ion;
  // the one-sweep kernel takes the tables block by block; every other form waits for all of them (a no-op for forward calls:
  // only the loss + gradient builds its tables on the second stream)
  if (p.form != SpectrumForm::one_sweep)
    if (int rc = join_pipe(h)) return rc;
  if (p.gpart) K.gpart = h->gpart.as<double>();
  if (p.form == SpectrumForm::one_sweep) K.lbrec = h->lbrec.as<double>();
  if (int rc = timing_begin(h)) return rc;
  const int nlaunch = p.interleaved ? 1 : nload / p.nfeat;
  for (int l = 0; l < nlaunch; ++l) {
    const int f0 = nlaunch == 2 ? l : (h->S.load[0] ? 0 : 1);
    const int flags = (l > 0 ? kFlagAccumulate : 0) | (p.ks ? kFlagKsCache : 0) | (p.interleaved ? kFlagInterleaved : 0) |
                      (p.wide ? kFlagOwnScalars : 0) | (p.split ? kFlagSplit : 0);
    switch (p.form) {
      case SpectrumForm::rows: {   // (loss + gradient, or its forward form)
        const bool fwd = mode == 0;
        TSFF_LAUNCH_FN(h, mode <= 1 ? rows_kernel(n, gm, p.zh, p.ex, fwd) : nullptr, ("k_spectrum_rows", n, gm, p.zh, p.ex, fwd), p.grid,
                       p.block, p.smem, h->stream, h->S, K, f0, flags, gmask, grad, h->rows.as<double>(),
                       p.split ? h->tickets.as<unsigned>() : nullptr);
        break;
      }
      case SpectrumForm::pairs: {   // (forward only)
        double* lrec = h->lrec.as<double>();
        // the exchange goes by 2 wide and with three workgroups per CU (which has the half Z' table), else by 1 (pairs_kernel)
        const bool three_ex = !p.wide && p.three && p.ex;
        const bool zh = three_ex || p.zh;
        const int exm = !p.ex ? 0 : (p.wide || three_ex) ? 2 : 1, npair = p.wide ? 1 : 2;
        if (!p.wide)
          TSFF_LAUNCH_ION(h, kFusedMaxIon, k_fused_prep, dim3((p.grid.x + 63) / 64), dim3(64), 0, h->stream, h->S, K.params, K.B, f0, nload,
                          lrec, h->finrec.as<double>(), (double*)nullptr);
        TSFF_LAUNCH_FN(h, mode == 0 && gm == 0 ? pairs_kernel(n, zh, exm, npair) : nullptr, ("k_forward_pairs", n, zh, exm, npair), p.grid,
                       p.block, p.smem, h->stream, h->S, K, f0, flags, lrec);
        break;
      }
      case SpectrumForm::one_sweep:   // (loss + gradient)
        if (int rc = launch_fused(h, mode == 1 ? gm : -1, K, p, f0, flags, nload)) return rc;
        break;
      case SpectrumForm::two_sweep: {
        const bool zh = p.tpf == kHalf ? p.zh : true;   // (512 threads per feature ships with the half Z' table only)
        TSFF_LAUNCH_FN(h, spectrum_kernel(n, mode, gm, p.tpf, zh), ("k_spectrum", n, mode, gm, p.tpf, zh), p.grid, p.block, p.smem,
                       h->stream, h->S, K, f0, p.nfeat, flags, gmask, grad);
        break;
      }
    }
    TSFF_HIP(h, hipGetLastError());
  }
  return timing_end(h);
}

// blockIdx.y extent of the form-factor kernels: with few lineouts the angles are spread over workgroups (ARTS: one
// lineout, 241 angles), with many lineouts one workgroup per lineout walks them all
static unsigned angle_chunks(const tsff_handle* h, int B) {
  const int want = 4 * h->ncu2d();
  return (unsigned)std::max(1, std::min(h->S.n_angles, want / std::max(B, 1)));
}

// The refusals every entry point shares, each written once.  An entry point checks in this order -- its own arguments (-1), the
// slot list (-1), the leaves (-2, -3), the batch (-1, -2) -- then sizes, then launches (tsff.h).

static int check_fe(tsff_handle* h, const double* fe) {
  if (h->fe_mode == TSFF_FE_PER_LINEOUT && !fe) return fail(h, -2, "fe_mode PER_LINEOUT needs fe[B][nvx]");
  return 0;
}

// the batch of a spectrum call: what the nine batch arguments of an entry point say ([0] the electron feature, [1] the ion one)
struct Batch {
  const double *params, *fe, *data[2], *amps[2], *noise[2];
  int B;
};

static int check_batch(tsff_handle* h, const Batch& b, bool need_data) {
  if (!b.params || b.B < 1) return fail(h, -1, "bad argument");
  for (int f = 0; f < 2; ++f) {
    if (h->S.load[f] && need_data && !b.data[f]) return fail(h, -1, "%c_data missing", "ei"[f]);
    if (h->S.load[f] && !b.amps[f]) return fail(h, -1, "%c_amps missing", "ei"[f]);
  }
  return check_fe(h, b.fe);
}

// the leaves a gradient mask asks for; m_ok: the DLM order m can be one (fe_mode DLM; tsff_angular_fit: a DLM deck)
static int check_mask(tsff_handle* h, const uint8_t* gm, bool m_ok) {
  if (gm[TSFF_P_M] && !m_ok)
    return fail(h, -2, "gradient w.r.t. the DLM order m needs fe_mode == TSFF_FE_DLM (tsff_angular_fit: a DLM deck)");
  for (int i = 0; i < h->n_ion; ++i)
    if (gm[TSFF_P_ION0 + 4 * i + TSFF_ION_A]) return fail(h, -3, "A is not a differentiable leaf (ts_params.py:296)");
  return 0;
}

// a list of n active slots, each in range and named once, as the gradient mask gm[kNP_MAX] (zeroed here), then check_mask
static int check_slots(tsff_handle* h, const int32_t* act, int n, uint8_t* gm, bool m_ok) {
  std::memset(gm, 0, kNP_MAX);
  for (int k = 0; k < n; ++k) {
    const int s = act[k];
    if (s < 0 || s >= h->S.NP) return fail(h, -1, "active slot %d out of range", s);
    if (gm[s]) return fail(h, -1, "active slot %d repeated", s);
    gm[s] = 1;
  }
  return check_mask(h, gm, m_ok);
}

}  // namespace tsff

using namespace tsff;

extern "C" {

int tsff_abi_version(void) { return TSFF_ABI_VERSION; }

const char* tsff_last_error(const tsff_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

const char* tsff_last_launch(const tsff_handle* h) { return h ? h->launched.c_str() : ""; }

int tsff_create(const tsff_config* c, tsff_handle** out) {
  if (!c || !out) return fail(nullptr, -1, "null argument");
  *out = nullptr;
  if (c->abi_version != TSFF_ABI_VERSION) return fail(nullptr, -1, "ABI version mismatch: %d vs %d", c->abi_version, TSFF_ABI_VERSION);
  if (c->npts < TSFF_NBINS || c->npts % TSFF_NBINS) return fail(nullptr, -2, "npts must be a multiple of 1024 (irf.py:74,124), got %d", c->npts);
  if (c->n_ion < 1 || c->n_ion > TSFF_MAX_ION) return fail(nullptr, -2, "n_ion must be 1..%d", TSFF_MAX_ION);
  if (c->n_angles < 1 || c->n_angles > TSFF_MAX_ANGLES) return fail(nullptr, -2, "n_angles must be 1..%d", TSFF_MAX_ANGLES);
  if (c->num_grad_points < 1) return fail(nullptr, -2, "num_grad_points must be >= 1");
  if (c->nvx < 4 || c->nvx > 4096) return fail(nullptr, -2, "nvx out of range");
  if (c->norm != 0) return fail(nullptr, -3, "PhysParams.norm > 0 is not implemented (irf.py:117-122)");
  if (!c->load_ele && !c->load_ion) return fail(nullptr, -2, "neither feature is loaded");
  if (c->load_ele && (c->n_taps_ele < 1 || !c->taps_ele)) return fail(nullptr, -2, "electron IRF taps missing");
  if (c->load_ion && c->n_taps_ion != 0 && (c->n_taps_ion < 1 || !c->taps_ion)) return fail(nullptr, -2, "ion IRF taps missing");
  // spect_stddev_ion == 0 (irf.py:82-86): ThryI = modlI, neither binned nor normalised -- [B, npts] in the reference, which
  // only fits its own [B, 1024] noise and data arrays (thomson_diagnostic.py:139-140) with one point per pixel
  if (c->load_ion && c->n_taps_ion == 0 && c->npts != TSFF_NBINS)
    return fail(nullptr, -2, "spect_stddev_ion == 0 (irf.py:82-86: ThryI = modlI, [npts] samples) needs npts == 1024");
  if (c->fe_mode == TSFF_FE_SHARED && !c->fe_shared) return fail(nullptr, -2, "fe_shared missing");
  if (c->fe_mode == TSFF_FE_DLM && !c->dlm_table) return fail(nullptr, -2, "dlm_table missing");
  if (c->fe_mode != TSFF_FE_SHARED && !c->lg_table) return fail(nullptr, -2, "lg_table missing (needed for per-lineout distribution functions)");
  if (c->fe_mode < 0 || c->fe_mode > 2) return fail(nullptr, -2, "bad fe_mode");
  if (!c->sa_deg || !c->sa_weights || !c->xi1 || !c->xi2 || !c->zprime_re || !c->zprime_im || !c->p_scale || !c->p_shift || !c->p_sigmoid)
    return fail(nullptr, -2, "missing table pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(nullptr, -4, "no HIP device: libtsff has no CPU fallback");

  tsff_handle* h = new tsff_handle();
  h->launched.reserve(1024);
  auto bail = [&](int rc) { g_create_error = h->err; delete h; return rc; };
#define TSFF_HIPC(call)                                                                        \
  do {                                                                                         \
    hipError_t e__ = (call);                                                                   \
    if (e__ != hipSuccess) { fail(h, -5, "%s failed: %s", #call, hipGetErrorString(e__)); return bail(-5); } \
  } while (0)
  TSFF_HIPC(hipGetDevice(&h->device));
  KStatic& S = h->S;
  h->n_ion = c->n_ion;
  h->fe_mode = c->fe_mode;
  S.npts = c->npts; S.ppp = c->npts / TSFF_NBINS; S.n_angles = c->n_angles; S.G = c->num_grad_points;
  S.nvx = c->nvx; S.NP = TSFF_NP(c->n_ion); S.shared_fe = c->fe_mode == TSFF_FE_SHARED;
  S.loss_method = c->loss_method; S.load[0] = c->load_ele; S.load[1] = c->load_ion;
  S.lam_shift[0] = c->ele_lam_shift; S.lam_shift[1] = 0.0;  // generate_spectra.py:90,99
  memcpy(S.ti_same, c->ti_same, sizeof S.ti_same);

  // wavelength axes: linspace like jnp.linspace (form_factor.py:132), omgs (:134), binned axes in nm
  const double* rng[2] = {c->lamrangE, c->lamrangI};
  for (int f = 0; f < 2; ++f) {
    const int n = c->npts;
    std::vector<double> lam(n), om(n), lb(TSFF_NBINS);
    const double step = (rng[f][1] - rng[f][0]) / (double)(n - 1);
    for (int i = 0; i < n; ++i) lam[i] = rng[f][0] + i * step;
    lam[n - 1] = rng[f][1];
    for (int i = 0; i < n; ++i) om[i] = 2e7 * kPi * kC / lam[i];
    for (int p = 0; p < TSFF_NBINS; ++p) {
      double s = 0.0;
      for (int q = 0; q < S.ppp; ++q) {
        // lamAxis = squeeze(2 pi c / omgs) * 1e7 (form_factor.py:293, generate_spectra.py:163,191)
        s += (2.0 * kPi * kC / om[p * S.ppp + q]) * 1e7;
      }
      lb[p] = s / S.ppp;
    }
    TSFF_HIPC(upload(h->omgs[f], om.data(), n));
    TSFF_HIPC(upload(h->lam_bin[f], lb.data(), TSFF_NBINS));
    S.omgs[f] = h->omgs[f].as<double>();
    S.lam_bin[f] = h->lam_bin[f].as<double>();
    h->omgs_host[f] = om;
    (f == 0 ? h->lamE_bin : h->lamI_bin) = lb;
  }
  if (c->ele_filter) { TSFF_HIPC(upload(h->filt, c->ele_filter, c->npts)); S.filt = h->filt.as<double>(); }
  {
    std::vector<double> cs(c->n_angles);
    for (int a = 0; a < c->n_angles; ++a) cs[a] = cos(c->sa_deg[a] * kPi / 180.0);
    TSFF_HIPC(upload(h->cos_sa, cs.data(), cs.size()));
    std::vector<double> sr(c->n_angles);
    for (int a = 0; a < c->n_angles; ++a) sr[a] = c->sa_deg[a] * kPi / 180.0;
    TSFF_HIPC(upload(h->sa_rad, sr.data(), sr.size()));
    S.sa_rad = h->sa_rad.as<double>();
    TSFF_HIPC(upload(h->w_sa, c->sa_weights, c->n_angles));
    S.cos_sa = h->cos_sa.as<double>(); S.w_sa = h->w_sa.as<double>();
  }
  {
    // Z' for xi >= 0 (ion_terms): node j <-> xi2[820 + j]; the node at +8.2 is the mirror of xi2[0] = -8.2.  The table
    // must be even / odd like the shipped one.
    double zmax = 0.0, zasym = 0.0;
    for (int i = 1; i < kNXi2; ++i) {
      zmax = std::max(zmax, std::max(std::fabs(c->zprime_re[i]), std::fabs(c->zprime_im[i])));
      zasym = std::max(zasym, std::max(std::fabs(c->zprime_re[i] - c->zprime_re[kNXi2 - i]),
                                       std::fabs(c->zprime_im[i] + c->zprime_im[kNXi2 - i])));
    }
    if (zasym > 1e-9 * zmax) { h->err = "zprime table is not even (Re) / odd (Im) about xi = 0"; return bail(-1); }
    // The caller's table is even / odd to rounding only (the reference interpolates rdWT / idWT onto arange(-8.2, 8.2, 0.01), whose
    // nodes are not exact mirrors of each other): both device tables are made EXACTLY even / odd from its xi >= 0 half (the
    // odd part an exact 0 at xi = 0), so that the half table and the full one hold the same numbers and a spectrum does not
    // depend on which of them a launch plan uses (ion_terms).  The change to a node is of the order of the table's own
    // interpolation rounding (1e-16 of Z').
    std::vector<double2> zp(kNZh);
    for (int j = 0; j < kNZh - 1; ++j) zp[j] = make_double2(c->zprime_re[kNXi2 / 2 + j], j ? c->zprime_im[kNXi2 / 2 + j] : 0.0);
    zp[kNZh - 1] = make_double2(c->zprime_re[0], -c->zprime_im[0]);
    TSFF_HIPC(upload(h->zp, zp.data(), zp.size()));
    S.zp = h->zp.as<double2>();
    std::vector<double2> zpf(kNXi2);
    for (int i = 0; i < kNXi2; ++i) {
      const int d = i - kNXi2 / 2;
      zpf[i] = d >= 0 ? zp[d] : make_double2(zp[-d].x, -zp[-d].y);
    }
    TSFF_HIPC(upload(h->zpf, zpf.data(), zpf.size()));
    S.zpf = h->zpf.as<double2>();
    TSFF_HIPC(upload(h->xi1, c->xi1, kNXi1));
    TSFF_HIPC(upload(h->xi2, c->xi2, kNXi2));
    S.xi1 = h->xi1.as<double>(); S.xi2 = h->xi2.as<double>();
    double et[kNExpTab];
    for (int j = 0; j < kNExpTab; ++j) et[j] = std::exp2((double)j / kNExpTab);   // (fexp_t)
    TSFF_HIPC(upload(h->etab, et, kNExpTab));
    S.etab = h->etab.as<double>();
  }
  static const double identity_tap[1] = {1.0};
  const bool raw_ion = c->load_ion && c->n_taps_ion == 0;   // no ion IRF: an identity tap, normalisation skipped in the kernels
  S.raw[0] = 0; S.raw[1] = raw_ion ? 1 : 0;
  const int nt[2] = {c->load_ele ? c->n_taps_ele : 0, c->load_ion ? (raw_ion ? 1 : c->n_taps_ion) : 0};
  const int dm[2] = {c->tap_off_ele, raw_ion ? 0 : c->tap_off_ion};
  const double* tp[2] = {c->taps_ele, raw_ion ? identity_tap : c->taps_ion};
  const uint8_t* mk[2] = {c->mask_ele, c->mask_ion};
  S.halo = 0;
  for (int f = 0; f < 2; ++f) {
    if (nt[f] > 0) {
      const int lo = -dm[f], hi = dm[f] + nt[f];  // x index range touched: [p ppp + off, p ppp + off + n)
      S.halo = std::max(S.halo, std::max(lo, hi));
    }
  }
  S.halo = (S.halo + 2) & ~1;  // even: keeps the buffers 16-byte aligned
  S.halo_bins = (S.halo / S.ppp + 3) & ~1;
  // phase-layout convolution (points_per_pixel = 1): taps padded with zeros so that both passes walk them in aligned
  // groups of four -- forward y[p] = sum_u hb[u - toff] x[p + u], adjoint xbar[i] = sum_u hb[-toff - u] ybar[i + u]
  S.hs = 0;
  auto fdiv4 = [](int v) { return v >= 0 ? v / 4 : -((-v + 3) / 4); };
  for (int f = 0; f < 2; ++f) {
    S.ptaps[f] = nullptr;
    S.cf_i0[f] = S.cf_na[f] = S.cf_a0[f] = S.ca_i0[f] = S.ca_na[f] = S.ca_a0[f] = 0;
    if (nt[f] > 0 && S.ppp != 1) {   // points_per_pixel > 1 (k_spectrum_rows): kTapPad zeros on both sides, so that groups of ppp
      std::vector<double> pt(nt[f] + 2 * kTapPad, 0.0);   // consecutive taps starting anywhere in (-ppp, n) are read without range checks
      for (int k = 0; k < nt[f]; ++k) pt[kTapPad + k] = tp[f][k];
      TSFF_HIPC(upload(h->ptaps[f], pt.data(), pt.size()));
      S.ptaps[f] = h->ptaps[f].as<double>();
    }
    if (nt[f] <= 0 || S.ppp != 1) continue;
    const int n = nt[f], toff = dm[f];
    const int u0f = 4 * fdiv4(toff), pre = toff - u0f;
    S.cf_a0[f] = u0f / 4; S.cf_na[f] = (pre + n + 3) / 4; S.cf_i0[f] = 3 - pre;
    const int uamin = -toff - n + 1, u0a = 4 * fdiv4(uamin), prea = uamin - u0a;
    S.ca_a0[f] = u0a / 4; S.ca_na[f] = (prea + n + 3) / 4; S.ca_i0[f] = 3 + n - 1 + prea;
    // (kTapLead zeros in front of entry 0 and 13 behind the last tap: the pipelined convolution reads two groups beyond its last
    //  one in either direction, entries -kTapLead .. n + 13 -- conv4_phase shows the index arithmetic)
    std::vector<double> pt(kTapLead + n + 16, 0.0);
    for (int k = 0; k < n; ++k) pt[kTapLead + 3 + k] = tp[f][k];
    TSFF_HIPC(upload(h->ptaps[f], pt.data(), pt.size()));
    S.ptaps[f] = h->ptaps[f].as<double>() + kTapLead;
    S.hs = std::max(S.hs, std::max(std::max(-S.cf_a0[f], S.cf_a0[f] + S.cf_na[f]), std::max(-S.ca_a0[f], S.ca_a0[f] + S.ca_na[f])) + 1);
  }
  for (int f = 0; f < 2; ++f) {
    S.ntaps[f] = nt[f]; S.toff[f] = dm[f];
    TSFF_HIPC(upload(h->taps[f], tp[f], nt[f]));
    S.taps[f] = h->taps[f].as<double>();
    std::vector<uint8_t> m(TSFF_NBINS, 0);
    if (mk[f]) memcpy(m.data(), mk[f], TSFF_NBINS);
    TSFF_HIPC(upload(h->mask[f], m.data(), m.size()));
    S.mask[f] = h->mask[f].as<uint8_t>();
  }
  TSFF_HIPC(upload(h->p_scale, c->p_scale, S.NP));
  TSFF_HIPC(upload(h->p_shift, c->p_shift, S.NP));
  TSFF_HIPC(upload(h->p_sig, c->p_sigmoid, S.NP));
  S.p_scale = h->p_scale.as<double>(); S.p_shift = h->p_shift.as<double>(); S.p_sig = h->p_sig.as<uint8_t>();
  TSFF_HIPC(h->gmask.ensure(kNP_MAX));
  if (c->fe_mode == TSFF_FE_DLM) {
    TSFF_HIPC(upload(h->dlm, c->dlm_table, (size_t)c->nvx * TSFF_DLM_NM));
    S.dlm_table = h->dlm.as<double>();
  }
  if (c->fe_mode != TSFF_FE_SHARED) {
    TSFF_HIPC(upload(h->lg, c->lg_table, (size_t)kNXi2 * kNXi1));
    S.lg = h->lg.as<double>();
  }
  {  // vx = linspace(-6 + dv/2, 6 - dv/2, nvx)   (base.py:149-151)
    const double vmax = 6.0, dv = 2.0 * vmax / c->nvx;
    const double v0 = -vmax + dv / 2, v1 = vmax - dv / 2;
    S.vx0 = v0; S.dv = (v1 - v0) / (double)(c->nvx - 1);
    // K window of k_wgemm: ratdf[i] = gradient(exp(H(xi1)))[i] can be non-zero only if one of xi1[i-1 .. i+1] lies inside the vx
    // grid [v0, v1] (H = -50 outside), and X rows i use ratdf[i], ratdf[i+1]: keep i with xi1[i-1 .. i+2] touching the grid,
    // one more on each side for safety, rounded outwards to multiples of the K chunk
    int lo = kNXi1, hi = 0;
    for (int i = 0; i < kNXi1; ++i)
      if (c->xi1[i] >= v0 && c->xi1[i] <= v1) { lo = std::min(lo, i); hi = std::max(hi, i); }
    if (lo <= hi) {
      h->kw_lo = std::max(0, lo - 3) / kGK * kGK;
      h->kw_hi = std::min((int)kNXi1, (hi + 4 + kGK - 1) / kGK * kGK);
    }
  }
  h->smem_spectrum = sizeof(double) * smem_doubles(S, 1, 0, false);  // k_form_factor
  if (sizeof(double) * smem_doubles(S, 1, c->fe_mode == TSFF_FE_DLM ? 1 : 0, false) > kLdsLimit) {
    fail(h, TSFF_ERR_LDS, "LDS budget exceeded (%zu B for one feature): reduce npts or the IRF cutoff",
         sizeof(double) * smem_doubles(S, 1, c->fe_mode == TSFF_FE_DLM ? 1 : 0, false));
    return bail(TSFF_ERR_LDS);
  }
  h->smem_prepare = sizeof(double) * (2 * (size_t)S.nvx + 3 * kNXi1 + 8) + sizeof(double2) * S.nvx;
  h->smem_vectors = sizeof(double2) * 6 * (size_t)S.nvx + sizeof(double) * (2 * (size_t)S.nvx + 4 * kNXi1 + 8);
  h->smem_adjoint = sizeof(double2) * 3 * (size_t)S.nvx + sizeof(double) * (2 * (size_t)S.nvx + 4 * kNXi1 + 8);
  TSFF_HIPC(raise_lds_limits(c->n_ion));
  // shared distribution function: build its tables once
  TSFF_HIPC(h->ht.ensure((size_t)S.nvx * sizeof(double2)));
  TSFF_HIPC(h->W.ensure((size_t)kNXi2 * sizeof(double)));
  if (c->fe_mode == TSFF_FE_SHARED) {
    DevBuf fe;
    TSFF_HIPC(upload(fe, c->fe_shared, c->nvx));
    int rc = launch_prepare(h, fe.as<double>(), TSFF_FE_SHARED, nullptr, 1, h->ht.as<double2>(), h->W.as<double>(), nullptr);
    if (rc) return bail(rc);
    TSFF_HIPC(hipStreamSynchronize(h->stream));
  }
  // (tsff_set_stream; it only orders streams of this device: a device-scope release, no system-wide cache write-back per call)
  TSFF_HIPC(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming | hipEventReleaseToDevice));
#undef TSFF_HIPC
  *out = h;
  return 0;
}

void tsff_destroy(tsff_handle* h) {
  if (!h) return;
  DevGuard dg__(h, false);
  if (h->ev_switch) (void)hipEventDestroy(h->ev_switch);
  for (auto e : h->ev0) (void)hipEventDestroy(e);
  for (auto e : h->ev1) (void)hipEventDestroy(e);
  for (auto e : h->blk_ev) (void)hipEventDestroy(e);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->aux) { (void)hipStreamSynchronize(h->aux); (void)hipStreamDestroy(h->aux); }
  delete h;
}

int tsff_set_stream(tsff_handle* h, void* s) {
  if (!h) return -1;
  const hipStream_t ns = reinterpret_cast<hipStream_t>(s);
  if (ns == h->stream) return 0;
  // the handle's scratch (tables, records, row scratch, partial sums) is shared by its calls: work a call left on the old stream
  // must finish before the new stream's first call rewrites it -- the new stream waits on an event recorded on the old one, once
  // per switch (recording one at the end of every call instead, which would let the old stream die first, costs the one-stream
  // hot path 0.6 %).  So the old stream must still exist (tsff.h); a stream that is capturing a graph does not take part (ordering
  // is then the caller's)
  if (h->enqueued) {
    DevGuard dg__(h, false);
    hipStreamCaptureStatus a = hipStreamCaptureStatusNone, b = hipStreamCaptureStatusNone;
    TSFF_HIP(h, hipStreamIsCapturing(h->stream, &a));
    TSFF_HIP(h, hipStreamIsCapturing(ns, &b));
    if (a == hipStreamCaptureStatusNone && b == hipStreamCaptureStatusNone) {
      TSFF_HIP(h, hipEventRecord(h->ev_switch, h->stream));
      TSFF_HIP(h, hipStreamWaitEvent(ns, h->ev_switch, 0));
    }
    h->enqueued = false;
  }
  h->stream = ns;
  return 0;
}

int tsff_set_option(tsff_handle* h, int32_t key, int32_t value) {
  if (!h) return -1;
  if (key == TSFF_OPT_LAUNCH_PLAN) {
    if (value < 0 || (value & ~kPlanBits)) return fail(h, -2, "TSFF_OPT_LAUNCH_PLAN is a bit mask: 1 never interleave the features, 2 never use the one-sweep kernel, 4 never three forward workgroups per CU, 8 no base-point exchange in the one-sweep kernel, 32 the 128 x 128 tiling of the W-table GEMM, 64 one workgroup per CU (measurements), 256 never the pair-sweep forward kernel");
    h->plan = value;
    return 0;
  }
  if (key == TSFF_OPT_DENOM_MODE) {
    if (value != 0 && value != 2) return fail(h, -2, "TSFF_OPT_DENOM_MODE must be 0 (constant) or 2 (|data| + 1e-10)");
    h->denom_mode = value;
    return 0;
  }
  if (key == TSFF_OPT_DLM_BLOCKS) {
    if (value < 0 || value > 64) return fail(h, -2, "TSFF_OPT_DLM_BLOCKS must be 0 / 1 (off) or the number of column blocks (<= 64)");
    h->dlm_blocks = value;
    return 0;
  }
  return fail(h, -2, "unknown option %d", key);
}

int tsff_reserve(tsff_handle* h, int32_t B) {
  DevGuard dg__(h);
  if (!h || B < 1) return -1;
  return ensure_workspace(h, B, true);
}

int tsff_get_axes(const tsff_handle* h, double* lamE, double* lamI) {
  if (!h) return -1;
  if (lamE) memcpy(lamE, h->lamE_bin.data(), TSFF_NBINS * sizeof(double));
  if (lamI) memcpy(lamI, h->lamI_bin.data(), TSFF_NBINS * sizeof(double));
  return 0;
}

int tsff_enable_timing(tsff_handle* h, int32_t ring) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (ring < 0 || ring > 65536) return fail(h, -2, "timing ring size out of range");
  h->timing = ring > 0;
  h->ev_count = 0;
  while ((int)h->ev0.size() < ring) {
    hipEvent_t a, b;
    TSFF_HIP(h, hipEventCreate(&a));
    TSFF_HIP(h, hipEventCreate(&b));
    h->ev0.push_back(a);
    h->ev1.push_back(b);
  }
  return 0;
}

int tsff_kernel_times(tsff_handle* h, float* ms, int32_t max_n, int32_t* n_out) {
  DevGuard dg__(h);
  if (!h || !ms || !n_out) return -1;
  const size_t ring = h->ev0.size();
  size_t n = h->ev_count < ring ? h->ev_count : ring;
  if ((size_t)max_n < n) n = max_n;
  for (size_t i = 0; i < n; ++i) {
    const size_t slot = (h->ev_count - n + i) % ring;
    TSFF_HIP(h, hipEventSynchronize(h->ev1[slot]));
    TSFF_HIP(h, hipEventElapsedTime(&ms[i], h->ev0[slot], h->ev1[slot]));
  }
  *n_out = (int32_t)n;
  return 0;
}

static int fp64_peak(tsff_handle* h, bool mfma, double* tflops);
int tsff_fp64_fma_peak(tsff_handle* h, double* tflops) { return fp64_peak(h, false, tflops); }
int tsff_fp64_mfma_peak(tsff_handle* h, double* tflops) { return fp64_peak(h, true, tflops); }
static int fp64_peak(tsff_handle* h, bool mfma, double* tflops) {
  if (!h || !tflops) return -1;
  DevGuard dg__(h);
  const int blocks = 256 * 8, iters = 4096, reps = 5;
  DevBuf out;
  TSFF_HIP(h, out.ensure((size_t)blocks * kThreads * sizeof(double)));
  hipEvent_t e0, e1;
  TSFF_HIP(h, hipEventCreate(&e0));
  TSFF_HIP(h, hipEventCreate(&e1));
  float best = 1e30f;
  for (int r = 0; r < reps + 1; ++r) {
    TSFF_HIP(h, hipEventRecord(e0, h->stream));
    if (mfma) TSFF_LAUNCH0(h, k_mfma_peak, dim3(blocks), dim3(kThreads), 0, h->stream, out.as<double>(), iters / 4, 0.999999, 1e-7);
    else TSFF_LAUNCH0(h, k_fma_peak, dim3(blocks), dim3(kThreads), 0, h->stream, out.as<double>(), iters, 0.999999, 1e-7);
    TSFF_HIP(h, hipEventRecord(e1, h->stream));
    TSFF_HIP(h, hipEventSynchronize(e1));
    float ms = 0.f;
    TSFF_HIP(h, hipEventElapsedTime(&ms, e0, e1));
    if (r > 0 && ms < best) best = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  const double flop = mfma ? 2048.0 * 8.0 * (double)(iters / 4) * (double)blocks * (kThreads / 64)
                           : 2.0 * 16.0 * (double)iters * (double)blocks * kThreads;
  *tflops = flop / (best * 1e-3) / 1e12;
  return 0;
}

int tsff_l1_read_peak(tsff_handle* h, double* tbps) {
  if (!h || !tbps) return -1;
  DevGuard dg__(h);
  const int blocks = h->ncu2d() * 8, iters = 2048, reps = 5;
  DevBuf src, out;
  TSFF_HIP(h, src.ensure(1024 * sizeof(double2)));
  TSFF_HIP(h, hipMemsetAsync(src.p, 0, 1024 * sizeof(double2), h->stream));
  TSFF_HIP(h, out.ensure((size_t)blocks * kThreads * sizeof(double)));
  hipEvent_t e0, e1;
  TSFF_HIP(h, hipEventCreate(&e0));
  TSFF_HIP(h, hipEventCreate(&e1));
  float best = 1e30f;
  for (int r = 0; r < reps + 1; ++r) {
    TSFF_HIP(h, hipEventRecord(e0, h->stream));
    TSFF_LAUNCH0(h, k_l1_peak, dim3(blocks), dim3(kThreads), 0, h->stream, src.as<double2>(), out.as<double>(), iters);
    TSFF_HIP(h, hipEventRecord(e1, h->stream));
    TSFF_HIP(h, hipEventSynchronize(e1));
    float ms = 0.f;
    TSFF_HIP(h, hipEventElapsedTime(&ms, e0, e1));
    if (r > 0 && ms < best) best = ms;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *tbps = (double)blocks * kThreads * (double)iters * 8.0 * 16.0 / (best * 1e-3) / 1e12;
  return 0;
}

int tsff_chi_table(tsff_handle* h, const double* fe, int32_t n, double* W) {
  DevGuard dg__(h);
  if (!h || !fe || !W || n < 1) return fail(h, -1, "bad argument");
  DevBuf ht;
  TSFF_HIP(h, ht.ensure((size_t)n * h->S.nvx * sizeof(double2)));
  int rc = launch_prepare(h, fe, TSFF_FE_PER_LINEOUT, nullptr, n, ht.as<double2>(), W, nullptr);
  if (rc) return rc;
  TSFF_HIP(h, hipStreamSynchronize(h->stream));  // ht is freed on return
  return 0;
}

// The form-factor, 2-D and ATS paths below have the shape of the loss + gradient path (loss_grad_prepare / loss_grad_enqueue).
// A plan struct holds what the launches of a path need.  X_prepare takes the shapes of a call: it refuses what they rule out
// (a point range, an LDS budget), then sizes every buffer of the path -- when it returns non-zero, nothing has been enqueued.
// X_enqueue takes the plan and the call's pointers and only launches (kernels, memsets, the timing ring's events): it allocates
// and refuses nothing, only a HIP error can fail it.  An entry point is its own argument checks + prepare + enqueue;
// tsff_angular_fit prepares its stages once and enqueues them every epoch.  dry: the refusals only, the handle stays as it is
// (tsff_angular_fit asks for every stage's refusals before it allocates anything).

// The tail of the f_e adjoint (tsff_form_factor_grad, tsff_loss_grad_fe): `lead` blocks [B][.] of table adjoints in Wb and Hys,
// which the caller sums into the first block (k_sum_chunks / k_add_parts), then Yt = Lg^T Wb (k_wgemm_t) and k_fe_adjoint
static int fe_tail_prepare(tsff_handle* h, size_t lead, int B) {
  TSFF_ENSURE(h, h->Wb, lead * B * kNXi2 * sizeof(double));
  TSFF_ENSURE(h, h->Hys, lead * B * 2 * h->S.nvx * sizeof(double));
  TSFF_ENSURE(h, h->Yt, (size_t)B * 2 * kNXi1 * sizeof(double));
  return 0;
}
static void fe_tail_outputs(tsff_handle* h, KCall& K, int B) {
  K.Wb_out = h->Wb.as<double>();
  K.Hy_out = h->Hys.as<double>();
  K.Hs_out = K.Hy_out + (size_t)B * h->S.nvx;
  K.htm = nullptr; K.Wm = nullptr;  // the LDS region of the tangent tables holds the table adjoints
}
static int fe_tail_enqueue(tsff_handle* h, const KCall& K, int B, double* grad_fe) {
  dim3 ggrid(kNXi1 / kGN, (2 * B + kGM - 1) / kGM);
  TSFF_LAUNCH0(h, k_wgemm_t, ggrid, dim3(kThreads), 0, h->stream, h->S.lg, K.Wb_out, h->S.xi2, (int)B, h->Yt.as<double>());
  TSFF_HIP(h, hipGetLastError());
  TSFF_LAUNCH0(h, k_fe_adjoint, dim3(B), dim3(kThreads), h->smem_adjoint, h->stream, h->S, K.ht, h->Yt.as<double>(),
                     K.Wb_out, K.Hy_out, K.Hs_out, grad_fe);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// ---- the 1-D form factor
struct FormFactorPlan {
  int feature = 0, B = 0;
  dim3 grid;
};

static int form_factor_prepare(tsff_handle* h, int feature, int B, FormFactorPlan& p, bool dry = false) {
  p.feature = feature; p.B = B;
  p.grid = dim3(B, angle_chunks(h, B));
  return dry ? 0 : ensure_workspace(h, B);
}

static int form_factor_enqueue(tsff_handle* h, const FormFactorPlan& p, const double* phys, const double* fe, double* P) {
  KCall K{};
  K.params = phys; K.B = p.B;
  if (int rc = prepare_tables(h, phys, fe, p.B, K)) return rc;
  TSFF_LAUNCH_FN(h, form_factor_kernel(h->n_ion), ("k_form_factor", h->n_ion), p.grid, dim3(kThreads), h->smem_spectrum, h->stream, h->S, K,
                 p.feature, h->S.omgs[p.feature], h->S.npts, P);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

int tsff_form_factor(tsff_handle* h, int32_t feature, const double* phys, const double* fe, int32_t B, double* P) {
  DevGuard dg__(h);
  if (!h || !phys || !P || B < 1 || feature < 0 || feature > 1) return fail(h, -1, "bad argument");
  if (h->fe_mode == TSFF_FE_DLM) return fail(h, -3, "tsff_form_factor takes explicit distribution functions (fe_mode SHARED or PER_LINEOUT)");
  FormFactorPlan p;
  int rc = check_fe(h, fe);
  if (!rc) rc = form_factor_prepare(h, feature, B, p);
  if (rc) return rc;
  return form_factor_enqueue(h, p, phys, fe, P);
}

// ---- its adjoint (grad_fe: with the f_e adjoint)
struct FormFactorAdjPlan {
  int feature = 0, B = 0;
  bool grad_fe = false;
  size_t smem = 0;                    // LDS of k_form_factor_adj
  unsigned nchunk = 1; int nworker = 0;   // angle chunks (blockIdx.y); partials of the lineout-scalar adjoints: one per wavefront
};                                        // and angle chunk (every slot is written)

static int form_factor_adj_prepare(tsff_handle* h, int feature, int B, bool grad_fe, FormFactorAdjPlan& p, bool dry = false) {
  p.feature = feature; p.B = B; p.grad_fe = grad_fe;
  p.smem = sizeof(double) * smem_doubles(h->S, 1, grad_fe ? 2 : 0, false);
  if (p.smem > kLdsLimit) return fail(h, TSFF_ERR_LDS, "LDS budget exceeded (%zu B)", p.smem);
  p.nchunk = angle_chunks(h, B);
  p.nworker = (int)p.nchunk * (kThreads / 64);
  if (dry) return 0;
  if (int rc = ensure_workspace(h, B)) return rc;
  const int NLB = 9 + 3 * h->n_ion;
  TSFF_ENSURE(h, h->lbacc, (size_t)B * h->S.G * NLB * sizeof(double));
  TSFF_ENSURE(h, h->lbparts, (size_t)B * h->S.G * p.nworker * NLB * sizeof(double));
  return grad_fe ? fe_tail_prepare(h, p.nchunk, B) : 0;   // per-chunk blocks [chunk][B][.], summed in order by k_sum_chunks
}

static int form_factor_adj_enqueue(tsff_handle* h, const FormFactorAdjPlan& p, const double* phys, const double* fe, const double* Pbar,
                                   double* grad_phys, double* grad_fe) {
  const int B = p.B, NLB = 9 + 3 * h->n_ion;
  KCall K{};
  K.params = phys; K.B = B;
  int rc = prepare_tables(h, phys, fe, B, K);
  if (rc) return rc;
  if (p.grad_fe) fe_tail_outputs(h, K, B);
  dim3 grid(B, p.nchunk), block(kThreads);
  TSFF_LAUNCH_FN(h, form_factor_adj_kernel(h->n_ion, p.grad_fe), ("k_form_factor_adj", h->n_ion, p.grad_fe ? 2 : 0), grid, block, p.smem,
                 h->stream, h->S, K, p.feature, h->S.omgs[p.feature], h->S.npts, Pbar, h->lbparts.as<double>());
  TSFF_LAUNCH0(h, k_lbacc_reduce, dim3(B * h->S.G), dim3(kThreads), 0, h->stream, h->lbparts.as<double>(), p.nworker, NLB,
               h->lbacc.as<double>());
  TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_ff2d_lines_adj, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->S, phys, p.feature, B,
                  h->lbacc.as<double>(), grad_phys, 1);
  TSFF_HIP(h, hipGetLastError());
  if (!p.grad_fe) return 0;
  if (p.nchunk > 1) {
    const long nw = (long)B * kNXi2, nh = (long)2 * B * h->S.nvx;
    TSFF_LAUNCH0(h, k_sum_chunks, dim3((unsigned)std::min<long>((nw + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0, h->stream,
                       K.Wb_out, nw, (int)p.nchunk);
    TSFF_LAUNCH0(h, k_sum_chunks, dim3((unsigned)std::min<long>((nh + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0, h->stream,
                       K.Hy_out, nh, (int)p.nchunk);
  }
  return fe_tail_enqueue(h, K, B, grad_fe);
}

int tsff_form_factor_grad(tsff_handle* h, int32_t feature, const double* phys, const double* fe, int32_t B, const double* Pbar,
                          double* grad_phys, double* grad_fe) {
  DevGuard dg__(h);
  if (!h || !phys || !Pbar || !grad_phys || B < 1 || feature < 0 || feature > 1) return fail(h, -1, "bad argument");
  if (h->fe_mode == TSFF_FE_DLM) return fail(h, -3, "tsff_form_factor_grad takes explicit distribution functions (fe_mode SHARED or PER_LINEOUT)");
  if (grad_fe && h->fe_mode != TSFF_FE_PER_LINEOUT) return fail(h, -2, "gradient w.r.t. f_e needs fe_mode == TSFF_FE_PER_LINEOUT");
  FormFactorAdjPlan p;
  int rc = check_fe(h, fe);
  if (!rc) rc = form_factor_adj_prepare(h, feature, B, grad_fe != nullptr, p);
  if (rc) return rc;
  return form_factor_adj_enqueue(h, p, phys, fe, Pbar, grad_phys, grad_fe);
}

// ---- its forward mode: groups of kFfjvpW directions per launch, the table tangents built for a block of directions at a time
constexpr int kFfjvpW = 3;
struct FormFactorJvpPlan {
  int feature = 0, B = 0, n_dir = 0;
  bool tab = false;        // fe_dot given: every lane of a group carries a table direction
  int gw = kFfjvpW;        // directions per group (1: the LDS holds one table lane only)
  int dblk = 0;            // directions whose table tangents are built at once (a multiple of gw)
  size_t smem = 0;
  dim3 grid;
};

static int form_factor_jvp_prepare(tsff_handle* h, int feature, int B, int n_dir, bool tab, FormFactorJvpPlan& p) {
  p.feature = feature; p.B = B; p.n_dir = n_dir; p.tab = tab;
  p.gw = kFfjvpW;
  p.smem = sizeof(double) * ffjvp_smem_doubles(h->S, tab ? kFfjvpW : 0, kFfjvpW);
  if (p.smem > kLdsLimit && tab) {   // one table lane per group before giving up
    p.gw = 1;
    p.smem = sizeof(double) * ffjvp_smem_doubles(h->S, 1, kFfjvpW);
  }
  if (p.smem > kLdsLimit)
    return fail(h, -2, "tsff_form_factor_jvp: LDS budget exceeded (%zu B with nvx = %d, %d angles%s): reduce nvx", p.smem, h->S.nvx,
                h->S.n_angles, tab ? " and one table direction per group" : "");
  p.grid = dim3(B, angle_chunks(h, B));
  // (blocks of about 384 table rows: 12 MB of GEMM input, a grid of the GEMM that fills the device)
  const int want = std::max(1, 384 / std::max(B, 1));
  p.dblk = std::min(std::max(p.gw, want / p.gw * p.gw), (n_dir + p.gw - 1) / p.gw * p.gw);
  if (int rc = ensure_workspace(h, B)) return rc;
  if (tab) {
    const size_t rows = (size_t)std::min(p.dblk, n_dir) * B;
    TSFF_ENSURE(h, h->jv_htd, rows * h->S.nvx * sizeof(double2));
    TSFF_ENSURE(h, h->jv_X, rows * 4 * kNXi1 * sizeof(double));
    TSFF_ENSURE(h, h->jv_cst, rows * 2 * sizeof(double));
    TSFF_ENSURE(h, h->jv_Wd, rows * kNXi2 * sizeof(double));
  }
  return 0;
}

static int form_factor_jvp_enqueue(tsff_handle* h, const FormFactorJvpPlan& p, const double* phys, const double* fe, const double* phys_dot,
                                   const double* fe_dot, double* P, double* P_dot) {
  const int B = p.B;
  const size_t nvx = h->S.nvx;
  if (int rc = timing_begin(h)) return rc;
  KCall K{};
  K.params = phys; K.B = B;
  if (int rc = prepare_tables(h, phys, fe, B, K)) return rc;
  if (P) {   // the value by the shipped forward: tsff_form_factor's bit for bit
    TSFF_LAUNCH_FN(h, form_factor_kernel(h->n_ion), ("k_form_factor", h->n_ion), p.grid, dim3(kThreads), h->smem_spectrum, h->stream, h->S, K,
                   p.feature, h->S.omgs[p.feature], h->S.npts, P);
    TSFF_HIP(h, hipGetLastError());
  }
  for (int d0 = 0; d0 < p.n_dir; d0 += p.dblk) {
    const int nb = std::min(p.dblk, p.n_dir - d0), rows = nb * B;
    if (p.tab) {
      TSFF_LAUNCH0(h, k_fe_direction, dim3(rows), dim3(kThreads), h->smem_vectors, h->stream, h->S, fe, fe_dot + (size_t)d0 * B * nvx, K.ht, B,
                   h->jv_htd.as<double2>(), h->jv_X.as<double>(), h->jv_cst.as<double>());
      const int nM = (rows + kGM / 2 - 1) / (kGM / 2), nQ = (kNXi2 + kGN - 1) / kGN;
      TSFF_LAUNCH(h, k_wgemm, (2), dim3(8 * ((nM + 7) / 8) * nQ), dim3(kThreads), 0, h->stream, h->S.lg, h->jv_X.as<double>(),
                  h->jv_cst.as<double>(), h->S.xi2, rows, h->jv_Wd.as<double>(), (double*)nullptr, h->kw_lo, h->kw_hi);
      TSFF_HIP(h, hipGetLastError());
    }
    for (int g0 = 0; g0 < nb; g0 += p.gw) {
      FfjvpArgs A{};
      A.d0 = d0 + g0; A.nd = std::min(p.gw, nb - g0);
      A.nlane = p.tab ? A.nd : 0;
      A.phys_dot = phys_dot;
      A.htd = p.tab ? h->jv_htd.as<double2>() + (size_t)g0 * B * nvx : nullptr;
      A.Wd = p.tab ? h->jv_Wd.as<double>() + (size_t)g0 * B * kNXi2 : nullptr;
      A.P_dot = P_dot;
      // (the LDS is carved for the lanes of this group: a last partial group asks for less than the plan's budget)
      const size_t smem = sizeof(double) * ffjvp_smem_doubles(h->S, A.nlane, kFfjvpW);
      TSFF_LAUNCH_FN(h, ffjvp_kernel(h->n_ion), ("k_ffjvp", h->n_ion, kFfjvpW), p.grid, dim3(kThreads), smem, h->stream, h->S, K, A, p.feature,
                     h->S.omgs[p.feature], h->S.npts);
    }
    TSFF_HIP(h, hipGetLastError());
  }
  return timing_end(h);
}

int tsff_form_factor_jvp(tsff_handle* h, int32_t feature, const double* phys, const double* fe, int32_t B, int32_t n_dir,
                         const double* phys_dot, const double* fe_dot, double* P, double* P_dot) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!phys || !phys_dot || !P_dot || B < 1 || n_dir < 1 || feature < 0 || feature > 1) return fail(h, -1, "bad argument");
  if (h->fe_mode == TSFF_FE_DLM) return fail(h, -3, "tsff_form_factor_jvp takes explicit distribution functions (fe_mode SHARED or PER_LINEOUT)");
  if (fe_dot && h->fe_mode != TSFF_FE_PER_LINEOUT) return fail(h, -2, "a direction of f_e needs fe_mode == TSFF_FE_PER_LINEOUT");
  FormFactorJvpPlan p;
  int rc = check_fe(h, fe);
  if (!rc) rc = form_factor_jvp_prepare(h, feature, B, n_dir, fe_dot != nullptr, p);
  if (rc) return rc;
  return form_factor_jvp_enqueue(h, p, phys, fe, phys_dot, fe_dot, P, P_dot);
}

// ---- the 2-D form factor (save: with the projection records of its points for the adjoint that follows)
struct FormFactor2dPlan {
  int feature = 0, nv = 0, B = 0;
  bool shared = true, save = false;
  long begin = 0, end = 0;          // the points [begin, end) of the flat point list (empty: nothing to launch)
  bool lds = false; int groups = 0; // the table fits LDS (nv <= 128; else read through L1/L2 from a padded copy); point groups per workgroup
  size_t smem = 0, tstride = 0;     // dynamic LDS; doubles from one lineout's table to the next
  long max_grid = 0;                // persistent workgroups of groups x 256 threads: one per CU with the table in LDS
};

// any 2-D forward invalidates the projection records of an earlier save, and their token
static void invalidate_proj(tsff_handle* h) {
  h->proj_rec.invalidate();
  h->proj_token = 0;
}

static int form_factor_2d_prepare(tsff_handle* h, int feature, int nv, bool shared, int B, int64_t point_begin, int64_t point_end,
                                  bool save, FormFactor2dPlan& p, bool dry = false) {
  p.feature = feature; p.nv = nv; p.B = B; p.shared = shared; p.save = save;
  const long ntotal = (long)B * h->S.G * h->S.npts * h->S.n_angles;
  p.begin = point_begin; p.end = point_end < 0 ? ntotal : point_end;
  if (p.begin < 0 || p.end > ntotal || p.begin > p.end) return fail(h, -1, "bad point range");
  if (!dry) invalidate_proj(h);
  if (p.begin == p.end) return 0;
  constexpr int kGL = TSFF_2D_GROUPS_LDS, kGG = TSFF_2D_GROUPS_L2;
  p.lds = sizeof(double) * smem2d_doubles(nv, true, kGL) <= kLdsLimit;
  p.groups = p.lds ? kGL : kGG;
  p.smem = sizeof(double) * smem2d_doubles(nv, p.lds, p.groups);
  if (p.smem > kLdsLimit) return fail(h, -2, "nv = %d needs %zu B of LDS scratch", nv, p.smem);
  p.max_grid = (long)h->ncu2d() * (p.lds ? 1 : 8);  // (the L2 variant is register-limited to two workgroups per CU)
  p.tstride = p.lds ? (size_t)nv * nv : pad2d_doubles(nv);
  if (dry) return 0;
  if (!p.lds) TSFF_ENSURE(h, h->fpad, p.tstride * (shared ? 1 : B) * sizeof(double));
  if (save) TSFF_ENSURE(h, h->proj, (size_t)(p.end - p.begin) * proj2d_doubles(nv) * sizeof(double));
  return 0;
}

static int form_factor_2d_enqueue(tsff_handle* h, const FormFactor2dPlan& p, const double* phys, const double* fe2d, double ud_angle_deg,
                                  double va_angle_deg, double* P) {
  if (p.begin == p.end) return 0;
  const long per_lineout = (long)h->S.G * h->S.npts * h->S.n_angles;
  // one table per launch: a shared table covers the whole range, per-lineout tables one launch per lineout
  const int b_first = p.shared ? 0 : (int)(p.begin / per_lineout), b_last = p.shared ? 0 : (int)((p.end - 1) / per_lineout);
  const double* tables = fe2d;
  if (!p.lds) {   // ghost cells by k_pad2d
    TSFF_LAUNCH0(h, k_pad2d, dim3(p.shared ? 1 : p.B), dim3(kThreads), 0, h->stream, fe2d, p.nv, h->fpad.as<double>());
    TSFF_HIP(h, hipGetLastError());
    tables = h->fpad.as<double>() + pad2d_margin(p.nv);   // (the padded table behind its leading margin; per-lineout tables tstride apart)
  }
  double* proj = nullptr;
  if (p.save) {
    proj = h->proj.as<double>();
    h->proj_rec = {p.begin, p.end, p.nv, p.feature, p.B, phys, fe2d, ud_angle_deg, va_angle_deg};
  }
  for (int b = b_first; b <= b_last; ++b) {
    const long lo = p.shared ? p.begin : std::max(p.begin, (long)b * per_lineout);
    const long hi = p.shared ? p.end : std::min(p.end, (long)(b + 1) * per_lineout);
    const double* table = tables + (p.shared ? 0 : (size_t)b * p.tstride);
    dim3 grid((unsigned)std::min((hi - lo + p.groups - 1) / p.groups, p.max_grid)), block(p.groups * kThreads);
    if (int rc = timing_begin(h)) return rc;
    TSFF_LAUNCH_FN(h, form_factor_2d_kernel(h->n_ion, p.lds, p.save), ("k_form_factor_2d", h->n_ion, p.lds, p.groups, p.save), grid, block,
                   p.smem, h->stream, h->S, phys, table, p.nv, ud_angle_deg * kPi / 180.0, va_angle_deg * kPi / 180.0, p.feature, lo, hi, P,
                   proj);
    TSFF_HIP(h, hipGetLastError());
    if (int rc = timing_end(h)) return rc;
  }
  return 0;
}

static int form_factor_2d(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv, int32_t shared_fe,
                          double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin, int64_t point_end, double* P,
                          bool save) {
  if (!h || !phys || !fe2d || !P || B < 1 || feature < 0 || feature > 1 || nv < 4 || nv > 2048)
    return fail(h, -1, "bad argument");
  FormFactor2dPlan p;
  if (int rc = form_factor_2d_prepare(h, feature, nv, shared_fe != 0, B, point_begin, point_end, save, p)) return rc;
  return form_factor_2d_enqueue(h, p, phys, fe2d, ud_angle_deg, va_angle_deg, P);
}

int tsff_form_factor_2d_range(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv,
                              int32_t shared_fe, double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin,
                              int64_t point_end, double* P) {
  DevGuard dg__(h);
  return form_factor_2d(h, feature, phys, fe2d, nv, shared_fe, ud_angle_deg, va_angle_deg, B, point_begin, point_end, P, false);
}

int tsff_form_factor_2d(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv,
                        int32_t shared_fe, double ud_angle_deg, double va_angle_deg, int32_t B, double* P) {
  return tsff_form_factor_2d_range(h, feature, phys, fe2d, nv, shared_fe, ud_angle_deg, va_angle_deg, B, 0, -1, P);
}

int tsff_form_factor_2d_save(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv,
                             double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin, int64_t point_end,
                             double* P, uint64_t* token) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!token) return fail(h, -1, "tsff_form_factor_2d_save: token missing");
  *token = 0;
  if (nv > 256) return fail(h, -2, "tsff_form_factor_2d_save: nv <= 256");
  const int rc = form_factor_2d(h, feature, phys, fe2d, nv, 1, ud_angle_deg, va_angle_deg, B, point_begin, point_end, P, true);
  if (rc) return rc;
  // generation token: a per-handle call counter mixed with what the records were made from (buffers, angles, range) -- never 0
  auto mix = [](uint64_t a, uint64_t b) { a ^= b + 0x9e3779b97f4a7c15ull + (a << 6) + (a >> 2); return a; };
  uint64_t t = ++h->proj_counter, bits;
  t = mix(t, (uint64_t)(uintptr_t)phys); t = mix(t, (uint64_t)(uintptr_t)fe2d);
  std::memcpy(&bits, &ud_angle_deg, 8); t = mix(t, bits);
  std::memcpy(&bits, &va_angle_deg, 8); t = mix(t, bits);
  t = mix(t, (uint64_t)h->proj_rec.begin); t = mix(t, (uint64_t)h->proj_rec.end);
  h->proj_token = (t << 16) | (h->proj_counter & 0xffff) | 1ull << 63;
  *token = h->proj_token;
  return 0;
}

// ---- its forward mode: the saving forward, per table direction the projection of the tangent table, then the tail in groups of
// kFf2dJvpW directions (k_ff2d_jvp.inc)
struct FormFactor2dJvpPlan {
  FormFactor2dPlan fwd;            // the saving forward of the range
  int n_dir = 0;
  bool tab = false;                // fe2d_dot given: every direction's table is projected
  long npoint = 0;
  size_t tail_smem = 0;
  unsigned tail_grid = 0;
};

static int form_factor_2d_jvp_prepare(tsff_handle* h, int feature, int nv, int B, int n_dir, bool tab, bool want_P, int64_t point_begin,
                                      int64_t point_end, FormFactor2dJvpPlan& p) {
  p.n_dir = n_dir; p.tab = tab;
  if (int rc = form_factor_2d_prepare(h, feature, nv, true, B, point_begin, point_end, true, p.fwd)) return rc;
  p.npoint = p.fwd.end - p.fwd.begin;
  if (p.npoint == 0) return 0;
  p.tail_smem = sizeof(double) * ff2d_jvp_smem_doubles(nv, kFf2dJvpW);
  // one wavefront per workgroup, each with a contiguous run of points: enough of them to fill the device's wavefront slots
  p.tail_grid = (unsigned)std::min<long>(p.npoint, (long)h->ncu2d() * 32);
  if (tab) {
    TSFF_ENSURE(h, h->ff2j_tab, (size_t)std::min(kFf2dJvpW, n_dir) * p.npoint * nv * sizeof(double));
    if (!p.fwd.lds) TSFF_ENSURE(h, h->ff2j_pad, pad2d_doubles(nv) * sizeof(double));
    TSFF_ENSURE(h, h->ff2j_flags, (size_t)n_dir * sizeof(int));
  }
  if (!want_P) TSFF_ENSURE(h, h->ff2j_P, (size_t)p.fwd.end * sizeof(double));
  return 0;
}

static int form_factor_2d_jvp_enqueue(tsff_handle* h, const FormFactor2dJvpPlan& p, const double* phys, const double* fe2d, double ud_angle_deg,
                                      double va_angle_deg, const double* phys_dot, const double* fe2d_dot, double* P, double* P_dot) {
  if (p.npoint == 0) return 0;
  const FormFactor2dPlan& q = p.fwd;
  const int nv = q.nv;
  if (int rc = form_factor_2d_enqueue(h, q, phys, fe2d, ud_angle_deg, va_angle_deg, P ? P : h->ff2j_P.as<double>())) return rc;
  invalidate_proj(h);   // (the records are this call's own: no token names them)
  if (int rc = timing_begin(h)) return rc;
  const double ud = ud_angle_deg * kPi / 180.0, va = va_angle_deg * kPi / 180.0;
  if (p.tab) TSFF_LAUNCH0(h, k_ff2d_tabflags, dim3(p.n_dir), dim3(kThreads), 0, h->stream, fe2d_dot, nv, h->ff2j_flags.as<int>());
  for (int d0 = 0; d0 < p.n_dir; d0 += kFf2dJvpW) {
    const int nd = std::min(kFf2dJvpW, p.n_dir - d0);
    for (int k = 0; p.tab && k < nd; ++k) {
      const double* table = fe2d_dot + (size_t)(d0 + k) * nv * nv;
      if (!q.lds) {   // the padded copy of the tangent table: its ghost cells are the tangents of the table's
        TSFF_LAUNCH0(h, k_pad2d, dim3(1), dim3(kThreads), 0, h->stream, table, nv, h->ff2j_pad.as<double>());
        table = h->ff2j_pad.as<double>() + pad2d_margin(nv);
      }
      dim3 grid((unsigned)std::min((p.npoint + q.groups - 1) / q.groups, q.max_grid)), block(q.groups * kThreads);
      TSFF_LAUNCH_FN(h, ff2d_project_kernel(h->n_ion, q.lds), ("k_ff2d_project", h->n_ion, q.lds, q.groups), grid, block, q.smem, h->stream,
                     h->S, phys, table, nv, ud, va, q.feature, q.begin, q.end, h->ff2j_tab.as<double>() + (size_t)k * p.npoint * nv,
                     h->ff2j_flags.as<int>() + d0 + k);
    }
    Ff2dJvpArgs A{};
    A.d0 = d0; A.nd = nd; A.B = q.B; A.nv = nv; A.feature = q.feature;
    A.pbegin = q.begin; A.pend = q.end; A.ud_ang = ud; A.va_ang = va;
    A.phys = phys; A.phys_dot = phys_dot; A.proj = h->proj.as<double>();
    A.f1tab = p.tab ? h->ff2j_tab.as<double>() : nullptr;
    A.tabflags = p.tab ? h->ff2j_flags.as<int>() + d0 : nullptr;
    A.P_dot = P_dot;
    TSFF_LAUNCH_FN(h, ff2d_jvp_kernel(h->n_ion), ("k_ff2d_jvp", h->n_ion, kFf2dJvpW), dim3(p.tail_grid), dim3(kFf2dJvpThreads), p.tail_smem,
                   h->stream, h->S, A);
    TSFF_HIP(h, hipGetLastError());
  }
  return timing_end(h);
}

int tsff_form_factor_2d_jvp(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv, double ud_angle_deg,
                            double va_angle_deg, int32_t B, int32_t n_dir, const double* phys_dot, const double* fe2d_dot,
                            int64_t point_begin, int64_t point_end, double* P, double* P_dot) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!phys || !fe2d || !phys_dot || !P_dot || B < 1 || n_dir < 1 || feature < 0 || feature > 1 || nv < 4) return fail(h, -1, "bad argument");
  if (nv > 256) return fail(h, -2, "tsff_form_factor_2d_jvp: nv <= 256 (the forward mode reads the projection records of a saving forward)");
  FormFactor2dJvpPlan p;
  if (int rc = form_factor_2d_jvp_prepare(h, feature, nv, B, n_dir, fe2d_dot != nullptr, P != nullptr, point_begin, point_end, p)) return rc;
  return form_factor_2d_jvp_enqueue(h, p, phys, fe2d, ud_angle_deg, va_angle_deg, phys_dot, fe2d_dot, P, P_dot);
}

// ---- its adjoint for the points [begin, end) (a rank's share; the adjoints are sums over points) of one table shared by all
// lineouts (the 2-D path is never batched in the reference); table: with the table adjoint
struct FormFactor2dAdjPlan {
  int feature = 0, nv = 0, B = 0;
  long begin = 0, end = 0;
  bool lds = false, table = false;  // the table fits LDS; with the table adjoint
  int groups = 0, nworker = 0;      // point groups per workgroup; partial slots of the lineout-scalar adjoints: one per point
  size_t smem = 0;                  // group and (lineout, gradient point); LDS of k_form_factor_2d_adj
  dim3 grid, block;
  // k_ff2d_table_adj: tiles of the table, workgroups per tile, LDS, doubles of a partial tile
  int ntiles = 0; unsigned per_tile = 0; size_t tile_smem = 0, slab = 0;
};

static int form_factor_2d_adj_prepare(tsff_handle* h, int feature, int nv, int B, long begin, long end, bool table,
                                      FormFactor2dAdjPlan& p, bool dry = false) {
  p.feature = feature; p.nv = nv; p.B = B; p.begin = begin; p.end = end; p.table = table;
  const int NLB = kNLB2 + 3 * h->n_ion;
  const long npoint = end - begin;
  constexpr int kGL = TSFF_2D_GROUPS_LDS, kGG = TSFF_2D_GROUPS_L2;
  p.lds = sizeof(double) * smem2d_adj_doubles(nv, true, kGL) <= kLdsLimit;
  p.groups = p.lds ? kGL : kGG;
  p.smem = sizeof(double) * smem2d_adj_doubles(nv, p.lds, p.groups);
  if (p.smem > kLdsLimit) return fail(h, -2, "nv = %d needs %zu B of LDS scratch", nv, p.smem);
  const long want = (long)h->ncu2d() * (p.lds ? 1 : 8);
  p.grid = dim3((unsigned)std::max<long>(1, std::min((npoint + p.groups - 1) / p.groups, want)));
  p.block = dim3(p.groups * kThreads);
  p.nworker = (int)p.grid.x * p.groups;
  if (table) {
    const int ncell = nv - 1, ntx = (ncell + kTile2 - 1) / kTile2, tmax = std::min(ncell, kTile2) + 3;
    p.ntiles = ntx * ntx;
    p.tile_smem = sizeof(double) * (size_t)tmax * (tmax | 1);
    p.per_tile = (unsigned)std::max<long>(1, std::min<long>((npoint + 3) / 4, h->ncu2d() / p.ntiles));
    p.slab = (size_t)tmax * tmax;
  }
  if (dry) return 0;
  TSFF_ENSURE(h, h->lbacc, (size_t)B * h->S.G * NLB * sizeof(double));
  if (table) TSFF_ENSURE(h, h->f1bar, (size_t)npoint * (nv + 2) * sizeof(double));
  if (!p.lds) TSFF_ENSURE(h, h->fpad, pad2d_doubles(nv) * sizeof(double));
  TSFF_ENSURE(h, h->lbparts, (size_t)B * h->S.G * p.nworker * NLB * sizeof(double));
  if (table) {
    TSFF_ENSURE(h, h->fbar_pad, (size_t)(nv + 2) * (nv + 2) * sizeof(double));
    TSFF_ENSURE(h, h->fbar_parts, (size_t)p.per_tile * p.ntiles * p.slab * sizeof(double));
  }
  return 0;
}

// proj: the projection records of the saving forward of exactly these points and inputs (checked by the caller), or nullptr
static int form_factor_2d_adj_enqueue(tsff_handle* h, const FormFactor2dAdjPlan& p, const double* phys, const double* fe2d,
                                      double ud_angle_deg, double va_angle_deg, const double* proj, const double* Pbar, double* grad_phys,
                                      double* grad_fe2d) {
  const int nv = p.nv, B = p.B, NLB = kNLB2 + 3 * h->n_ion;
  double* f1bar = p.table ? h->f1bar.as<double>() : nullptr;
  const double* table = fe2d;
  if (!p.lds) {
    TSFF_LAUNCH0(h, k_pad2d, dim3(1), dim3(kThreads), 0, h->stream, fe2d, nv, h->fpad.as<double>());
    table = h->fpad.as<double>() + pad2d_margin(nv);
  }
  const double ud = ud_angle_deg * kPi / 180.0, va = va_angle_deg * kPi / 180.0;
  // a point group only writes the partial slots of the (b, g) it meets, the others stay zero
  TSFF_HIP(h, hipMemsetAsync(h->lbparts.p, 0, (size_t)B * h->S.G * p.nworker * NLB * sizeof(double), h->stream));
  TSFF_LAUNCH_FN(h, form_factor_2d_adj_kernel(h->n_ion, p.lds), ("k_form_factor_2d_adj", h->n_ion, p.lds, p.groups), p.grid, p.block, p.smem,
                 h->stream, h->S, phys, table, nv, ud, va, p.feature, p.begin, p.end, Pbar, h->lbparts.as<double>(), f1bar, proj);
  TSFF_LAUNCH0(h, k_lbacc_reduce, dim3(B * h->S.G), dim3(kThreads), 0, h->stream, h->lbparts.as<double>(), p.nworker, NLB,
               h->lbacc.as<double>());
  TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_ff2d_lines_adj, dim3((B + 63) / 64), dim3(64), 0, h->stream, h->S, phys, p.feature, B,
                  h->lbacc.as<double>(), grad_phys, 0);
  TSFF_HIP(h, hipGetLastError());
  if (!p.table) return 0;
  TSFF_HIP(h, hipMemsetAsync(h->fbar_pad.p, 0, (size_t)(nv + 2) * (nv + 2) * sizeof(double), h->stream));
  TSFF_LAUNCH0(h, k_ff2d_table_adj, dim3(p.per_tile, p.ntiles), dim3(4 * kThreads), p.tile_smem, h->stream, nv, f1bar, p.end - p.begin,
               h->fbar_parts.as<double>(), p.slab);
  for (int t = 0; t < p.ntiles; ++t)   // one launch per tile, in order: the overlapping halos of neighbouring tiles add up without atomics
    TSFF_LAUNCH0(h, k_ff2d_sum_tiles, dim3((unsigned)((p.slab + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, nv,
                       h->fbar_parts.as<double>(), (int)p.per_tile, p.slab, h->fbar_pad.as<double>(), t);
  TSFF_LAUNCH0(h, k_ff2d_fold_ghosts, dim3(1), dim3(kThreads), 0, h->stream, nv, h->fbar_pad.as<double>(), grad_fe2d);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

int tsff_form_factor_2d_grad(tsff_handle* h, int32_t feature, const double* phys, const double* fe2d, int32_t nv,
                             double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin, int64_t point_end,
                             uint64_t saved_token, const double* Pbar, double* grad_phys, double* grad_fe2d) {
  const bool use_saved = saved_token != 0;
  DevGuard dg__(h);
  if (!h || !phys || !fe2d || !Pbar || !grad_phys || B < 1 || feature < 0 || feature > 1 || nv < 4 || nv > 2048)
    return fail(h, -1, "bad argument");
  const long per_lineout = (long)h->S.G * h->S.npts * h->S.n_angles, nall = per_lineout * B;
  const long pb = point_begin, pe = point_end < 0 ? nall : point_end;
  if (pb < 0 || pe > nall || pb > pe) return fail(h, -1, "point range [%ld, %ld) outside [0, %ld]", pb, pe, nall);
  if (use_saved) {
    if (saved_token != h->proj_token)
      return fail(h, -22, "saved_token: stale or foreign token (the projection records belong to the LAST tsff_form_factor_2d_save of this "
                          "handle; any later 2-D forward invalidates them)");
    if (!h->proj_rec.covers(pb, pe, nv, feature))
      return fail(h, -2, "use_saved: no projection records of tsff_form_factor_2d_save for this point range / table size");
    if (!h->proj_rec.made_from(phys, fe2d, ud_angle_deg, va_angle_deg, B))
      return fail(h, -2, "use_saved: the projection records were made from other inputs (phys / fe2d buffers, drift or flow angle, B)");
  }
  FormFactor2dAdjPlan p;
  if (int rc = form_factor_2d_adj_prepare(h, feature, nv, B, pb, pe, grad_fe2d != nullptr, p)) return rc;
  return form_factor_2d_adj_enqueue(h, p, phys, fe2d, ud_angle_deg, va_angle_deg, use_saved ? h->proj.as<double>() : nullptr, Pbar,
                                    grad_phys, grad_fe2d);
}

int tsff_ats_setup(tsff_handle* h, const tsff_ats_config* c) {
  DevGuard dg__(h);
  if (!h || !c || !c->weights || !c->taps_ang || !c->taps_lam || !c->lam_axis) return fail(h, -1, "bad argument");
  if (c->n_px < 1 || c->lam_step < 1 || c->ang_step < 1 || h->S.npts % c->lam_step || c->n_px % c->ang_step)
    return fail(h, -2, "resolution units must divide the image");
  if (c->row_start < 0 || c->row_end > c->n_px / c->ang_step || c->row_end <= c->row_start)
    return fail(h, -2, "bad lineout range");
  TSFF_HIP(h, upload(h->ats_w, c->weights, (size_t)c->n_px * h->S.n_angles));
  TSFF_HIP(h, upload(h->ats_ta, c->taps_ang, c->n_taps_ang));
  TSFF_HIP(h, upload(h->ats_tl, c->taps_lam, c->n_taps_lam));
  TSFF_HIP(h, upload(h->ats_lam, c->lam_axis, h->S.npts));
  const size_t img = (size_t)c->n_px * h->S.npts * sizeof(double);
  TSFF_ENSURE(h, h->ats_M, img);
  TSFF_ENSURE(h, h->ats_A, img);
  TSFF_ENSURE(h, h->ats_B, img);
  h->ats_npx = c->n_px; h->ats_nta = c->n_taps_ang; h->ats_offa = c->tap_off_ang; h->ats_ntl = c->n_taps_lam;
  h->ats_offl = c->tap_off_lam; h->ats_lam_step = c->lam_step; h->ats_ang_step = c->ang_step;
  h->ats_row_start = c->row_start; h->ats_row_end = c->row_end;
  return 0;
}

// ---- the ATS instrument chain and its reverse.  adjoint: the reverse chain's refusal and buffers too
static int ats_prepare(tsff_handle* h, bool adjoint, bool dry = false) {
  if (h->ats_npx == 0) return fail(h, -2, "tsff_ats_setup has not been called");
  if (!adjoint) return 0;
  const int npts = h->S.npts, npx = h->ats_npx, rows = h->ats_row_end - h->ats_row_start;
  if (npts / h->ats_lam_step > TSFF_NBINS) return fail(h, -2, "more than %d wavelength resolution units per row", TSFF_NBINS);
  if (dry) return 0;
  const size_t img = (size_t)npx * npts * sizeof(double);
  TSFF_ENSURE(h, h->ats_C, img);
  TSFF_ENSURE(h, h->ats_D, img);
  TSFF_ENSURE(h, h->ats_stats, (size_t)npx * 4 * sizeof(double) + (size_t)rows * 2 * sizeof(double));
  return 0;
}

// the forward chain up to the unscaled convolved image: M = weights x P, A = M * taps_ang, B = A * taps_lam
static void ats_forward_chain(tsff_handle* h, const double* P) {
  const int npts = h->S.npts, npx = h->ats_npx;
  dim3 block(kThreads), grid((npts + kThreads - 1) / kThreads, npx);
  double* M = h->ats_M.as<double>();
  double* A = h->ats_A.as<double>();
  TSFF_LAUNCH0(h, k_ats_weights, grid, block, 0, h->stream, P, h->ats_w.as<double>(), h->S.filt, h->S.G, npts,
                     h->S.n_angles, npx, M);
  TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, M, h->ats_ta.as<double>(), h->ats_nta, h->ats_offa, 1, npx, npts, A);
  TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, A, h->ats_tl.as<double>(), h->ats_ntl, h->ats_offl, 0, npx, npts,
                     h->ats_B.as<double>());
}

// phys (device, optional): lam, amp1 and amp2 read from these physical parameters on the device instead of the scalars
static int ats_spectrum_enqueue(tsff_handle* h, const double* P, const double* e_amps, double lam, double amp1, double amp2,
                                const double* phys, double* ThryE) {
  const int npts = h->S.npts;
  double* Bm = h->ats_B.as<double>();
  ats_forward_chain(h, P);
  TSFF_LAUNCH0(h, k_ats_rownorm, dim3(h->ats_npx), dim3(kThreads), 0, h->stream, h->ats_M.as<double>(), Bm, npts);
  TSFF_LAUNCH0(h, k_ats_resunit, dim3(h->ats_row_end - h->ats_row_start), dim3(kThreads), 0, h->stream, Bm, h->ats_lam.as<double>(),
                     npts, h->ats_lam_step, h->ats_ang_step, h->ats_row_start, e_amps, lam, amp1, amp2, phys, ThryE);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

int tsff_ats_spectrum(tsff_handle* h, const double* P, const double* e_amps, double lam, double amp1, double amp2, double* ThryE) {
  DevGuard dg__(h);
  if (!h || !P || !ThryE || !e_amps) return fail(h, -1, "bad argument");
  if (int rc = ats_prepare(h, false)) return rc;
  return ats_spectrum_enqueue(h, P, e_amps, lam, amp1, amp2, nullptr, ThryE);
}

// the amplitude adjoints of the reverse chain stay on the device, per output row: [rows][2] behind the row statistics
static double* ats_amp_bar(tsff_handle* h) { return h->ats_stats.as<double>() + (size_t)h->ats_npx * 4; }

static int ats_adjoint_enqueue(tsff_handle* h, const double* P, const double* e_amps, double lam, double amp1, double amp2,
                               const double* phys, const double* Ebar, double* Pbar) {
  const int npts = h->S.npts, npx = h->ats_npx, rows = h->ats_row_end - h->ats_row_start;
  dim3 block(kThreads), grid((npts + kThreads - 1) / kThreads, npx);
  double* M = h->ats_M.as<double>();
  double* A = h->ats_A.as<double>();
  double* Bm = h->ats_B.as<double>();
  double* Cb = h->ats_C.as<double>();
  double* Db = h->ats_D.as<double>();
  double* stats = h->ats_stats.as<double>();
  ats_forward_chain(h, P);
  TSFF_LAUNCH0(h, k_ats_rowstats, dim3(npx), block, 0, h->stream, M, Bm, npts, stats);
  // reverse
  TSFF_HIP(h, hipMemsetAsync(Cb, 0, (size_t)npx * npts * sizeof(double), h->stream));
  TSFF_LAUNCH0(h, k_ats_resunit_adj, dim3(rows), block, 0, h->stream, Bm, stats, h->ats_lam.as<double>(), npts, h->ats_lam_step,
                     h->ats_ang_step, h->ats_row_start, e_amps, lam, amp1, amp2, phys, Ebar, Cb, ats_amp_bar(h));
  TSFF_LAUNCH0(h, k_ats_rownorm_adj, dim3(npx), block, 0, h->stream, Bm, stats, npts, Cb, Db);              // Cb -> Bmbar, Db = Mbar one-hots
  TSFF_LAUNCH0(h, k_ats_conv_adj, grid, block, 0, h->stream, Cb, h->ats_tl.as<double>(), h->ats_ntl, h->ats_offl, 0, npx, npts, 0, A);   // A = Abar
  TSFF_LAUNCH0(h, k_ats_conv_adj, grid, block, 0, h->stream, A, h->ats_ta.as<double>(), h->ats_nta, h->ats_offa, 1, npx, npts, 1, Db);  // Db += conv^T
  dim3 wgrid((h->S.n_angles + kThreads - 1) / kThreads, npts);
  TSFF_LAUNCH0(h, k_ats_weights_adj, wgrid, block, 0, h->stream, Db, h->ats_w.as<double>(), h->S.filt, h->S.G, npts, h->S.n_angles,
                     npx, Pbar);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

int tsff_ats_adjoint(tsff_handle* h, const double* P, const double* e_amps, double lam, double amp1, double amp2,
                     const double* Ebar, double* Pbar, double* amp_bar) {
  DevGuard dg__(h);
  if (!amp_bar || !h || !P || !e_amps || !Ebar || !Pbar) return fail(h, -1, "bad argument");
  int rc = ats_prepare(h, true);
  if (!rc) rc = ats_adjoint_enqueue(h, P, e_amps, lam, amp1, amp2, nullptr, Ebar, Pbar);
  if (rc) return rc;
  const int rows = h->ats_row_end - h->ats_row_start;
  // amp adjoints: sum over the rows (host: a few hundred numbers)
  std::vector<double> hb((size_t)rows * 2);
  TSFF_HIP(h, hipMemcpyAsync(hb.data(), ats_amp_bar(h), hb.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  TSFF_HIP(h, hipStreamSynchronize(h->stream));
  amp_bar[0] = amp_bar[1] = 0.0;
  for (int r = 0; r < rows; ++r) { amp_bar[0] += hb[2 * r]; amp_bar[1] += hb[2 * r + 1]; }
  return 0;
}

// ---- forward mode of the ATS chain.  The linear stages (weights, the two convolutions) run on each tangent image with the shipped
// kernels; the two row normalisations take their tangent through 1 / max at the value's arg-max (k_ats_rownorm_jvp, k_ats_resunit_jvp)
static int ats_jvp_prepare(tsff_handle* h) {
  if (int rc = ats_prepare(h, true)) return rc;   // (the row statistics and two of the three tangent images are the reverse chain's buffers)
  TSFF_ENSURE(h, h->ats_E, (size_t)h->ats_npx * h->S.npts * sizeof(double));
  return 0;
}

static int ats_jvp_enqueue(tsff_handle* h, const double* P, const double* P_dot, int n_dir, const double* e_amps, double lam, double amp1,
                           double amp2, const double* amp_dot, double* ThryE, double* ThryE_dot) {
  const int npts = h->S.npts, npx = h->ats_npx, rows = h->ats_row_end - h->ats_row_start, nJ = npts / h->ats_lam_step;
  dim3 block(kThreads), grid((npts + kThreads - 1) / kThreads, npx);
  double* M = h->ats_M.as<double>();
  double* Bm = h->ats_B.as<double>();
  double* Md = h->ats_C.as<double>();
  double* Ad = h->ats_D.as<double>();
  double* Bd = h->ats_E.as<double>();
  double* stats = h->ats_stats.as<double>();
  if (int rc = timing_begin(h)) return rc;
  // the value: tsff_ats_spectrum's launches, with the row statistics taken before k_ats_rownorm scales the image in place
  ats_forward_chain(h, P);
  TSFF_LAUNCH0(h, k_ats_rowstats, dim3(npx), block, 0, h->stream, M, Bm, npts, stats);
  TSFF_LAUNCH0(h, k_ats_rownorm, dim3(npx), block, 0, h->stream, M, Bm, npts);
  if (ThryE)
    TSFF_LAUNCH0(h, k_ats_resunit, dim3(rows), block, 0, h->stream, Bm, h->ats_lam.as<double>(), npts, h->ats_lam_step, h->ats_ang_step,
                 h->ats_row_start, e_amps, lam, amp1, amp2, (const double*)nullptr, ThryE);
  TSFF_HIP(h, hipGetLastError());
  const size_t pimg = (size_t)h->S.G * npts * h->S.n_angles;
  for (int d = 0; d < n_dir; ++d) {
    TSFF_LAUNCH0(h, k_ats_weights, grid, block, 0, h->stream, P_dot + (size_t)d * pimg, h->ats_w.as<double>(), h->S.filt, h->S.G, npts,
                 h->S.n_angles, npx, Md);
    TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, Md, h->ats_ta.as<double>(), h->ats_nta, h->ats_offa, 1, npx, npts, Ad);
    TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, Ad, h->ats_tl.as<double>(), h->ats_ntl, h->ats_offl, 0, npx, npts, Bd);
    TSFF_LAUNCH0(h, k_ats_rownorm_jvp, dim3(npx), block, 0, h->stream, Bm, stats, Md, npts, Bd);
    TSFF_LAUNCH0(h, k_ats_resunit_jvp, dim3(rows), block, 0, h->stream, Bm, Bd, h->ats_lam.as<double>(), npts, h->ats_lam_step,
                 h->ats_ang_step, h->ats_row_start, e_amps, lam, amp1, amp2, amp_dot[2 * d], amp_dot[2 * d + 1],
                 ThryE_dot + (size_t)d * rows * nJ);
    TSFF_HIP(h, hipGetLastError());
  }
  return timing_end(h);
}

int tsff_ats_jvp(tsff_handle* h, const double* P, const double* P_dot, int32_t n_dir, const double* e_amps, double lam, double amp1,
                 double amp2, const double* amp_dot, double* ThryE, double* ThryE_dot) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!P || !P_dot || !e_amps || !amp_dot || !ThryE_dot || n_dir < 1) return fail(h, -1, "bad argument");
  if (int rc = ats_jvp_prepare(h)) return rc;
  return ats_jvp_enqueue(h, P, P_dot, n_dir, e_amps, lam, amp1, amp2, amp_dot, ThryE, ThryE_dot);
}

// the KCall of a batch and its tables.  Launches only: the batch is checked (check_batch) and the workspace sized
// (ensure_workspace) by then
static int fill_call(tsff_handle* h, KCall& K, const Batch& b, double* ThryE, double* ThryI, bool pipe = false) {
  K.params = b.params; K.B = b.B; K.b0 = 0; K.Btot = b.B;
  for (int f = 0; f < 2; ++f) { K.data[f] = b.data[f]; K.amps[f] = b.amps[f]; K.noise[f] = b.noise[f]; }
  K.thry[0] = ThryE; K.thry[1] = ThryI;
  K.lpart = h->lpart.as<double>();
  return prepare_tables(h, b.params, b.fe, b.B, K, pipe);
}

int tsff_forward(tsff_handle* h, const double* params, const double* fe, const double* e_amps, const double* i_amps,
                 const double* noise_e, const double* noise_i, int32_t B, double* ThryE, double* ThryI) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (h->S.load[0] && !ThryE) return fail(h, -1, "ThryE missing");
  if (h->S.load[1] && !ThryI) return fail(h, -1, "ThryI missing");
  const Batch b{params, fe, {nullptr, nullptr}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  SpectrumPlan plan;
  int rc = check_batch(h, b, false);
  if (!rc) rc = size_plan(h, 0, 0, B, plan);
  if (!rc) rc = ensure_workspace(h, B);
  if (rc) return rc;
  KCall K{};
  if ((rc = fill_call(h, K, b, ThryE, ThryI))) return rc;
  return launch_spectrum(h, 0, 0, K, plan);
}

struct PackedOut {   // tsff_loss_grad_packed
  const int32_t* act = nullptr;
  int32_t n_act = 0;
  int64_t B_global = 0, b_off = 0;
  double* packed = nullptr;
};

// One loss + gradient evaluation: what it reads and where its results go (the entry point's), then what loss_grad_prepare
// decided.  loss_grad_prepare holds everything that can refuse, allocate, upload or synchronise; loss_grad_enqueue only
// launches, so a fit loop prepares once and enqueues once per step.
struct LossGradCall {
  Batch b;
  const double* weights;
  const uint8_t* grad_mask;
  double *loss_terms, *grad, *grad_fe;
  bool want_fe;            // tsff_loss_grad_fe: the f_e gradient too
  double *ThryE, *ThryI;
  const PackedOut* po;     // the packed form (loss_terms and grad are then the handle's)
  bool with_m = false;     // loss_grad_prepare: the DLM order is a leaf
  int gm = 0;              // loss_grad_prepare: GM of the spectrum kernels (0 plasma parameters, 1 + the DLM order, 2 + the table adjoints)
  SpectrumPlan plan;       // loss_grad_prepare: the sized plan
};

// every argument is checked before anything is enqueued: a refused call leaves nothing behind
static int loss_grad_prepare(tsff_handle* h, LossGradCall& c) {
  const PackedOut* po = c.po;
  const int B = c.b.B;
  if (po) {
    if (!po->act || !po->packed || po->n_act < 1 || po->n_act > h->S.NP || po->b_off < 0 || po->b_off + B > po->B_global)
      return fail(h, -1, "bad packed-output argument (slots %d, lineouts [%lld, %lld) of %lld)", (int)po->n_act, (long long)po->b_off,
                  (long long)(po->b_off + B), (long long)po->B_global);
    for (int k = 0; k < po->n_act; ++k)
      if (po->act[k] < 0 || po->act[k] >= h->S.NP) return fail(h, -1, "active slot %d out of range", (int)po->act[k]);
    c.loss_terms = po->packed;
  }
  if (!c.weights || !c.grad_mask || !c.loss_terms || (!po && !c.grad)) return fail(h, -1, "bad argument");
  if (c.want_fe && (h->fe_mode != TSFF_FE_PER_LINEOUT || !c.grad_fe))
    return fail(h, -2, "gradient w.r.t. f_e needs fe_mode == TSFF_FE_PER_LINEOUT and an output buffer");
  int rc = check_mask(h, c.grad_mask, h->fe_mode == TSFF_FE_DLM);
  if (!rc) rc = check_batch(h, c.b, true);
  if (rc) return rc;
  c.with_m = c.grad_mask[TSFF_P_M] != 0;
  // a changed mask / slot list is uploaded synchronously (pageable source, once per change) -- refused inside graph capture
  if ((rc = upload_mask(h, c.grad_mask))) return rc;
  if (po && (rc = upload_slots(h, po->act, po->n_act))) return rc;
  // (the pipelined DLM plan forks onto the handle's second stream: not inside a capture, which this library keeps to one stream)
  if (h->capturing && h->fe_mode == TSFF_FE_DLM && !c.want_fe && c.with_m && h->dlm_blocks > 1)
    return fail(h, -2, "graph capture: TSFF_OPT_DLM_BLOCKS > 1 would fork onto a second stream (set it to 0 before capturing)");
  c.gm = c.want_fe ? 2 : c.with_m ? 1 : 0;
  if ((rc = size_plan(h, 1, c.gm, B, c.plan))) return rc;
  if ((rc = ensure_workspace(h, B))) return rc;
  if (c.want_fe && (rc = fe_tail_prepare(h, 2, B))) return rc;    // (x 2: per-feature parts of the interleaved plan)
  if (po) TSFF_ENSURE(h, h->gradws, gradws_bytes(h->S, B));
  return 0;
}

// the launches of a prepared call: the tables, the spectrum kernels of the plan, the reduction.  What can fail here is a HIP
// error (the timing ring's events and the second stream of the pipelined DLM plan included)
static int loss_grad_enqueue(tsff_handle* h, const LossGradCall& c) {
  const PackedOut* po = c.po;
  const int B = c.b.B;
  const bool with_m = c.with_m;
  double* const grad = po ? h->gradws.as<double>() : c.grad;
  KCall K{};
  // (the DLM order as a leaf, no table adjoints: the one-sweep kernel can take the per-lineout tables block by block)
  const bool pipe = h->fe_mode == TSFF_FE_DLM && !c.want_fe && with_m;
  int rc = fill_call(h, K, c.b, c.ThryE, c.ThryI, pipe);
  if (rc) return rc;
  K.wts[0] = c.weights[0]; K.wts[1] = c.weights[1]; K.wts[2] = c.weights[2];
  K.denom_mode = h->denom_mode;
  const bool parts = c.plan.gpart != 0, lbrec = c.plan.form == SpectrumForm::one_sweep;
  if (c.want_fe) fe_tail_outputs(h, K, B);
  if ((rc = launch_spectrum(h, 1, c.gm, K, c.plan, h->gmask.as<uint8_t>(), grad))) return rc;
  if (c.want_fe) {
    if (parts) {
      const long nw = (long)B * kNXi2, nh = (long)2 * B * h->S.nvx;
      TSFF_LAUNCH0(h, k_add_parts, dim3((unsigned)std::min<long>((nw + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0, h->stream,
                         K.Wb_out, K.Wb_out + nw, nw);
      TSFF_LAUNCH0(h, k_add_parts, dim3((unsigned)std::min<long>((nh + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0, h->stream,
                         K.Hy_out, K.Hy_out + nh, nh);
      TSFF_HIP(h, hipGetLastError());
    }
    if ((rc = fe_tail_enqueue(h, K, B, c.grad_fe))) return rc;
  }
  const long ng = (long)B * h->S.NP;
  if (lbrec) {   // the one-sweep kernel ran: one thread per lineout finishes the gradient and packs it (k_spectrum_fused.inc)
    const int nload = (h->S.load[0] ? 1 : 0) + (h->S.load[1] ? 1 : 0), f0 = h->S.load[0] ? 0 : 1;
    const int per_wg = kThreads / nload;
    const dim3 fgrid((unsigned)((B + per_wg - 1) / per_wg) + 1);   // (+ 1: the last workgroup reduces the loss sums)
    TSFF_LAUNCH_ION(h, kFusedMaxIon, k_fused_finish, fgrid, dim3(kThreads), 0, h->stream, h->S, h->finrec.as<double>(), K.lbrec, K.lpart, (int)B,
                    f0, nload, with_m ? 1 : 0, h->gmask.as<uint8_t>(), grad, po ? nullptr : c.loss_terms, po ? h->act.as<int>() : nullptr,
                    po ? (int)po->n_act : 0, po ? (long)po->B_global : 0L, po ? (long)po->b_off : 0L, po ? po->packed : nullptr);
  } else if (po) {
    const long n = (long)po->n_act * po->B_global;
    TSFF_LAUNCH0(h, k_loss_reduce_packed, dim3((unsigned)std::max<long>(1, std::min<long>((n + kThreads - 1) / kThreads, 1024))), dim3(kThreads),
                       0, h->stream, K.lpart, (int)B, parts ? K.gpart : nullptr, grad, h->S.NP, h->act.as<int>(), (int)po->n_act,
                       (long)po->B_global, (long)po->b_off, po->packed);
  } else {
    TSFF_LAUNCH0(h, k_loss_reduce, dim3(parts ? (unsigned)std::min<long>((ng + kThreads - 1) / kThreads, 256) : 1), dim3(kThreads), 0,
                       h->stream, K.lpart, (int)B, c.loss_terms, parts ? K.gpart : nullptr, ng, grad);
  }
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

static int loss_grad(tsff_handle* h, LossGradCall c) {
  if (!h) return -1;
  if (int rc = loss_grad_prepare(h, c)) return rc;
  return loss_grad_enqueue(h, c);
}

int tsff_loss_grad(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                   const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                   const double* weights, const uint8_t* grad_mask, double* loss_terms, double* grad, double* ThryE,
                   double* ThryI) {
  DevGuard dg__(h);
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  return loss_grad(h, {b, weights, grad_mask, loss_terms, grad, nullptr, false, ThryE, ThryI, nullptr});
}

int tsff_loss_grad_fe(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                      const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                      const double* weights, const uint8_t* grad_mask, double* loss_terms, double* grad, double* grad_fe,
                      double* ThryE, double* ThryI) {
  DevGuard dg__(h);
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  return loss_grad(h, {b, weights, grad_mask, loss_terms, grad, grad_fe, true, ThryE, ThryI, nullptr});
}

int tsff_loss_grad_packed(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                          const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                          const double* weights, const uint8_t* grad_mask, const int32_t* active_slots, int32_t n_active,
                          int64_t B_global, int64_t b_offset, double* packed, double* ThryE, double* ThryI) {
  DevGuard dg__(h);
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  const PackedOut po{active_slots, n_active, B_global, b_offset, packed};
  return loss_grad(h, {b, weights, grad_mask, nullptr, nullptr, nullptr, false, ThryE, ThryI, &po});
}

// The set-up tsff_adam_fit and tsff_lbfgs_fit share once their arguments are checked (F.gm: the mask check_slots made of the
// slot list): the packed buffer of 3 + n_active * B doubles their steps write and read, and loss_grad_prepare in the packed
// form.  The loop that follows calls loss_grad_enqueue and its own step kernel, nothing else: it allocates nothing, never
// synchronises and refuses nothing after the first launch.
struct PackedFit {
  uint8_t gm[kNP_MAX];
  PackedOut po;
  LossGradCall c;
};
static int prepare_packed_fit(tsff_handle* h, PackedFit& F, const Batch& b, const double* weights, const int32_t* act, int n_act) {
  TSFF_ENSURE(h, h->fit_packed, (size_t)(3 + (long)n_act * b.B) * sizeof(double));
  F.po = {act, n_act, b.B, 0, h->fit_packed.as<double>()};
  F.c = {b, weights, F.gm, nullptr, nullptr, nullptr, false, nullptr, nullptr, &F.po};
  return loss_grad_prepare(h, F.c);
}

// the 1-D Adam fit on the device (k_adam.inc): prepare_packed_fit, then n_steps x (loss_grad_enqueue + k_adam_step), all
// enqueued on the handle's stream
int tsff_adam_fit(tsff_handle* h, double* params, const double* fe, const double* e_data, const double* i_data, const double* e_amps,
                  const double* i_amps, const double* noise_e, const double* noise_i, int32_t B, const double* weights,
                  const int32_t* active_slots, int32_t n_active, int32_t n_steps, int32_t step0, const double* hyper, double* state,
                  double* loss_hist, double* best) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!params || B < 1 || !weights || !active_slots || !hyper || !state || !best || n_active < 1 || n_active > h->S.NP ||
      n_steps < 0 || step0 < 0 || (int64_t)step0 + n_steps > 0x7fffffffLL)
    return fail(h, -1, "bad argument");
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  PackedFit F;
  int rc = check_slots(h, active_slots, n_active, F.gm, h->fe_mode == TSFF_FE_DLM);
  if (!rc) rc = check_batch(h, b, true);
  if (rc || n_steps == 0) return rc;
  if ((rc = prepare_packed_fit(h, F, b, weights, active_slots, n_active))) return rc;
  TSFF_ENSURE(h, h->adam_best, 2 * sizeof(double));
  const long n = (long)n_active * B;
  // the optimiser's scalars exactly as tree.Adam computes them in Python (1 - b1, -lr, 1 - b1**count: glibc pow is Python's **)
  const double lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3];
  const double omb1 = 1.0 - b1, omb2 = 1.0 - b2, neg_lr = -lr;
  const double* packed = F.po.packed;
  double* bl = h->adam_best.as<double>();   // bl[t & 1]: the best loss before step t, bl[(t + 1) & 1]: after it
  double* mu = state;
  double* nu = state + n;
  TSFF_HIP(h, hipMemcpyAsync(bl, best, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  const dim3 agrid((unsigned)std::min<long>((n + kThreads - 1) / kThreads, 1024));
  for (int t = 0; t < n_steps; ++t) {
    if ((rc = loss_grad_enqueue(h, F.c))) return rc;
    const double count = (double)step0 + t + 1;
    const double c1 = 1.0 - std::pow(b1, count), c2 = 1.0 - std::pow(b2, count);
    TSFF_LAUNCH0(h, k_adam_step, agrid, dim3(kThreads), 0, h->stream, packed, weights[0], weights[1], weights[2],
                 h->act.as<int>(), (int)n_active, (int)B, h->S.NP, params, mu, nu, b1, omb1, b2, omb2, neg_lr, c1, c2, eps,
                 loss_hist ? loss_hist + t : nullptr, (const double*)(bl + (t & 1)), bl + ((t + 1) & 1),
                 t == n_steps - 1 ? best : nullptr, best + 1);
    TSFF_HIP(h, hipGetLastError());
  }
  return 0;
}

// ---- the trained f_e generators (k_sph.inc, k_arb1v.inc).  sph_check, arb1v_check: the refusals; gen_forward, gen_adjoint: the
// launches of generator gen (TSFF_ANG_SPH: S, n_gen parameters; TSFF_ANG_ARB1V: gen_data = S | S^T; any other: none), for the stand-alone
// entry points and for tsff_angular_fit.  The caller has checked the sizes and holds sph_ws_doubles / arb1v_ws_doubles in ws.
static int sph_check(tsff_handle* h, int type, int H, int nv, int nvr, int n_gen) {
  if (type != TSFF_SPH_MORA_YAHI && type != TSFF_SPH_ARBITRARY) return fail(h, -2, "unknown radial type %d", type);
  if (type == TSFF_SPH_MORA_YAHI && H != 2) return fail(h, -2, "Mora-Yahi radial functions: l = 1 only (n_harm = 2), got %d", H);
  if (H < 1 || H > kSphMaxH) return fail(h, -2, "n_harm must be 1 .. %d, got %d", kSphMaxH, H);
  if (nvr < 2) return fail(h, -2, "nvr must be >= 2, got %d", nvr);
  if (nv < 2 || nv > 4096) return fail(h, -2, "nv must be 2 .. 4096, got %d", nv);
  const long want = type == TSFF_SPH_MORA_YAHI ? (long)H + 1 : 2L * H * nvr + 1;
  if (n_gen != want) return fail(h, -2, "n_gen = %d, the generator has %ld parameters", n_gen, want);
  return 0;
}

static int arb1v_check(tsff_handle* h, int nv) {
  return nv < 4 || nv > kArb1vMaxNv ? fail(h, -2, "nv must be 4 .. %d, got %d", kArb1vMaxNv, nv) : 0;
}

static void arb1v_matvec(tsff_handle* h, const double* M, const double* x, int nv, double* y) {
  TSFF_LAUNCH0(h, k_arb1v_matvec, dim3((unsigned)((nv + kArb1vRows - 1) / kArb1vRows)), dim3(kThreads), 0, h->stream, M, x, nv, y);
}

// theta -> fe.  TSFF_ANG_ARB1V: fval -> u (ws) -> fe
static int gen_forward(tsff_handle* h, int gen, const SphGen& S, int n_gen, const double* gen_data, int nv, double dvx,
                       const double* theta, double* ws, double* fe) {
  if (gen == TSFF_ANG_SPH) TSFF_LAUNCH0(h, k_sph_table, dim3(1), dim3(kThreads), 0, h->stream, S, theta, n_gen, dvx * dvx, ws, fe);
  if (gen == TSFF_ANG_ARB1V) {
    arb1v_matvec(h, gen_data, theta, nv, ws);
    TSFF_LAUNCH0(h, k_arb1v_point, dim3(1), dim3(kThreads), 0, h->stream, (const double*)ws, nv, dvx, std::log(10.0), (const double*)nullptr, fe);
  }
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// fe_bar = d loss / d fe -> grad = d loss / d theta.  TSFF_ANG_ARB1V: u (ws, left by the forward), fe_bar -> g_u (ws) -> grad
static int gen_adjoint(tsff_handle* h, int gen, const SphGen& S, int n_gen, const double* gen_data, int nv, double dvx,
                       const double* theta, const double* fe_bar, double* ws, double* grad) {
  if (gen == TSFF_ANG_SPH)
    TSFF_LAUNCH0(h, k_sph_vjp, dim3(1), dim3(kThreads), 0, h->stream, S, theta, n_gen, 1.0 / (dvx * dvx), std::log(10.0), fe_bar, ws, grad);
  if (gen == TSFF_ANG_ARB1V) {
    TSFF_LAUNCH0(h, k_arb1v_point, dim3(1), dim3(kThreads), 0, h->stream, (const double*)ws, nv, dvx, std::log(10.0), fe_bar, ws + nv);
    arb1v_matvec(h, gen_data + (size_t)nv * nv, ws + nv, nv, grad);
  }
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

int tsff_sph_table(tsff_handle* h, int32_t sph_type, int32_t n_harm, int32_t nv, int32_t nvr, int32_t n_gen, double dvx,
                   const double* theta, const double* gen_data, double* fe) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!theta || !gen_data || !fe) return fail(h, -1, "bad argument");
  if (int rc = sph_check(h, sph_type, n_harm, nv, nvr, n_gen)) return rc;
  TSFF_ENSURE(h, h->sph_ws, sph_ws_doubles(n_harm, nv, nvr) * sizeof(double));
  return gen_forward(h, TSFF_ANG_SPH, sph_gen(sph_type, n_harm, nv, nvr, gen_data), n_gen, nullptr, nv, dvx, theta, h->sph_ws.as<double>(), fe);
}

int tsff_sph_table_vjp(tsff_handle* h, int32_t sph_type, int32_t n_harm, int32_t nv, int32_t nvr, int32_t n_gen, double dvx,
                       const double* theta, const double* gen_data, const double* fe_bar, double* grad) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!theta || !gen_data || !fe_bar || !grad) return fail(h, -1, "bad argument");
  if (int rc = sph_check(h, sph_type, n_harm, nv, nvr, n_gen)) return rc;
  TSFF_ENSURE(h, h->sph_ws, sph_ws_doubles(n_harm, nv, nvr) * sizeof(double));
  return gen_adjoint(h, TSFF_ANG_SPH, sph_gen(sph_type, n_harm, nv, nvr, gen_data), n_gen, nullptr, nv, dvx, theta, fe_bar,
                     h->sph_ws.as<double>(), grad);
}

int tsff_arb1v_table(tsff_handle* h, int32_t nv, double dvx, const double* fval, const double* gen_data, double* fe) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!fval || !gen_data || !fe) return fail(h, -1, "bad argument");
  if (int rc = arb1v_check(h, nv)) return rc;
  TSFF_ENSURE(h, h->arb1v_ws, arb1v_ws_doubles(nv) * sizeof(double));
  return gen_forward(h, TSFF_ANG_ARB1V, SphGen{}, 0, gen_data, nv, dvx, fval, h->arb1v_ws.as<double>(), fe);
}

int tsff_arb1v_table_vjp(tsff_handle* h, int32_t nv, double dvx, const double* fval, const double* gen_data, const double* fe_bar,
                         double* grad) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!fval || !gen_data || !fe_bar || !grad) return fail(h, -1, "bad argument");
  if (int rc = arb1v_check(h, nv)) return rc;
  TSFF_ENSURE(h, h->arb1v_ws, arb1v_ws_doubles(nv) * sizeof(double));
  double* ws = h->arb1v_ws.as<double>();
  arb1v_matvec(h, gen_data, fval, nv, ws);   // (u alone: the adjoint's pointwise kernel rebuilds f_e from it)
  return gen_adjoint(h, TSFF_ANG_ARB1V, SphGen{}, 0, gen_data, nv, dvx, fval, fe_bar, ws, grad);
}

// ---- tsff_angular_fit's f_e generator: a row of the table in include/tsff.h; ang_gen_describe makes every generator refusal of the fit
struct AngGen {
  bool two_d, m_leaf;        // f_e is an nv x nv table through the 2-D form factor (else nv values, 1-D); m may be an active slot
  bool fe_is_data, fe_bar;   // no f_e is built, gen_data is the table; the form-factor adjoint must return d loss / d f_e
  long n_table, hist_tail;   // leaves behind the NP scalars; how many of them a row of best_hist keeps
  size_t ws_doubles;         // the generator's scratch
  SphGen sph;                // TSFF_ANG_SPH: its constants
};
static int ang_gen_describe(tsff_handle* h, const tsff_angular_spec* sp, const double* gen_data, AngGen& G) {
  const int gen = sp->generator, nv = sp->nv, nvx = h->S.nvx;
  switch (gen) {   //            two_d  m_leaf fe_is_data fe_bar n_table hist_tail ws_doubles
    case TSFF_ANG_TABLE2D: G = {true, false, true, false, 0, 0, 0}; break;
    case TSFF_ANG_DLM: G = {false, true, false, false, 0, 0, 0}; break;   // (fe_bar: the fit asks for it when m is a leaf)
    case TSFF_ANG_ARB2V: G = {true, false, false, true, (long)nv * nv, 0, 0}; break;
    case TSFF_ANG_SPH: G = {true, false, false, true, sp->n_gen, sp->n_gen, 0}; break;   // (ws_doubles: below, once checked)
    case TSFF_ANG_ARB1V: G = {false, false, false, true, nv, nv, arb1v_ws_doubles(nv)}; break;
    default: return fail(h, -2, "unknown generator %d", gen);
  }
  int rc = 0;
  if (gen == TSFF_ANG_DLM && nv != nvx) return fail(h, -1, "DLM: nv must be the handle's nvx (%d)", nvx);
  if (gen == TSFF_ANG_ARB1V && nv != nvx) return fail(h, -1, "free-form 1-D f_e: nv must be the handle's nvx (%d), got %d", nvx, nv);
  if (gen == TSFF_ANG_ARB1V && (rc = arb1v_check(h, nv))) return rc;
  if (G.two_d && (nv < 4 || nv > 256)) return fail(h, -2, "2-D tables of nv = 4 .. 256 (the fit keeps the projection records)");
  if (gen != TSFF_ANG_ARB2V && !gen_data) return fail(h, -1, "gen_data missing");
  if (gen != TSFF_ANG_SPH || (rc = sph_check(h, sp->sph_type, sp->n_harm, nv, sp->nvr, sp->n_gen))) return rc;
  G.ws_doubles = sph_ws_doubles(sp->n_harm, nv, sp->nvr);
  G.sph = sph_gen(sp->sph_type, sp->n_harm, nv, sp->nvr, gen_data);
  return 0;
}

// the angular (ARTS) fit on the device (k_angular.inc): n_epochs x (leaves -> physical parameters and f_e, form factor, ATS
// chain, loss and seed, ATS adjoint, form-factor adjoint, chain rule, optimiser + early stop), all enqueued on the handle's
// stream.  The stages are prepared once, for one lineout and all its points -- every refusal before anything is allocated,
// every buffer before the first launch; the epochs only enqueue, nothing synchronises.  The generator: AngGen, gen_forward, gen_adjoint.
int tsff_angular_fit(tsff_handle* h, const tsff_angular_spec* sp, double* leaves, const double* gen_data, const double* e_data,
                     const double* noise_e, const double* wcol, const double* e_amps, double* moments, double* best, int32_t* ctl,
                     double* loss_hist, double* best_hist) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!sp || !leaves || !e_data || !noise_e || !wcol || !e_amps || !moments || !best || !ctl || sp->n_epochs < 0 || sp->epoch0 < 0 ||
      (int64_t)sp->epoch0 + sp->n_epochs > 0x7fffffffLL || sp->n_active < 0 || sp->n_active > h->S.NP ||
      (sp->n_active > 0 && !sp->active_slots))
    return fail(h, -1, "bad argument");
  if (h->ats_npx == 0) return fail(h, -2, "tsff_ats_setup has not been called");
  if (h->fe_mode != TSFF_FE_PER_LINEOUT) return fail(h, -2, "tsff_angular_fit needs fe_mode == TSFF_FE_PER_LINEOUT");
  AngGen G;
  if (int rc = ang_gen_describe(h, sp, gen_data, G)) return rc;
  if (sp->method != TSFF_ANG_ADAM && sp->method != TSFF_ANG_RMSPROP) return fail(h, -2, "unknown optimiser %d", sp->method);
  if (sp->loss_method < 0 || sp->loss_method > 3) return fail(h, -2, "unknown loss method %d", sp->loss_method);
  uint8_t gm[kNP_MAX];
  if (int rc = check_slots(h, sp->active_slots, sp->n_active, gm, G.m_leaf)) return rc;
  const long n = sp->n_active + G.n_table;
  if (n < 1) return fail(h, -1, "nothing to train");
  const int gen = sp->generator, nv = sp->nv, npts = h->S.npts, NA = h->S.n_angles, NP = h->S.NP;
  const int rows = h->ats_row_end - h->ats_row_start, nJ = npts / h->ats_lam_step;
  if (nJ > TSFF_NBINS) return fail(h, -2, "more than %d wavelength resolution units per row", TSFF_NBINS);
  const bool want_dm = gm[TSFF_P_M] != 0, train_table = gen == TSFF_ANG_ARB2V;
  const size_t nP = (size_t)h->S.G * npts * NA, nimg = (size_t)rows * nJ;
  // the stages of an epoch: the form factor (2-D: saving), the ATS chain and its reverse, the form-factor adjoint (with the
  // table or f_e adjoint when the generator chains it back, or when m is a leaf)
  FormFactorPlan ff;
  FormFactorAdjPlan ffa;
  FormFactor2dPlan ff2;
  FormFactor2dAdjPlan ff2a;
  auto prepare_stages = [&](bool dry) {
    int rc = G.two_d ? form_factor_2d_prepare(h, 0, nv, true, 1, 0, -1, true, ff2, dry) : form_factor_prepare(h, 0, 1, ff, dry);
    if (!rc) rc = ats_prepare(h, false, dry);
    if (!rc) rc = ats_prepare(h, true, dry);
    if (!rc) rc = G.two_d ? form_factor_2d_adj_prepare(h, 0, nv, 1, 0, (long)nP, G.fe_bar, ff2a, dry)
                          : form_factor_adj_prepare(h, 0, 1, want_dm || G.fe_bar, ffa, dry);
    return rc;
  };
  int rc = prepare_stages(true);
  if (rc || sp->n_epochs == 0) return rc;
  // scratch: phys | fe | dfe (2 nv) | aux | P | ThryE | Ebar | Pbar | gphys | gfe | grad | loss | its partial sums | the generator's
  const size_t nfe = G.two_d ? (size_t)nv * nv : (size_t)nv;
  size_t off = 0;
  auto take = [&](size_t k) { const size_t o = off; off += (k + 1) & ~(size_t)1; return o; };
  const size_t o_phys = take(NP + 1), o_fe = take(nfe), o_dfe = take(2 * (size_t)nv), o_aux = take(4), o_P = take(nP),
               o_E = take(nimg), o_Eb = take(nimg), o_Pb = take(nP), o_gp = take(NP), o_gfe = take(nfe), o_grad = take(n),
               o_loss = take(1), o_part = take(kAngLossBlocks), o_gen = take(G.ws_doubles);
  TSFF_ENSURE(h, h->ang_ws, off * sizeof(double));
  if (sp->n_active > 0 && (rc = upload_slots(h, sp->active_slots, sp->n_active))) return rc;
  if ((rc = prepare_stages(false))) return rc;
  double* ws = h->ang_ws.as<double>();
  double *phys = ws + o_phys, *fe = ws + o_fe, *dfe = ws + o_dfe, *aux = ws + o_aux, *P = ws + o_P, *E = ws + o_E, *Eb = ws + o_Eb,
         *Pb = ws + o_Pb, *gphys = ws + o_gp, *gfe = ws + o_gfe, *grad = ws + o_grad, *lossv = ws + o_loss,
         *lpart = ws + o_part, *gws = ws + o_gen;
  const double *table = G.fe_is_data ? gen_data : fe, *theta = leaves + NP;
  const int n_hist = NP + (int)G.hist_tail;
  const double dv2 = sp->dvx * sp->dvx, cvjp = 1.0 / dv2, ln10 = std::log(10.0);
  // the optimiser's scalars as tree.Adam / tree.RMSProp compute them in Python (1 - b1, -lr, 1 - b1**count with glibc pow)
  const bool adam = sp->method == TSFF_ANG_ADAM;
  const double b1 = sp->b1, b2 = adam ? sp->b2 : sp->decay, omb1 = 1.0 - b1, omb2 = 1.0 - b2, neg_lr = -sp->lr;
  const int* act = sp->n_active > 0 ? h->act.as<int>() : nullptr;
  const double* ampb = ats_amp_bar(h);
  const unsigned nloss = (unsigned)std::min<long>(kAngLossBlocks, ((long)nimg + kThreads - 1) / kThreads);   // (a fixed partition)
  for (int t = 0; t < sp->n_epochs; ++t) {
    const int epoch = sp->epoch0 + t;
    TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_ang_leaves, dim3(1), dim3(kThreads), 0, h->stream, h->S, (const double*)leaves, gen,
                    (int)sp->learn_log, nv, gen_data, sp->dvx, dv2, (int)want_dm, phys, fe, dfe, aux);
    if ((rc = gen_forward(h, gen, G.sph, sp->n_gen, gen_data, nv, sp->dvx, theta, gws, fe))) return rc;
    rc = G.two_d ? form_factor_2d_enqueue(h, ff2, phys, table, sp->ud_angle, sp->va_angle, P) : form_factor_enqueue(h, ff, phys, fe, P);
    if (rc) return rc;
    if ((rc = ats_spectrum_enqueue(h, P, e_amps, 0.0, 0.0, 0.0, phys, E))) return rc;
    TSFF_LAUNCH0(h, k_ang_loss, dim3(nloss), dim3(kThreads), 0, h->stream, (const double*)E, noise_e, e_data, wcol, rows, nJ,
                 (int)sp->loss_method, sp->un, Eb, lpart);
    TSFF_LAUNCH0(h, k_ang_loss_sum, dim3(1), dim3(kThreads), 0, h->stream, (const double*)lpart, (int)nloss, lossv);
    TSFF_HIP(h, hipGetLastError());
    if ((rc = ats_adjoint_enqueue(h, P, e_amps, 0.0, 0.0, 0.0, phys, Eb, Pb))) return rc;
    rc = G.two_d ? form_factor_2d_adj_enqueue(h, ff2a, phys, table, sp->ud_angle, sp->va_angle, h->proj.as<double>(), Pb, gphys, gfe)
                 : form_factor_adj_enqueue(h, ffa, phys, fe, Pb, gphys, gfe);
    if (rc) return rc;
    TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_ang_chain, dim3(1), dim3(kThreads), 0, h->stream, h->S, (const double*)leaves, (const double*)gphys,
                    ampb, rows, (const double*)gfe, want_dm ? (const double*)dfe : nullptr, nv, (int)train_table,
                    (int)sp->learn_log, nv, (const double*)aux, cvjp, ln10, act, (int)sp->n_active, grad);
    if ((rc = gen_adjoint(h, gen, G.sph, sp->n_gen, gen_data, nv, sp->dvx, theta, gfe, gws, grad + sp->n_active))) return rc;
    const double count = (double)epoch + 1;
    const double c1 = 1.0 - std::pow(b1, count), c2 = 1.0 - std::pow(b2, count);
    TSFF_LAUNCH0(h, k_ang_opt, dim3(1), dim3(kThreads), 0, h->stream, (const double*)lossv, (const double*)grad, act, (int)sp->n_active,
                 NP, G.n_table, leaves, moments, adam ? 0 : 1, b1, omb1, b2, omb2, neg_lr, c1, c2, sp->eps, ctl, best, epoch,
                 loss_hist ? loss_hist + t : nullptr, best_hist ? best_hist + (size_t)t * n_hist : nullptr, n_hist);
    TSFF_HIP(h, hipGetLastError());
  }
  return 0;
}

int tsff_lbfgs_state_size(int32_t B, int32_t n_active, int32_t maxcor, int64_t* n_doubles) {
  if (B < 1 || n_active < 1 || maxcor < 1 || maxcor > kLbMaxCor || !n_doubles) return -1;
  *n_doubles = lb_vec_offset(maxcor) + (int64_t)(4 + 2 * maxcor) * n_active * B;
  return 0;
}

// the 1-D L-BFGS-B fit on the device (k_lbfgs.inc): prepare_packed_fit, then n_evals x (loss_grad_enqueue + lb_passes(maxcor)
// launches of k_lbfgs_step on lb_blocks(n) workgroups), all enqueued on the handle's stream
int tsff_lbfgs_fit(tsff_handle* h, double* params, const double* fe, const double* e_data, const double* i_data, const double* e_amps,
                   const double* i_amps, const double* noise_e, const double* noise_i, int32_t B, const double* weights,
                   const int32_t* active_slots, int32_t n_active, int32_t n_evals, const double* opts, double* state, int64_t n_state,
                   double* f_hist, int32_t* info) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!params || B < 1 || !weights || !active_slots || !opts || !state || n_active < 1 || n_active > h->S.NP || n_evals < 0)
    return fail(h, -1, "bad argument");
  const double maxcor_d = opts[0], ftol = opts[1], gtol = opts[2], maxiter_d = opts[3], maxfun_d = opts[4], maxls_d = opts[5];
  auto whole = [](double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); };
  if (!whole(maxcor_d, 1, kLbMaxCor) || !whole(maxiter_d, 0, 0x7fffffff) || !whole(maxfun_d, 0, 0x7fffffff) ||
      !whole(maxls_d, 1, 0x7fffffff) || !(ftol >= 0.0) || !(gtol >= 0.0))
    return fail(h, -1, "bad option (opts = maxcor in [1, %d], ftol >= 0, gtol >= 0, maxiter >= 0, maxfun >= 0, maxls >= 1)", kLbMaxCor);
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  PackedFit F;
  int rc = check_slots(h, active_slots, n_active, F.gm, h->fe_mode == TSFF_FE_DLM);
  if (!rc) rc = check_batch(h, b, true);
  if (rc) return rc;
  const int maxcor = (int)maxcor_d;
  int64_t need = 0;
  if (tsff_lbfgs_state_size(B, n_active, maxcor, &need) || n_state < need)
    return fail(h, -1, "state holds %lld doubles, needs %lld", (long long)n_state, (long long)need);
  if (n_evals == 0) return 0;
  if ((rc = prepare_packed_fit(h, F, b, weights, active_slots, n_active))) return rc;
  const long n = (long)n_active * B;
  // mainlb's tol = factr * epsmch with the wrapper's factr = ftol / eps (lbfgs.Lbfgs)
  const double tol = (ftol / kLbEps) * kLbEps;
  const int maxiter = (int)maxiter_d, maxfun = (int)maxfun_d, maxls = (int)maxls_d;
  const double* packed = F.po.packed;
  const dim3 grid((unsigned)lb_blocks(n));
  const int passes = lb_passes(maxcor);
  for (int t = 0; t < n_evals; ++t) {
    if ((rc = loss_grad_enqueue(h, F.c))) return rc;
    for (int k = 0; k < passes; ++k) {   // (a pass the evaluation does not need returns at once)
      TSFF_LAUNCH0(h, k_lbfgs_step, grid, dim3(kLbThreads), 0, h->stream, packed, weights[0], weights[1], weights[2],
                   h->act.as<int>(), (int)n_active, (int)B, h->S.NP, params, state, maxcor, tol, gtol, maxiter, maxfun, maxls, k,
                   f_hist ? f_hist + t : nullptr, info);
      TSFF_HIP(h, hipGetLastError());
    }
  }
  return 0;
}

int tsff_pack_fe_rows(tsff_handle* h, const double* loss_terms, const double* grad, const double* grad_fe, int32_t B,
                      const int32_t* active_slots, int32_t n_active, int64_t B_global, int64_t b_offset, double* packed) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!loss_terms || !grad || !grad_fe || !active_slots || !packed || B < 1 || n_active < 0 || n_active > h->S.NP || b_offset < 0 ||
      b_offset + B > B_global)
    return fail(h, -1, "bad argument");
  for (int k = 0; k < n_active; ++k)
    if (active_slots[k] < 0 || active_slots[k] >= h->S.NP) return fail(h, -1, "active slot %d out of range", (int)active_slots[k]);
  if (int rc = upload_slots(h, active_slots, n_active)) return rc;
  const long tiles = ((B_global + 31) / 32) * ((n_active + h->S.nvx + 31) / 32);
  TSFF_LAUNCH0(h, k_pack_fe_rows, dim3((unsigned)std::max<long>(1, std::min<long>(tiles, 2048))), dim3(kThreads), 0, h->stream, loss_terms, grad,
                     h->S.NP, grad_fe, h->S.nvx, (int)B, h->act.as<int>(), (int)n_active, (long)B_global, (long)b_offset, packed);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// exact per-lineout Hessian (k_hessian.inc): persistent k_hess_pairs over (lineout, pair of active leaves), k_hess_finish,
// k_loss_reduce -- the same launches whatever the number of active leaves
constexpr int kHessMaxWG = 1024;   // persistent workgroups of k_hess_pairs (bounds the scratch: 4 npts doubles each)
int tsff_loss_hess(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                   const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                   const double* weights, const int32_t* active_slots, int32_t n_active, double* loss_terms, double* grad,
                   double* hess) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!weights || !active_slots || !loss_terms || !grad || !hess || n_active < 1 || n_active > h->S.NP)
    return fail(h, -1, "bad argument");
  uint8_t gm[kNP_MAX];
  if (int rc = check_slots(h, active_slots, n_active, gm, h->fe_mode == TSFF_FE_DLM)) return rc;
  HessArgs A{};
  A.n = n_active;
  A.npair = n_active * (n_active + 1) / 2;
  std::copy(active_slots, active_slots + n_active, A.slot);
  A.with_m = gm[TSFF_P_M];
  if ((long)B * A.npair > 0x7fffffffL) return fail(h, -1, "too many (lineout, pair) tasks");
  A.tasks = B * A.npair;
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  if (int rc = check_batch(h, b, true)) return rc;
  const size_t smem = sizeof(double) * hess_smem_doubles(h->S, A.with_m != 0);
  if (smem > kLdsLimit)
    return fail(h, -2, "tsff_loss_hess: LDS budget exceeded (%zu B with nvx = %d%s): reduce nvx", smem, h->S.nvx,
                A.with_m ? " and the DLM order as a leaf" : "");
  // every buffer of the call before the first launch (fill_call enqueues the tables)
  const int nwg = std::min(A.tasks, kHessMaxWG);
  if (A.with_m) {
    const size_t nvx = h->S.nvx;
    TSFF_ENSURE(h, h->htmm, (size_t)B * nvx * sizeof(double2));
    TSFF_ENSURE(h, h->Xmm, (size_t)B * 4 * kNXi1 * sizeof(double));
    TSFF_ENSURE(h, h->cstmm, (size_t)B * 2 * sizeof(double));
    TSFF_ENSURE(h, h->Wmm, (size_t)B * kNXi2 * sizeof(double));
    TSFF_ENSURE(h, h->Wmm_unused, (size_t)B * kNXi2 * sizeof(double));
  }
  TSFF_ENSURE(h, h->hws, (size_t)nwg * 4 * h->S.npts * sizeof(double));
  TSFF_ENSURE(h, h->hout, (size_t)A.tasks * 12 * sizeof(double));
  int rc = ensure_workspace(h, B);
  if (rc) return rc;
  KCall K{};
  if ((rc = fill_call(h, K, b, nullptr, nullptr))) return rc;
  if (A.with_m) {   // second m-derivative tables: k_hess_mtab, then the shipped W-table GEMM on its rows
    const size_t nvx = h->S.nvx;
    const size_t smem_t = sizeof(double2) * 6 * nvx + sizeof(double) * (nvx + 2 * kNXi1 + 8);
    TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_hess_mtab, dim3(B), dim3(kThreads), smem_t, h->stream, h->S, params, K.ht, K.htm, h->htmm.as<double2>(),
                    h->Xmm.as<double>(), h->cstmm.as<double>());
    TSFF_HIP(h, hipGetLastError());
    const int nM = (B + kGM / 4 - 1) / (kGM / 4);
    dim3 wgrid(8 * ((nM + 7) / 8) * ((kNXi2 + kGNw - 1) / kGNw));
    TSFF_LAUNCH0(h, k_wgemm_w, wgrid, dim3(kThreads), kWgemmWSmem, h->stream, h->S.lg, h->Xmm.as<double>(), h->cstmm.as<double>(),
                 h->S.xi2, (int)B, h->Wmm.as<double>(), h->Wmm_unused.as<double>(), h->kw_lo, h->kw_hi);
    TSFF_HIP(h, hipGetLastError());
    A.htmm = h->htmm.as<double2>();
    A.Wmm = h->Wmm.as<double>();
  }
  TSFF_LAUNCH_FN(h, hess_pairs_kernel(h->n_ion), ("k_hess_pairs", h->n_ion), dim3(nwg), dim3(kThreads), smem, h->stream, h->S, K, A,
                 h->hws.as<double>(), h->hout.as<double>());
  TSFF_HIP(h, hipGetLastError());
  TSFF_LAUNCH0(h, k_hess_finish, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, h->stream, h->hout.as<double>(), A, (int)B,
               weights[0], weights[1], weights[2], K.lpart, grad, hess);
  TSFF_HIP(h, hipGetLastError());
  TSFF_LAUNCH0(h, k_loss_reduce, dim3(1), dim3(kThreads), 0, h->stream, K.lpart, (int)B, loss_terms, (const double*)nullptr, 0L,
               (double*)nullptr);
  TSFF_HIP(h, hipGetLastError());
  return 0;
}

// ---- exact Hessian of the angular (ARTS) loss: second-order forward mode of the form factor (k_ffhess.inc: one workgroup column
// per pair of leaves that reach the form factor), the ARTS chain at second order (the linear stages on every derivative image, the
// two row normalisations by k_ats_rownorm_jvp2 / k_ats_resunit_jvp2), k_ats_hess_reduce.  The value image is the shipped forward's
// (k_form_factor on the physical parameters k_ang_leaves stages: tsff_form_factor's bits); the first-order images come from the
// diagonal pairs of the same k_ffhess launch.  prepare: every refusal and every buffer; enqueue: launches only.
// workgroups per CU the grid of k_ffhess aims at: angle chunks = min(n_angles, kFfhessWGPerCU x CUs / pairs).
// The 4 is angle_chunks' figure, taken over; it has not been tuned for this kernel.
constexpr int kFfhessWGPerCU = 4;
struct AngHessCall {
  const double *leaves, *fe, *e_data, *noise_e, *e_amps, *wcol;
  int method = 0, n = 0;
  double *loss, *grad, *hess, *gn, *E, *E1, *E2, *phys_out;
};
struct AngHessPlan {
  int n = 0, npair = 0;
  int slot[kNP_MAX];       // the active slots, ravel order
  int ff[kNP_MAX];         // per active leaf: its index among the leaves that reach the form factor, or -1 (an amplitude)
  FfhessArgs A{};
  size_t smem = 0;
  dim3 grid;
  // the workspace (doubles into ahess_ws)
  size_t o_phys = 0, o_P = 0, o_P1 = 0, o_P2 = 0, o_Md = 0, o_Bd = 0, o_Yd = 0, o_E = 0, o_E1 = 0, o_E2 = 0;
};

static int ang_hess_prepare(tsff_handle* h, const AngHessCall& c, const int32_t* active_slots, AngHessPlan& p) {
  uint8_t gm[kNP_MAX];
  if (int rc = check_slots(h, active_slots, c.n, gm, h->fe_mode == TSFF_FE_DLM)) return rc;
  if (int rc = check_fe(h, c.fe)) return rc;
  if (int rc = ats_jvp_prepare(h)) return rc;   // (tsff_ats_setup has run; the row statistics and the three images of a derivative)
  p.n = c.n; p.npair = c.n * (c.n + 1) / 2;
  FfhessArgs& A = p.A;
  A.nf = 0;
  for (int k = 0; k < c.n; ++k) {
    const int s = active_slots[k];
    p.slot[k] = s;
    const bool amp = s == TSFF_P_AMP1 || s == TSFF_P_AMP2 || s == TSFF_P_AMP3;   // (the amplitudes never reach the form factor)
    p.ff[k] = amp ? -1 : A.nf;
    if (!amp) A.slot[A.nf++] = s;
  }
  A.npair = A.nf * (A.nf + 1) / 2;
  A.with_m = gm[TSFF_P_M];
  p.smem = sizeof(double) * ffhess_smem_doubles(h->S, A.with_m != 0);
  if (p.smem > kLdsLimit)
    return fail(h, -2, "tsff_angular_loss_hess: LDS budget exceeded (%zu B with nvx = %d, %d angles%s): reduce nvx", p.smem, h->S.nvx,
                h->S.n_angles, A.with_m ? " and the DLM order as a leaf" : "");
  const int want = kFfhessWGPerCU * h->ncu2d();
  p.grid = dim3(std::max(A.npair, 1), (unsigned)std::max(1, std::min(h->S.n_angles, want / std::max(A.npair, 1))));
  if (int rc = ensure_workspace(h, 1)) return rc;
  if (A.with_m) {
    const size_t nvx = h->S.nvx;
    TSFF_ENSURE(h, h->htmm, nvx * sizeof(double2));
    TSFF_ENSURE(h, h->Xmm, (size_t)4 * kNXi1 * sizeof(double));
    TSFF_ENSURE(h, h->cstmm, (size_t)2 * sizeof(double));
    TSFF_ENSURE(h, h->Wmm, (size_t)kNXi2 * sizeof(double));
    TSFF_ENSURE(h, h->Wmm_unused, (size_t)kNXi2 * sizeof(double));
  }
  const size_t pimg = (size_t)h->S.G * h->S.npts * h->S.n_angles, aimg = (size_t)h->ats_npx * h->S.npts;
  const size_t rimg = (size_t)(h->ats_row_end - h->ats_row_start) * (h->S.npts / h->ats_lam_step);
  size_t o = 0;
  auto carve = [&](size_t nd) { const size_t at = o; o += (nd + 1) & ~(size_t)1; return at; };
  p.o_phys = carve(kNP_MAX + 1);
  p.o_P = carve(pimg); p.o_P1 = carve(A.nf * pimg); p.o_P2 = carve(A.npair * pimg);
  p.o_Md = carve(A.nf * aimg); p.o_Bd = carve(A.nf * aimg); p.o_Yd = carve(A.nf * aimg);
  p.o_E = carve(c.E ? 0 : rimg); p.o_E1 = carve(c.E1 ? 0 : c.n * rimg); p.o_E2 = carve(c.E2 ? 0 : p.npair * rimg);
  TSFF_ENSURE(h, h->ahess_ws, std::max<size_t>(o, 2) * sizeof(double));
  return 0;
}

static int ang_hess_enqueue(tsff_handle* h, const AngHessCall& c, AngHessPlan& p) {
  const int npts = h->S.npts, npx = h->ats_npx, rows = h->ats_row_end - h->ats_row_start, nJ = npts / h->ats_lam_step;
  const size_t pimg = (size_t)h->S.G * npts * h->S.n_angles, aimg = (size_t)npx * npts, rimg = (size_t)rows * nJ;
  double* ws = h->ahess_ws.as<double>();
  double* phys = c.phys_out ? c.phys_out : ws + p.o_phys;
  double *P = ws + p.o_P, *P1 = ws + p.o_P1, *P2 = ws + p.o_P2, *Md = ws + p.o_Md, *Bd = ws + p.o_Bd, *Yd = ws + p.o_Yd;
  double* E = c.E ? c.E : ws + p.o_E;
  double* E1 = c.E1 ? c.E1 : ws + p.o_E1;
  double* E2 = c.E2 ? c.E2 : ws + p.o_E2;
  FfhessArgs& A = p.A;
  if (int rc = timing_begin(h)) return rc;
  KCall K{};
  K.params = c.leaves; K.B = 1;
  if (int rc = prepare_tables(h, c.leaves, c.fe, 1, K)) return rc;
  if (A.with_m) {   // second m-derivative tables, as tsff_loss_hess builds them: k_hess_mtab, then the shipped W-table GEMM on its rows
    const size_t nvx = h->S.nvx;
    const size_t smem_t = sizeof(double2) * 6 * nvx + sizeof(double) * (nvx + 2 * kNXi1 + 8);
    TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_hess_mtab, dim3(1), dim3(kThreads), smem_t, h->stream, h->S, c.leaves, K.ht, K.htm, h->htmm.as<double2>(),
                    h->Xmm.as<double>(), h->cstmm.as<double>());
    TSFF_HIP(h, hipGetLastError());
    const int nM = (1 + kGM / 4 - 1) / (kGM / 4);
    dim3 wgrid(8 * ((nM + 7) / 8) * ((kNXi2 + kGNw - 1) / kGNw));
    TSFF_LAUNCH0(h, k_wgemm_w, wgrid, dim3(kThreads), kWgemmWSmem, h->stream, h->S.lg, h->Xmm.as<double>(), h->cstmm.as<double>(),
                 h->S.xi2, 1, h->Wmm.as<double>(), h->Wmm_unused.as<double>(), h->kw_lo, h->kw_hi);
    TSFF_HIP(h, hipGetLastError());
    A.htmm = h->htmm.as<double2>();
    A.Wmm = h->Wmm.as<double>();
  }
  // the physical parameters (k_ang_leaves with a generator it has no table for: the parameters only) and the value image
  TSFF_LAUNCH_ION(h, TSFF_MAX_ION, k_ang_leaves, dim3(1), dim3(kThreads), 0, h->stream, h->S, c.leaves, (int)TSFF_ANG_ARB1V, 0, 0,
                  (const double*)nullptr, 0.0, 0.0, 0, phys, (double*)nullptr, (double*)nullptr, (double*)nullptr);
  KCall Kp = K;
  Kp.params = phys;
  TSFF_LAUNCH_FN(h, form_factor_kernel(h->n_ion), ("k_form_factor", h->n_ion), dim3(1, angle_chunks(h, 1)), dim3(kThreads), h->smem_spectrum,
                 h->stream, h->S, Kp, 0, h->S.omgs[0], npts, P);
  TSFF_HIP(h, hipGetLastError());
  if (A.nf > 0) {
    A.P1 = P1; A.P2 = P2;
    TSFF_LAUNCH_FN(h, ffhess_kernel(h->n_ion), ("k_ffhess", h->n_ion), p.grid, dim3(kThreads), p.smem, h->stream, h->S, K, A, 0, h->S.omgs[0], npts);
    TSFF_HIP(h, hipGetLastError());
  }
  // ---- the ARTS chain: value, first order per leaf that reaches the form factor, second order per pair ----
  dim3 block(kThreads), grid((npts + kThreads - 1) / kThreads, npx);
  double* Bm = h->ats_B.as<double>();
  double* Mt = h->ats_C.as<double>();
  double* At = h->ats_D.as<double>();
  double* Bt = h->ats_E.as<double>();
  double* stats = h->ats_stats.as<double>();
  const double *wts = h->ats_w.as<double>(), *ta = h->ats_ta.as<double>(), *tl = h->ats_tl.as<double>(), *lam_nm = h->ats_lam.as<double>();
  ats_forward_chain(h, P);
  TSFF_LAUNCH0(h, k_ats_rowstats, dim3(npx), block, 0, h->stream, h->ats_M.as<double>(), Bm, npts, stats);
  TSFF_LAUNCH0(h, k_ats_rownorm, dim3(npx), block, 0, h->stream, h->ats_M.as<double>(), Bm, npts);
  TSFF_LAUNCH0(h, k_ats_resunit, dim3(rows), block, 0, h->stream, Bm, lam_nm, npts, h->ats_lam_step, h->ats_ang_step, h->ats_row_start,
               c.e_amps, 0.0, 0.0, 0.0, (const double*)phys, E);
  TSFF_HIP(h, hipGetLastError());
  for (int i = 0; i < A.nf; ++i) {
    double *Mi = Md + i * aimg, *Bi = Bd + i * aimg, *Yi = Yd + i * aimg;
    TSFF_LAUNCH0(h, k_ats_weights, grid, block, 0, h->stream, P1 + i * pimg, wts, h->S.filt, h->S.G, npts, h->S.n_angles, npx, Mi);
    TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, Mi, ta, h->ats_nta, h->ats_offa, 1, npx, npts, At);
    TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, At, tl, h->ats_ntl, h->ats_offl, 0, npx, npts, Bi);
    TSFF_HIP(h, hipMemcpyAsync(Yi, Bi, aimg * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    TSFF_LAUNCH0(h, k_ats_rownorm_jvp, dim3(npx), block, 0, h->stream, Bm, stats, Mi, npts, Yi);
    TSFF_HIP(h, hipGetLastError());
  }
  int pr = 0;
  for (int a = 0; a < p.n; ++a)
    for (int cc = a; cc < p.n; ++cc, ++pr) {
      const int fa = p.ff[a], fc = p.ff[cc];
      const double* Yac = nullptr;
      if (fa >= 0 && fc >= 0) {   // (a pair with an amplitude has P2 = 0: no form-factor task, no image)
        const int q = fa * A.nf - fa * (fa - 1) / 2 + (fc - fa);
        TSFF_LAUNCH0(h, k_ats_weights, grid, block, 0, h->stream, P2 + q * pimg, wts, h->S.filt, h->S.G, npts, h->S.n_angles, npx, Mt);
        TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, Mt, ta, h->ats_nta, h->ats_offa, 1, npx, npts, At);
        TSFF_LAUNCH0(h, k_ats_conv, grid, block, 0, h->stream, At, tl, h->ats_ntl, h->ats_offl, 0, npx, npts, Bt);
        TSFF_LAUNCH0(h, k_ats_rownorm_jvp2, dim3(npx), block, 0, h->stream, Bm, stats, Md + fa * aimg, Md + fc * aimg, Mt, Bd + fa * aimg,
                     Bd + fc * aimg, npts, Bt);
        Yac = Bt;
      }
      TSFF_LAUNCH0(h, k_ats_resunit_jvp2, dim3(rows), block, 0, h->stream, h->S, c.leaves, (const double*)phys, p.slot[a], p.slot[cc], Bm,
                   fa >= 0 ? Yd + fa * aimg : (const double*)nullptr, fc >= 0 ? Yd + fc * aimg : (const double*)nullptr, Yac, lam_nm, npts,
                   h->ats_lam_step, h->ats_ang_step, h->ats_row_start, c.e_amps, a == cc ? E1 + a * rimg : (double*)nullptr, E2 + pr * rimg);
      TSFF_HIP(h, hipGetLastError());
    }
  TSFF_LAUNCH0(h, k_ats_hess_reduce, dim3(p.npair), block, 0, h->stream, E, E1, E2, c.noise_e, c.e_data, c.wcol, rows, nJ, c.method, p.n,
               c.loss, c.grad, c.hess, c.gn);
  TSFF_HIP(h, hipGetLastError());
  return timing_end(h);
}

int tsff_angular_loss_hess(tsff_handle* h, const double* leaves, const double* fe, const int32_t* active_slots, int32_t n_active,
                           const double* e_data, const double* noise_e, const double* e_amps, const double* wcol, int32_t loss_method,
                           double* loss, double* grad, double* hess, double* gn, double* E, double* E1, double* E2, double* phys) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!leaves || !active_slots || !e_data || !e_amps || !wcol || !loss || !grad || !hess || !gn) return fail(h, -1, "bad argument");
  if (n_active < 1 || n_active > h->S.NP) return fail(h, -1, "bad argument: n_active = %d", (int)n_active);
  if (loss_method < TSFF_LOSS_L2 || loss_method > TSFF_LOSS_POISSON) return fail(h, -1, "bad argument: loss_method = %d", (int)loss_method);
  if (!h->S.load[0]) return fail(h, -2, "tsff_angular_loss_hess needs the electron feature (load_ele)");
  AngHessCall c{leaves, fe, e_data, noise_e, e_amps, wcol, (int)loss_method, (int)n_active, loss, grad, hess, gn, E, E1, E2, phys};
  AngHessPlan p;
  if (int rc = ang_hess_prepare(h, c, active_slots, p)) return rc;
  return ang_hess_enqueue(h, c, p);
}

// Jacobian of the spectra and Gauss-Newton curvature (k_jacobian.inc): the deck's table kernels, then k_jac_sweep on persistent
// workgroups (one lineout per task); tsff_loss_gauss_newton adds k_loss_reduce (a call with loss_terms).  jac_prepare holds
// everything that can refuse, allocate or upload; jac_enqueue only launches.
constexpr int kJacMaxWG = 1024;   // persistent workgroups of k_jac_sweep (bounds the row scratch: n_active x 1024 doubles each)
struct JacCall {
  Batch b;
  JacArgs A{};
  double* loss_terms = nullptr;
  int width = 0, nwg = 0;   // jac_prepare: tangents per group, workgroups
  bool rows = false;        // jac_prepare: the row form of the sweep
  size_t smem = 0;
};

static int jac_prepare(tsff_handle* h, JacCall& c, const int32_t* active_slots, int n_active, const char* who) {
  uint8_t gm[kNP_MAX];
  if (int rc = check_slots(h, active_slots, n_active, gm, h->fe_mode == TSFF_FE_DLM)) return rc;
  JacArgs& A = c.A;
  A.n = n_active;
  std::copy(active_slots, active_slots + n_active, A.slot);
  A.with_m = gm[TSFF_P_M];
  if (int rc = check_batch(h, c.b, A.want_gn != 0)) return rc;
  if (A.want_gn && h->S.loss_method == TSFF_LOSS_L1)
    return fail(h, -2, "%s: loss_method l1 has l'' = 0, its Gauss-Newton matrix vanishes (use l2, log-cosh or poisson)", who);
  // three tangents per group when the leaves and the LDS allow it, else one
  c.width = n_active == 1 ? 1 : 3;
  c.smem = sizeof(double) * jac_smem_doubles(h->S, A.with_m != 0, c.width);
  if (c.smem > kLdsLimit) {
    c.width = 1;
    c.smem = sizeof(double) * jac_smem_doubles(h->S, A.with_m != 0, 1);
  }
  if (c.smem > kLdsLimit)
    return fail(h, -2, "%s: LDS budget exceeded (%zu B with nvx = %d, npts = %d%s): reduce nvx or points_per_pixel", who, c.smem, h->S.nvx,
                h->S.npts, A.with_m ? " and the DLM order as a leaf" : "");
  c.nwg = std::min(c.b.B, kJacMaxWG);
  // the row form where the reverse of the pair sweeps exists: 1-2 ion species, one gradient point, the DLM order not a leaf, both
  // features through their instrument response, and three tangents per group
  const size_t smem_rows = sizeof(double) * jac_rows_smem_doubles(h->S, n_active);
  c.rows = c.width == 3 && h->n_ion <= kFusedMaxIon && h->S.G == 1 && !A.with_m && !h->S.raw[0] && !h->S.raw[1] && smem_rows <= kLdsLimit;
  if (c.rows) c.smem = smem_rows;
  const size_t xg_doubles = c.rows ? (size_t)(1 + n_active) * h->S.npts : 0;
  TSFF_ENSURE(h, h->jrows, (size_t)c.nwg * (xg_doubles + (A.want_gn ? (size_t)n_active * TSFF_NBINS : 0)) * sizeof(double));
  return ensure_workspace(h, c.b.B);
}

static int jac_enqueue(tsff_handle* h, JacCall& c) {
  KCall K{};
  if (int rc = fill_call(h, K, c.b, nullptr, nullptr)) return rc;
  const size_t xg_doubles = c.rows ? (size_t)c.nwg * (1 + c.A.n) * h->S.npts : 0;   // (the row form's spectra in front of the rows)
  c.A.xg = c.rows ? h->jrows.as<double>() : nullptr;
  c.A.rows = c.A.want_gn ? h->jrows.as<double>() + xg_doubles : nullptr;
  TSFF_LAUNCH_FN(h, jac_kernel(h->n_ion, c.width, c.rows), ("k_jac_sweep", h->n_ion, c.width, c.rows), dim3(c.nwg), dim3(kThreads), c.smem, h->stream,
                 h->S, K, c.A);
  TSFF_HIP(h, hipGetLastError());
  if (c.A.want_gn && c.loss_terms) {
    TSFF_LAUNCH0(h, k_loss_reduce, dim3(1), dim3(kThreads), 0, h->stream, K.lpart, (int)c.b.B, c.loss_terms, (const double*)nullptr, 0L,
                 (double*)nullptr);
    TSFF_HIP(h, hipGetLastError());
  }
  return 0;
}

int tsff_spectrum_jacobian(tsff_handle* h, const double* params, const double* fe, const double* e_amps, const double* i_amps, int32_t B,
                           const int32_t* active_slots, int32_t n_active, double* jac_e, double* jac_i) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!active_slots || (!jac_e && !jac_i) || n_active < 1 || n_active > h->S.NP) return fail(h, -1, "bad argument");
  if ((jac_e && !h->S.load[0]) || (jac_i && !h->S.load[1]))
    return fail(h, -1, "tsff_spectrum_jacobian: the Jacobian of a feature that is not loaded");
  JacCall c;
  c.b = Batch{params, fe, {nullptr, nullptr}, {e_amps, i_amps}, {nullptr, nullptr}, B};
  c.A.jac[0] = jac_e; c.A.jac[1] = jac_i;
  if (int rc = jac_prepare(h, c, active_slots, n_active, "tsff_spectrum_jacobian")) return rc;
  return jac_enqueue(h, c);
}

int tsff_loss_gauss_newton(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                           const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                           const double* weights, const int32_t* active_slots, int32_t n_active, double* loss_terms, double* grad,
                           double* gn) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!weights || !active_slots || !loss_terms || !grad || !gn || n_active < 1 || n_active > h->S.NP)
    return fail(h, -1, "bad argument");
  JacCall c;
  c.b = Batch{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  c.A.want_gn = 1;
  c.A.grad = grad; c.A.gn = gn;
  std::copy(weights, weights + 3, c.A.w);
  c.loss_terms = loss_terms;
  if (int rc = jac_prepare(h, c, active_slots, n_active, "tsff_loss_gauss_newton")) return rc;
  return jac_enqueue(h, c);
}

int tsff_lm_state_size(int32_t B, int32_t n_active, int64_t* n_doubles) {
  if (B < 1 || n_active < 1 || n_active > kNP_MAX || !n_doubles) return -1;
  *n_doubles = lm_rec_offset(B) + (int64_t)B * lm_rec_doubles(n_active);
  return 0;
}

// the per-lineout Levenberg-Marquardt fit on the device (k_lm.inc): jac_prepare once, then n_evals x (jac_enqueue with want_gn
// + k_lm_step), all enqueued on the handle's stream.  The status words at the head of the state are the sweep's skip flags: a
// lineout that has ended is not evaluated again
int tsff_lm_fit(tsff_handle* h, double* params, const double* fe, const double* e_data, const double* i_data, const double* e_amps,
                const double* i_amps, const double* noise_e, const double* noise_i, int32_t B, const double* weights,
                const int32_t* active_slots, int32_t n_active, int32_t n_evals, const double* opts, double* state, int64_t n_state,
                double* x_hist, double* eval_hist) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!params || B < 1 || !weights || !active_slots || !opts || !state || n_active < 1 || n_active > h->S.NP || n_evals < 0)
    return fail(h, -1, "bad argument");
  const double tau = opts[0], gtol = opts[1], ftol = opts[2], xtol = opts[3], maxiter = opts[4], maxfun = opts[5], lam_max = opts[6];
  auto whole = [](double v) { return v >= 0.0 && v <= 0x7fffffff && v == std::floor(v); };
  if (!(tau > 0.0) || !std::isfinite(tau) || !(gtol >= 0.0) || !(ftol >= 0.0) || !(xtol >= 0.0) || !whole(maxiter) || !whole(maxfun) ||
      !(lam_max > 0.0) || !std::isfinite(lam_max))
    return fail(h, -1, "bad option (opts = tau > 0, gtol >= 0, ftol >= 0, xtol >= 0, maxiter >= 0, maxfun >= 0, lambda_max > 0, all finite)");
  int64_t need = 0;
  if (tsff_lm_state_size(B, n_active, &need) || n_state < need)
    return fail(h, -1, "state holds %lld doubles, needs %lld", (long long)n_state, (long long)need);
  JacCall c;
  c.b = Batch{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  c.A.want_gn = 1;
  std::copy(weights, weights + 3, c.A.w);
  c.A.fit_denoms = h->denom_mode == 0;
  c.A.skip = reinterpret_cast<const int32_t*>(state);
  if (int rc = jac_prepare(h, c, active_slots, n_active, "tsff_lm_fit")) return rc;
  if (n_evals == 0) return 0;
  const size_t n = n_active, row = lm_eval_doubles(n_active);
  TSFF_ENSURE(h, h->lm_ws, (size_t)B * (n + n * n) * sizeof(double));
  c.A.grad = h->lm_ws.as<double>();
  c.A.gn = c.A.grad + (size_t)B * n;
  LmArgs P{};
  P.n = n_active; P.B = B; P.NP = h->S.NP;
  std::copy(active_slots, active_slots + n_active, P.slot);
  std::copy(weights, weights + 3, P.w);
  P.tau = tau; P.gtol = gtol; P.ftol = ftol; P.xtol = xtol; P.maxiter = maxiter; P.maxfun = maxfun; P.lam_max = lam_max;
  const dim3 grid((unsigned)((B + kLmWaves - 1) / kLmWaves));
  const size_t smem = sizeof(double) * kLmWaves * lm_wave_doubles(n_active);
  for (int t = 0; t < n_evals; ++t) {
    if (int rc = jac_enqueue(h, c)) return rc;
    TSFF_LAUNCH0(h, k_lm_step, grid, dim3(kLmWaves * 64), smem, h->stream, P, (const double*)h->lpart.as<double>(), (const double*)c.A.grad,
                 (const double*)c.A.gn, params, state, x_hist ? x_hist + (size_t)t * B * n : nullptr,
                 eval_hist ? eval_hist + (size_t)t * B * row : nullptr);
    TSFF_HIP(h, hipGetLastError());
  }
  return 0;
}

int tsff_array_loss(tsff_handle* h, const double* params, const double* fe, const double* e_data, const double* i_data,
                    const double* e_amps, const double* i_amps, const double* noise_e, const double* noise_i, int32_t B,
                    double* sums, double* sqdev_e, double* sqdev_i, double* ThryE, double* ThryI) {
  DevGuard dg__(h);
  if (!h) return -1;
  if (!sums) return fail(h, -1, "bad argument");
  const Batch b{params, fe, {e_data, i_data}, {e_amps, i_amps}, {noise_e, noise_i}, B};
  SpectrumPlan plan;
  int rc = check_batch(h, b, true);
  if (!rc) rc = size_plan(h, 2, 0, B, plan);
  if (!rc) rc = ensure_workspace(h, B);
  if (rc) return rc;
  KCall K{};
  if ((rc = fill_call(h, K, b, ThryE, ThryI))) return rc;
  K.sqdev[0] = sqdev_e; K.sqdev[1] = sqdev_i;
  K.lpart = sums;
  TSFF_HIP(h, hipMemsetAsync(sums, 0, (size_t)B * 3 * sizeof(double), h->stream));
  return launch_spectrum(h, 2, 0, K, plan);
}

#ifdef TSFF_TRACE
// measurement builds only: device buffer [grid][16] of u64 that k_spectrum_fused stamps (nullptr switches it off)
int tsff_debug_trace(void* devptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(tsff::g_trace_buf), &devptr, sizeof(devptr)) == hipSuccess ? 0 : -5;
}
#endif

}  // extern "C"
