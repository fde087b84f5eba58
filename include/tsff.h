/*
 * tsff.h -- C ABI of libtsff.so, the MI355X (gfx950) Thomson-scattering form-factor engine.
 *
 * Drop-in boundary for ONE hot path of ergodicio/tsadar: the S(k,w) forward model and its
 * parameter gradient over a batch of lineouts.  Citations are file:line in the reference tree.
 *
 *   reference interface                                            replaced by
 *   -------------------------------------------------------------  ---------------------------
 *   FormFactor.__init__            core/physics/form_factor.py:120-161      tsff_create
 *   FormFactor.__call__            core/physics/form_factor.py:163-298      tsff_form_factor
 *   ratintn / ratcen               core/physics/ratintn.py:4-52             tsff_chi_table
 *   DLM1V.__call__                 core/modules/distribution_functions/base.py:277-294
 *                                                                           (fe_mode TSFF_FE_DLM)
 *   ThomsonParams.__call__         core/modules/ts_params.py:583-603        (inside every call)
 *   ThomsonScatteringDiagnostic.__call__  core/thomson_diagnostic.py:109-142  tsff_forward
 *     FitModel.ion/electron_spectrum core/physics/generate_spectra.py:139-220
 *     add_ion_IRF / add_electron_IRF core/physics/irf.py:50-132
 *   LossFunction.vg_loss / __loss__ inverse/loss_function.py:128-168,364-373  tsff_loss_grad
 *   LossFunction.array_loss (post_loss) inverse/loss_function.py:375-384      tsff_array_loss
 *   FormFactor.calc_in_2D / rotate / calc_chi_vals  core/physics/form_factor.py:300-587   tsff_form_factor_2d(_range)
 *   angular_full electron_spectrum, add_ATS_IRF, reduce_ATS_to_resunit
 *       generate_spectra.py:193-216, irf.py:5-47, thomson_diagnostic.py:78-107           tsff_ats_setup / tsff_ats_spectrum
 *   jax reverse mode through the above (equinox.filter_value_and_grad, loss_function.py:108)
 *       tsff_loss_grad(_fe), tsff_form_factor_grad, tsff_form_factor_2d_grad, tsff_ats_adjoint
 *   jax.jvp of FormFactor.__call__, and of add_ATS_IRF + reduce_ATS_to_resunit (the reference has no such call; its post-fit
 *       half on angular decks, postprocess.py:106-136, differentiates the whole chain twice)   tsff_form_factor_jvp, tsff_ats_jvp
 *   jax.jvp of FormFactor.calc_in_2D (the post-fit half of the arts2v decks)                     tsff_form_factor_2d_jvp
 *   LossFunction.h_loss_wrt_params (equinox.filter_hessian) inverse/loss_function.py:170-188  tsff_loss_hess
 *   jax.jacfwd of ThomsonScatteringDiagnostic.__call__ w.r.t. the normalised leaves (the reference has no such call: its
 *       uncertainties come from the full Hessian, postprocess.py:188-251)           tsff_spectrum_jacobian / tsff_loss_gauss_newton
 *   _1d_adam_loop_ (optax.adam + eqx.apply_updates + best tracking)  inverse/loops.py:59-95        tsff_adam_fit
 *   _1d_scipy_loop_ (scipy L-BFGS-B, bounds=None)                     inverse/loops.py:20-56        tsff_lbfgs_fit
 *   angular_optax (optax adam / rmsprop + early stop, ARTS decks)    inverse/loops.py:167-275      tsff_angular_fit
 *   (no reference row: each lineout of a 1-D batch fitted on its own by Levenberg-Marquardt)         tsff_lm_fit
 *
 * Conventions
 *   - every array pointer in a *call* is a DEVICE pointer (hipMalloc'ed or a torch CUDA tensor);
 *     every pointer inside tsff_config is a HOST pointer and is copied by tsff_create;
 *   - all arithmetic and all arrays are float64, row-major;
 *   - the caller owns every buffer; the library never frees caller memory;
 *   - calls are asynchronous on the handle's stream (tsff_set_stream); the caller synchronises;
 *   - return value 0 = success, negative = error, text via tsff_last_error();
 *   - a refused call (negative return) of tsff_forward, tsff_loss_grad(_packed, _fe), tsff_loss_hess, tsff_spectrum_jacobian,
 *     tsff_loss_gauss_newton, tsff_array_loss,
 *     tsff_adam_fit, tsff_lm_fit, tsff_angular_fit, tsff_form_factor(_grad, _jvp), tsff_form_factor_2d(_range, _save, _grad, _jvp),
 *     tsff_ats_spectrum, tsff_ats_adjoint and tsff_ats_jvp has enqueued nothing: their arguments, LDS budgets and buffers are checked before the first
 *     launch, and tsff_last_launch reports an empty list (other entry points may have enqueued work before a failure);
 *   - a call that breaks several conditions is refused for the first of: the entry point's own arguments (-1), the active slot
 *     list (-1), a leaf the configuration does not have (-2), the leaf A (-3), the batch arguments (-1, then -2),
 *     what the entry point checks against the batch (the state size of tsff_lbfgs_fit, the LDS budget of tsff_loss_hess);
 *   - a handle is bound to the device that was current at tsff_create; handles are not thread-safe,
 *     the library is re-entrant across handles.
 *   - no CPU fallback exists: without a HIP device every entry point fails.
 */
#ifndef TSFF_H
#define TSFF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSFF_ABI_VERSION 19
/* error codes (every entry point returns 0 or one of these; text via tsff_last_error):
 * -1 bad argument, -2 unsupported configuration / option, -3 not a differentiable leaf, -5 HIP runtime error,
 * -22 stale or foreign token of saved projection records (tsff_form_factor_2d_grad),
 * TSFF_ERR_LDS: the configuration needs more LDS than a CU has (wide instrument functions at several points per pixel:
 * spectrum + halo + taps) -- the caller may retry with fewer IRF taps. */
#define TSFF_ERR_LDS (-7)

/* ---- parameter slots of one lineout: params[b][TSFF_NP(n_ion)] (normalised leaves of the
 * reference's ThomsonParams pytree, core/modules/ts_params.py:49-60,395-420,253-262) ---------- */
enum {
  TSFF_P_TE = 0,
  TSFF_P_NE = 1,
  TSFF_P_M = 2, /* DLM super-Gaussian order (base.py:252-262); ignored unless fe_mode == DLM */
  TSFF_P_LAM = 3,
  TSFF_P_AMP1 = 4,
  TSFF_P_AMP2 = 5,
  TSFF_P_AMP3 = 6,
  TSFF_P_NE_GRADIENT = 7,
  TSFF_P_TE_GRADIENT = 8,
  TSFF_P_UD = 9,
  TSFF_P_VA = 10,
  TSFF_P_ION0 = 11 /* then per ion species s: +4s+0 Ti, +1 Z, +2 A, +3 fract */
};
#define TSFF_ION_TI 0
#define TSFF_ION_Z 1
#define TSFF_ION_A 2
#define TSFF_ION_FRACT 3
#define TSFF_NP(n_ion) (TSFF_P_ION0 + 4 * (n_ion))
#define TSFF_MAX_ION 4
#define TSFF_MAX_ANGLES 1024
#define TSFF_NBINS 1024 /* irf.py:74,124: reshape(1024, -1) */
#define TSFF_NXI2 1640  /* form_factor.py:138 */
#define TSFF_NXI1 1024  /* form_factor.py:137 */
#define TSFF_DLM_NM 31  /* base.py:270 */

enum { TSFF_FE_SHARED = 0, TSFF_FE_PER_LINEOUT = 1, TSFF_FE_DLM = 2 };
enum { TSFF_LOSS_L2 = 0, TSFF_LOSS_L1 = 1, TSFF_LOSS_LOGCOSH = 2, TSFF_LOSS_POISSON = 3 };
enum { TSFF_FEATURE_ELE = 0, TSFF_FEATURE_ION = 1 };

typedef struct tsff_config {
  int32_t abi_version; /* = TSFF_ABI_VERSION */

  /* wavelength grids (form_factor.py:132-135; cfg other.lamrangE/lamrangI/npts) */
  double lamrangE[2];
  double lamrangI[2];
  int32_t npts;         /* = 1024 * points_per_pixel */
  int32_t load_ele;     /* other.extraoptions.load_ele_spec */
  int32_t load_ion;     /* other.extraoptions.load_ion_spec */
  double ele_lam_shift; /* data.ele_lam_shift (form_factor.py:196) */

  /* scattering angles and the row `weights[0]` (generate_spectra.py:165,197) */
  int32_t n_angles;
  const double *sa_deg;     /* [n_angles] */
  const double *sa_weights; /* [n_angles] */

  int32_t num_grad_points; /* parameters.general.*_gradient.num_grad_points */
  int32_t n_ion;

  /* electron distribution function */
  int32_t nvx;
  int32_t fe_mode;
  const double *fe_shared; /* [nvx], TSFF_FE_SHARED */
  const double *dlm_table; /* [nvx][TSFF_DLM_NM] = f_vx_m of base.py:272, TSFF_FE_DLM */

  /* static grids/tables of FormFactor.__init__ (form_factor.py:137-139) */
  const double *xi1;       /* [TSFF_NXI1] */
  const double *xi2;       /* [TSFF_NXI2] */
  const double *zprime_re; /* [TSFF_NXI2] rdWT.txt interpolated on xi2 */
  const double *zprime_im; /* [TSFF_NXI2] */
  /* log-ratio table of ratintn.py:49 on the (xi1, xi2) grids, Lg[q][i] = log|(gav + gdif/2)/(gav - gdif/2)|,
   * [TSFF_NXI2][TSFF_NXI1] with the two unused columns (i >= 1022) zero.  Required unless fe_mode == SHARED:
   * per-lineout W tables are then two matrix-vector products with this constant table. */
  const double *lg_table;

  /* instrument response + binning (irf.py:50-132) as ONE set of bin-averaged taps per feature:
   *   ybin[p] = sum_{s < n_taps} taps[s] * x[p * ppp + tap_off + s],   ppp = npts / 1024,
   * i.e. taps = (1/ppp) * (Gaussian of irf.py:66-72 / 110-114, in the reference's "same" alignment) convolved
   * with a ppp-wide box (irf.py:74,124); see DESIGN.md section 3 and engine.binned_taps(). */
  int32_t n_taps_ele;
  int32_t tap_off_ele;
  const double *taps_ele;
  int32_t n_taps_ion; /* 0 <=> spect_stddev_ion == 0 (irf.py:82-86): ThryI = modlI + noise_i, not convolved, not normalised, no
                         amplitudes (needs npts == 1024, as in the reference where [npts] must match the [1024] data) */
  int32_t tap_off_ion;
  const double *taps_ion;
  int32_t norm; /* other.PhysParams.norm; only 0 is implemented */

  /* iawfilter (generate_spectra.py:210-216) as a per-sample multiplier on the EPW grid */
  const double *ele_filter; /* [npts] or NULL (= all ones) */

  /* parameter transform (ts_params.py:329-350): phys = act(x) * scale + shift */
  const double *p_scale;        /* [NP] */
  const double *p_shift;        /* [NP] */
  const uint8_t *p_sigmoid;     /* [NP] 1 = sigmoid activation, 0 = identity */
  uint8_t ti_same[TSFF_MAX_ION]; /* ion-k.Ti.same (ts_params.py:557-558) */

  /* loss (loss_function.py:190-267, 386-418) */
  int32_t loss_method;
  const uint8_t *mask_ele; /* [1024] bit0: blue range fitted, bit1: red range fitted */
  const uint8_t *mask_ion; /* [1024] bit0: IAW range fitted */
} tsff_config;

typedef struct tsff_handle tsff_handle;

/* lifecycle ------------------------------------------------------------------------------- */
int tsff_create(const tsff_config *cfg, tsff_handle **out);
void tsff_destroy(tsff_handle *h);
const char *tsff_last_error(const tsff_handle *h); /* h == NULL: last tsff_create failure */
/* the kernels the most recent entry point on h enqueued, in launch order, ';'-separated, each spelled like its demangled
 * device symbol without "void tsff::" (e.g. "k_fused_prep<1>;k_spectrum_fused<1, 0, false, true>;k_fused_finish<1>");
 * valid until the next call on h.  Recorded on the host: no device synchronisation. */
const char *tsff_last_launch(const tsff_handle *h);
int tsff_abi_version(void);
/* Bind the handle to a stream; later calls enqueue on it.  The handle's scratch is shared by its calls, so when the stream
 * changes after a call, the new stream first waits on an event recorded on the old one: a call on the new stream never
 * overtakes the handle's work still running on the old one (the caller's own buffers are the caller's to order).  Setting the
 * stream the handle already has is a no-op.  The stream a handle is bound to must stay valid while it is bound: to retire a
 * stream, first bind the handle to another one (or to the null stream), then destroy it.  If either stream is capturing a
 * graph, the new stream does not wait: ordering it behind earlier work is then the caller's job (see the graph-capture contract
 * at tsff_reserve). */
int tsff_set_stream(tsff_handle *h, void *hip_stream);
/* options.  TSFF_OPT_DENOM_MODE: denominators of the l1/l2 functionals in tsff_loss_grad -- 0 (default):
 * constants folded into `weights` (LossFunction.__loss__, loss_function.py:364-373); 2: |data| + 1e-10 per sample
 * (LossFunction._loss_for_hess_fn_, loss_function.py:173-188, the loss whose Hessian gives the fit uncertainties).
 * TSFF_OPT_LAUNCH_PLAN: bit mask, 0 (default) automatic -- with two loaded features one launch of 2B 256-thread workgroups, one
 * per (lineout, feature), when two of them fit a CU; tsff_loss_grad runs the one-sweep kernel (forward value and Jacobian rows
 * of every wavelength sample in one pass over the points) where it applies: one gradient point, n_ion <= 2, no gradient w.r.t.
 * the tabulated f_e; with one point per pixel the rows stay in registers, with more (the reference's default decks: 5) they go
 * through a scratch array in device memory that the handle allocates on first use: B x loaded features x (8 + 3 n_ion) x npts
 * doubles, 1 GB at B = 1024 and 5 points per pixel (above 16 GB the two-sweep kernel is used instead).  Bit 0: never interleave (both features in one 512-thread workgroup) and never spread the
 * rounds of a lineout over several workgroups (the small-batch form of the several-points-per-pixel kernel); bit 1: always the
 * two-sweep kernel (and, for tsff_forward at several points per pixel, k_spectrum instead of the forward form of the rounds kernel); bit 2: never three forward-only workgroups per CU (tsff_forward runs three 256-thread workgroups per CU when
 * the batch is large enough to need them); bit 3: the one-sweep kernel evaluates every base point itself instead of taking its pair's
 * right neighbour from the next lane; bit 5 (32): the per-lineout W tables by the 128 x 128-tiled GEMM instead of the 128 x 144 one (bit 4 is
 * unused and refused).  The spectra are identical either way; the gradient differs by rounding.
 * TSFF_OPT_DLM_BLOCKS (experimental, default off): tsff_loss_grad(_packed) with fe_mode TSFF_FE_DLM and the DLM order among the
 * differentiated leaves builds the per-lineout tables (k_fe_vectors + the FP64-MFMA GEMM) in n column blocks of the batch on a second
 * stream owned by the handle (non-blocking, higher priority) while the one-sweep kernel works on the previous block on the handle's
 * stream; the call still returns with everything ordered on the handle's stream (fork / join by events).  0 / 1: off (one stream),
 * n: n blocks (rounded to multiples of 256 lineouts).  Same bits either way.  On gfx950 it is slower than one stream (the FP64 matrix
 * and vector instructions share one datapath: DESIGN.md section 4.2), which is why it is off. */
enum { TSFF_OPT_DENOM_MODE = 1, TSFF_OPT_LAUNCH_PLAN = 2, TSFF_OPT_DLM_BLOCKS = 3 };
int tsff_set_option(tsff_handle *h, int32_t key, int32_t value);
/* make sure the workspace holds B lineouts (calls grow it lazily).
 * Graph capture: tsff_forward and tsff_loss_grad(_packed) can be captured on the handle's stream after (1) tsff_reserve(h, B) with B at least the captured batch, (2) one eager call with the grad mask and slot list to
 * be captured, (3) a synchronisation of the stream.  A call on a capturing stream that would have to allocate, upload a changed
 * mask or slot list, or synchronise is refused with -2 and enqueues nothing; so is a loss + gradient call that would run the
 * pipelined DLM plan (TSFF_OPT_DLM_BLOCKS > 1 forks onto a second stream: set the option to 0 before capturing).  The captured kernels take the device pointers and
 * the host scalars (weights, B, offsets) of the call: replays read new parameters from the same buffers. */
int tsff_reserve(tsff_handle *h, int32_t B);

/* wavelength axes (HOST pointers): the binned axes lamAxisE/lamAxisI [1024] in nm that the
 * reference returns per lineout (irf.py:75,125) -- they do not depend on the parameters. */
int tsff_get_axes(const tsff_handle *h, double *lamE, double *lamI);

/* Re(chi_e) table W[1640] and the Hermite table of ln fe for `n` distribution functions
 * fe[n][nvx] (form_factor.py:263-268 + ratintn.py).  W: [n][1640]. */
int tsff_chi_table(tsff_handle *h, const double *fe, int32_t n, double *W);

/* FormFactor.__call__ for B lineouts without the instrument chain: P[B][G][npts][n_angles]
 * (W/m^... arbitrary units of the reference).  `phys` holds PHYSICAL parameters [B][NP]
 * (no activation); fe is [B][nvx] (PER_LINEOUT), ignored otherwise. */
int tsff_form_factor(tsff_handle *h, int32_t feature, const double *phys, const double *fe,
                     int32_t B, double *P);

/* Adjoint of tsff_form_factor for an arbitrary seed Pbar = d loss / d P (device, [B][G][npts][n_angles]):
 *   grad_phys [B][NP] (device): d loss / d PHYSICAL parameters (the DLM order m carries none here: it acts through fe),
 *   grad_fe   [B][nvx] (device, or NULL): d loss / d fe[b][i] through both uses of the distribution function (Hermite
 *     ln f_e lookup and the ratintn table W), fe_mode PER_LINEOUT only.
 * The angular (ARTS) instrument chain hands back one adjoint per (wavelength, angle) point (tsff_ats_adjoint); this is
 * what reverse-mode JAX does for angular decks with a 1-D distribution function (inverse/loops.py:167-275). */
int tsff_form_factor_grad(tsff_handle *h, int32_t feature, const double *phys, const double *fe, int32_t B,
                          const double *Pbar, double *grad_phys, double *grad_fe);

/* Forward mode of tsff_form_factor -- what jax.jvp of FormFactor.__call__ (core/physics/form_factor.py:163-298) gives -- for n_dir
 * directions at once:  P_dot[k] = dP/dphys . phys_dot[k] + dP/dfe . fe_dot[k],  the same arguments, parameter handling (PHYSICAL
 * parameters, Ti tying) and table convention as tsff_form_factor / tsff_loss_hess (the Z' and W lookups carry their slope, the
 * Hermite ln f_e lookup its true derivative).
 *   phys_dot [n_dir][B][NP] (device); fe_dot [n_dir][B][nvx] (device) or NULL: no direction of f_e (fe_mode PER_LINEOUT only: -2);
 *   P [B][G][npts][n_angles] (device) or NULL: the value, bit for bit tsff_form_factor's;  P_dot [n_dir][B][G][npts][n_angles].
 * The directions run three to a launch (the groups loop inside the call, n_dir is unbounded); with fe_dot each of the three
 * carries its own tangent tables in LDS (13 KB + 32 nvx B each), one per launch when three do not fit, -2 when one does not.
 * Two calls give bit-identical results (no atomics).  A null phys, phys_dot or P_dot, or n_dir < 1: -1. */
int tsff_form_factor_jvp(tsff_handle *h, int32_t feature, const double *phys, const double *fe, int32_t B, int32_t n_dir,
                         const double *phys_dot, const double *fe_dot, double *P, double *P_dot);

/* FormFactor.calc_in_2D (core/physics/form_factor.py:449-587, with rotate :300-324 and calc_chi_vals :349-388)
 * for a 2-D electron distribution fe2d[nv][nv] on the grid linspace(-6 + dv/2, 6 - dv/2, nv) (first index = v_x;
 * one table shared by all lineouts when shared_fe != 0, else [B][nv][nv]): P[B][G][npts][n_angles].  `phys` holds
 * PHYSICAL parameters [B][NP]; ud_angle / va_angle are the drift and flow directions in degrees
 * (parameters.general.ud.angle / Va.angle).  Its adjoint is tsff_form_factor_2d_grad.  Parity with the reference is unpinned for this entry:
 * its golden vectors are not part of the reference source tree. */
int tsff_form_factor_2d(tsff_handle *h, int32_t feature, const double *phys, const double *fe2d, int32_t nv,
                        int32_t shared_fe, double ud_angle_deg, double va_angle_deg, int32_t B, double *P);
/* The same for the points [point_begin, point_end) of the flat (lineout, gradient point, wavelength, angle) list only;
 * the rest of P is left untouched (point_end < 0: to the end).  This is the unit of work the reference shards across
 * devices (parallel_calc_all_chi_vals, form_factor.py:431-447): each rank evaluates its range, the ranges are gathered. */
int tsff_form_factor_2d_range(tsff_handle *h, int32_t feature, const double *phys, const double *fe2d, int32_t nv,
                              int32_t shared_fe, double ud_angle_deg, double va_angle_deg, int32_t B,
                              int64_t point_begin, int64_t point_end, double *P);

/* tsff_form_factor_2d_range for ONE shared table (nv <= 256) that also keeps, in the handle, the projection record of
 * every point of the range (the projected distribution and the derivative sums of its rotation: proj2d_doubles(nv)
 * doubles per point): the adjoint that follows in a fit step (tsff_form_factor_2d_grad with saved_token = *token, same
 * feature / table size / point range, same phys and fe2d) then does no sampling of its own.  *token (HOST pointer, never 0 on
 * success) names this generation of records: a per-handle call counter mixed with the buffers, angles and range they were made
 * from.  Only the token of the LAST save is valid, and any later 2-D forward on the handle invalidates it.  Precondition the
 * token cannot check: the CONTENTS of phys / fe2d must not change between the save and the adjoint that presents its token. */
int tsff_form_factor_2d_save(tsff_handle *h, int32_t feature, const double *phys, const double *fe2d, int32_t nv,
                             double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin,
                             int64_t point_end, double *P, uint64_t *token);

/* Adjoint of tsff_form_factor_2d for ONE shared table (the 2-D path is never batched in the reference): given
 * Pbar = d loss / d P (device, [B][G][npts][n_angles]) ->
 *   grad_phys [B][NP] (device): d loss / d PHYSICAL parameters (Te, ne, lam, ne_gradient, Te_gradient, ud, Va, Ti, Z;
 *     amplitudes and A carry none here), and, when grad_fe2d != NULL,
 *   grad_fe2d [nv][nv] (device): d loss / d fe2d[i][j] -- the table adjoint of the rotate-and-project step (bicubic
 *     weights scattered by LDS atomics, ghost cells folded back).
 * [point_begin, point_end) (point_end < 0: to the end): the contributions of that slice of the flat point list only --
 * both adjoints are sums over points, so the ranks of a node each take a slice and all-reduce the two outputs.
 * saved_token != 0: the projections come from the records of the tsff_form_factor_2d_save that returned this token (see
 * there); a stale or foreign token is refused with -22 (EINVAL), records made from other buffers / angles / range with -2.
 * Replaces what JAX reverse mode gives the reference for angular fits (inverse/loops.py:167-275). */
int tsff_form_factor_2d_grad(tsff_handle *h, int32_t feature, const double *phys, const double *fe2d, int32_t nv,
                             double ud_angle_deg, double va_angle_deg, int32_t B, int64_t point_begin,
                             int64_t point_end, uint64_t saved_token, const double *Pbar, double *grad_phys,
                             double *grad_fe2d);

/* Forward mode of tsff_form_factor_2d for ONE shared table, 4 <= nv <= 256, and n_dir directions at once:
 *   P_dot[k] = dP/dphys . phys_dot[k] + dP/dfe2d . fe2d_dot[k].
 * `phys` [B][NP] holds PHYSICAL parameters, handled as tsff_form_factor_2d / _2d_grad handle them (no activation, Ti tying);
 *   phys_dot [n_dir][B][NP] (device); fe2d_dot [n_dir][nv][nv] (device) or NULL: no table direction;
 *   P [B][G][npts][n_angles] (device) or NULL: the value, bit for bit what tsff_form_factor_2d_save writes (that kernel writes it);
 *   P_dot [n_dir][B][G][npts][n_angles] (device).
 * [point_begin, point_end) as in tsff_form_factor_2d_range / _save (point_end < 0: to the end); points outside the range are left
 * untouched in P and P_dot.  The call runs a saving forward (its records feed the tangents: proj2d_doubles(nv) doubles per point
 * in the handle, and with fe2d_dot three projections of nv doubles per point more), so it INVALIDATES the token of any earlier
 * tsff_form_factor_2d_save on the handle, and leaves none of its own.  The directions run three to a launch (the groups loop inside
 * the call, n_dir is unbounded); with fe2d_dot the table of every direction that has a non-zero entry is projected
 * (k_ff2d_project; a flag per direction is made on the device, the host does not look at it), and a direction whose table tangent
 * is all zeros gives the same bits as the same call with fe2d_dot = NULL.  Conventions: the two linear lookups at |xi_e|
 * carry their cell's slope where the position is not clamped and none where it is, the half-plane term of the rotation angle carries
 * no tangent, the ion terms follow tsff_form_factor_jvp (Z' with its slope, no curvature).  Two calls give bit-identical results and
 * a point's result does not depend on the range it was computed in (no atomics, every sum in a fixed order).
 * nv > 256 (no records there): -2; per-lineout tables are not taken (the signature has none).  A null phys, fe2d, phys_dot or P_dot,
 * n_dir < 1 or a bad range: -1. */
int tsff_form_factor_2d_jvp(tsff_handle *h, int32_t feature, const double *phys, const double *fe2d, int32_t nv,
                            double ud_angle_deg, double va_angle_deg, int32_t B, int32_t n_dir, const double *phys_dot,
                            const double *fe2d_dot, int64_t point_begin, int64_t point_end, double *P, double *P_dot);

/* Angular (ARTS) instrument chain for one image P[G][npts][n_angles] (device; from tsff_form_factor_2d or, for a 1-D
 * distribution function, tsff_form_factor): FitModel.electron_spectrum "angular_full" branch
 * (core/physics/generate_spectra.py:193-216: weight-matrix product, iawfilter), add_ATS_IRF (core/physics/irf.py:5-47,
 * norm == 0), reduce_ATS_to_resunit (core/thomson_diagnostic.py:78-107).  Output ThryE (device)
 * [row_end - row_start][npts / lam_step].  Every pointer of tsff_ats_config is a HOST pointer, copied by tsff_ats_setup.
 * Convolution taps are in the flipped "same" form y[i] = sum_s taps[s] x[i + tap_off + s] (engine.binned_taps with ppp = 1). */
typedef struct tsff_ats_config {
  int32_t n_px;           /* rows of the weight matrix = angular pixels (1024) */
  const double *weights;  /* [n_px][n_angles] */
  int32_t n_taps_ang, tap_off_ang;
  const double *taps_ang; /* Gaussian over sas["angAxis"], ang_FWHM_ele / 2.3548 */
  int32_t n_taps_lam, tap_off_lam;
  const double *taps_lam; /* Gaussian over the wavelength axis, spect_FWHM_ele / 2.3548 */
  int32_t lam_step, ang_step; /* thomson_diagnostic.py:93-94 */
  int32_t row_start, row_end; /* data.lineouts.start / end (rows of the reduced image) */
  const double *lam_axis;     /* [npts] wavelength axis in nm */
} tsff_ats_config;
int tsff_ats_setup(tsff_handle *h, const tsff_ats_config *cfg);
int tsff_ats_spectrum(tsff_handle *h, const double *P, const double *e_amps /* device [rows] */, double lam, double amp1, double amp2, double *ThryE);
/* Reverse of tsff_ats_spectrum: given Ebar = d loss / d ThryE (device, [rows][npts / lam_step]) -> Pbar = d loss / d P
 * (device, [G][npts][n_angles]) and amp_bar[2] = d loss / d (amp1, amp2) (host).  `lam` enters the model only through
 * the blue / red split of the wavelength axis and carries no gradient, like in the reference's jnp.where. */
int tsff_ats_adjoint(tsff_handle *h, const double *P, const double *e_amps, double lam, double amp1, double amp2,
                     const double *Ebar, double *Pbar, double *amp_bar);
/* Forward mode of tsff_ats_spectrum -- jax.jvp of add_ATS_IRF + reduce_ATS_to_resunit (irf.py:5-47,
 * thomson_diagnostic.py:78-107) behind the angular electron_spectrum -- for n_dir directions:
 *   P_dot [n_dir][G][npts][n_angles] (device), amp_dot [n_dir][2] (HOST): the tangents of (amp1, amp2);
 *   ThryE [rows][npts / lam_step] (device) or NULL: the value, bit for bit tsff_ats_spectrum's;  ThryE_dot [n_dir][rows][npts / lam_step].
 * The weight matrix, the notch filter, the convolutions and the block means are linear; the two row normalisations take their
 * tangent through 1 / max at the arg-max of the value (the first in index order).  `lam` only selects between the amplitudes
 * and carries no tangent here (it does through P). */
int tsff_ats_jvp(tsff_handle *h, const double *P, const double *P_dot, int32_t n_dir, const double *e_amps, double lam, double amp1,
                 double amp2, const double *amp_dot, double *ThryE, double *ThryE_dot);

/* ThomsonScatteringDiagnostic.__call__: ThryE/ThryI [B][1024].  noise_* may be NULL (= 0).
 * params: normalised leaves [B][NP]; fe: [B][nvx] when fe_mode == PER_LINEOUT else NULL. */
int tsff_forward(tsff_handle *h, const double *params, const double *fe, const double *e_amps,
                 const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                 double *ThryE, double *ThryI);

/* LossFunction.vg_loss: value and gradient.
 *   weights[3] (HOST): w_iaw, w_blue, w_red -- the factor each masked sum carries in the total
 *   loss, i.e. ion_loss_scale/(N_iaw*i_norm^2), c/(N_blue*e_norm^2), c/(N_red*e_norm^2) with N_* the
 *   number of fitted samples over the WHOLE (global, all ranks) batch and c = 1/2 when both EPW
 *   ranges are fitted (loss_function.py:262-264, 335-338).
 *   loss_terms[3] (device): un-weighted masked sums  S_iaw, S_blue, S_red  over these B lineouts;
 *   total loss = sum_k weights[k] * S_k (summed over ranks).
 *   grad (device) [B][NP]: d(total loss)/d(params[b][slot]) for slots with grad_mask[slot] != 0
 *   (HOST uint8 [NP]), 0 elsewhere.  The DLM order slot (TSFF_P_M) is differentiable when
 *   fe_mode == TSFF_FE_DLM (through the ln f_e and W tables).  ThryE/ThryI may be NULL. */
int tsff_loss_grad(tsff_handle *h, const double *params, const double *fe, const double *e_data,
                   const double *i_data, const double *e_amps, const double *i_amps,
                   const double *noise_e, const double *noise_i, int32_t B,
                   const double *weights, const uint8_t *grad_mask, double *loss_terms,
                   double *grad, double *ThryE, double *ThryI);

/* tsff_loss_grad delivering the gradient the way the optimiser consumes it -- the flat vector of ravel_pytree that
 * scipy L-BFGS-B iterates on (inverse/loops.py:40-54: trainable leaves outermost, lineouts innermost) over the GLOBAL
 * batch of a lineout-sharded fit -- written straight into the buffer of the step's one all-reduce:
 *   packed (device) [3 + n_active * B_global] = [S_iaw, S_blue, S_red | g[k][b]],  k < n_active, b < B_global;
 *   active_slots (HOST) [n_active]: the parameter slot of each row k (the ravel order of the trainable leaves);
 *   this call fills the loss sums of ITS B lineouts and the columns [b_offset, b_offset + B) of every row, and writes
 *   zero to every other column: summed over the ranks (in place, no memset between steps) the buffer is the full
 *   loss and gradient on every rank; with one rank (B_global == B, b_offset == 0) it is what LossFunction.vg_loss
 *   returns after one device-to-host copy.  weights / grad_mask as for tsff_loss_grad. */
int tsff_loss_grad_packed(tsff_handle *h, const double *params, const double *fe, const double *e_data,
                          const double *i_data, const double *e_amps, const double *i_amps, const double *noise_e,
                          const double *noise_i, int32_t B, const double *weights, const uint8_t *grad_mask,
                          const int32_t *active_slots, int32_t n_active, int64_t B_global, int64_t b_offset,
                          double *packed, double *ThryE, double *ThryI);

/* The reference's 1-D Adam loop (_1d_adam_loop_, inverse/loops.py:59-95) on the device: n_steps steps, each the packed
 * loss + gradient of tsff_loss_grad_packed (B_global = B, b_offset = 0, no spectra) into a buffer owned by the handle followed by
 * one Adam update of the active leaves, all enqueued on the handle's stream; the call returns once they are enqueued (no
 * synchronisation and no allocation between the steps -- everything is sized and uploaded before the first launch).
 *   params (device [B][NP], in/out): normalised leaves; the slots of active_slots are trained, the others stay as they are;
 *   fe: as tsff_loss_grad -- with fe_mode PER_LINEOUT the given [B][nvx] table is a constant: this entry never trains f_e;
 *   weights (HOST [3]): as tsff_loss_grad; the loss of a step is (w[0] S_iaw + w[1] S_blue) + w[2] S_red;
 *   active_slots (HOST [n_active]): the trained slots in ravel order (as tsff_loss_grad_packed); the gradient mask is derived
 *   from them.  A slot out of range or repeated returns -1, TSFF_P_M without fe_mode == TSFF_FE_DLM -2, an ion's A slot -3;
 *   step0: the optimiser's step count before the first step (optax's `count`): a fit run in chunks of 10 + 10 + 10 steps with
 *   step0 = 0, 10, 20 is bit for bit one call of 30 steps;
 *   hyper (HOST [4]): lr, b1, b2, eps;
 *   state (device [2][n_active][B], in/out): mu, nu of the active leaves; zeros start a fit;
 *   loss_hist (device [n_steps] or NULL): the loss of each step, measured at the parameters BEFORE its update;
 *   best (device [1 + B * NP], in/out): [best loss | best params]; start a fit with [1e16 | params].  A step whose loss is below
 *   best[0] (never a NaN) makes it the best loss and copies the step's UPDATED iterate into the active slots of the best
 *   params (loops.py:88-93 store diff_params after apply_updates: the iterate one step past the one whose loss was measured).
 * The update is tsadar_amd.tree.Adam's, operation for operation in double and unfused (k_adam.inc):
 *   mu = b1 mu + (1 - b1) g;  nu = b2 nu + ((1 - b2) g) g;  x += ((-lr) (mu / c1)) / (sqrt(nu / c2) + eps),
 *   c1 = 1 - b1^count, c2 = 1 - b2^count (computed on the host with pow), count = step0 + step + 1,
 * so it reproduces that host loop bit for bit (optax associates -lr * ((m / c1) / (...)) and (1 - b2) g^2: an ulp apart).
 * n_steps == 0 returns 0 and enqueues nothing; n_steps < 0, a null params, state, best or hyper returns -1. */
int tsff_adam_fit(tsff_handle *h, double *params, const double *fe, const double *e_data, const double *i_data,
                  const double *e_amps, const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                  const double *weights, const int32_t *active_slots, int32_t n_active, int32_t n_steps, int32_t step0,
                  const double *hyper, double *state, double *loss_hist, double *best);

/* The reference's default 1-D loop (_1d_scipy_loop_, inverse/loops.py:20-56: scipy L-BFGS-B on the activated leaves, bounds=None)
 * on the device: n_evals x (the packed loss + gradient of tsff_loss_grad_packed with B_global = B, b_offset = 0 and no spectra,
 * into a buffer owned by the handle, then 2 maxcor + 6 launches of k_lbfgs_step, one pass of the optimiser each), all enqueued
 * on the handle's stream; the call returns once they are enqueued (no synchronisation and no allocation between the evaluations).  The optimiser is joint, unbounded L-BFGS-B on the
 * flat vector of n = n_active x B unknowns in ravel order, as tsadar_amd/lbfgs.py restates it: the device reproduces that host
 * restatement bit for bit (fixed-order inner products, k_lbfgs.inc) and scipy's iterates up to rounding.
 *   params (device [B][NP], in/out): normalised leaves; k_lbfgs_step writes the next point to evaluate into the active slots;
 *   once the status is terminal they hold the result (the last accepted iterate) and later evaluations change nothing;
 *   fe, e_data .. noise_i, B, weights, active_slots, n_active: as tsff_adam_fit (the same refusals: a slot out of range or
 *   repeated -1, TSFF_P_M without fe_mode == TSFF_FE_DLM -2, an ion's A slot -3); the loss of an evaluation is
 *   (w[0] S_iaw + w[1] S_blue) + w[2] S_red;
 *   opts (HOST [6]): maxcor (1..64), ftol, gtol, maxiter, maxfun, maxls -- scipy's options of the same names;
 *   state (device [n_state], in/out): the optimiser (line search, x0, g0, d and the (s, y) ring); all zeros starts a fit at
 *   params; n_state >= tsff_lbfgs_state_size(B, n_active, maxcor), else -1.  A fit run in chunks of 7 + 7 + 7 evaluations on
 *   the same state is bit for bit one call of 21;
 *   f_hist (device [n_evals] or NULL): the loss of each evaluation (NaN for an evaluation after the end);
 *   info (device int32 [4] or NULL): status, nit, nfev, nskip after the last evaluation.  status: 0 running, 1 converged
 *   (max|g| <= gtol), 2 converged (relative reduction of f <= ftol), 3 nit >= maxiter, 4 nfev > maxfun, 5 abnormal (the line
 *   search failed with an empty memory); scipy's status is 0 for 1-2, 1 for 3-4, 2 for 5.
 * n_evals == 0 returns 0 and enqueues nothing; n_evals < 0, a null params, weights, active_slots, opts or state, or a bad option
 * returns -1. */
int tsff_lbfgs_state_size(int32_t B, int32_t n_active, int32_t maxcor, int64_t *n_doubles);
int tsff_lbfgs_fit(tsff_handle *h, double *params, const double *fe, const double *e_data, const double *i_data,
                   const double *e_amps, const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                   const double *weights, const int32_t *active_slots, int32_t n_active, int32_t n_evals, const double *opts,
                   double *state, int64_t n_state, double *f_hist, int32_t *info);

/* The reference's angular loop (angular_optax, inverse/loops.py:167-275) on the device for one ARTS image: n_epochs epochs of
 *   leaves -> physical parameters (ThomsonParams.__call__) and f_e of the generator -> tsff_form_factor (1-D) or the saving
 *   tsff_form_factor_2d -> tsff_ats_spectrum with lam, amp1, amp2 read on the device -> loss and its seed (k_ang_loss: the
 *   masks and loss functionals of LossFunction._angular_value, noise_e added) -> tsff_ats_adjoint, amplitude adjoints kept on
 *   the device -> tsff_form_factor_grad or tsff_form_factor_2d_grad (saved records; the table adjoint when the table is
 *   trained) -> chain rule (k_ang_chain: amplitudes, Ti tying, activation, the DLM order by central differences with h = 1e-6,
 *   the Arbitrary2V VJP) -> optimiser step and early stop (k_ang_opt),
 * all enqueued on the handle's stream; the call returns once they are enqueued.  Every refusal is checked before anything is
 * allocated, and the handle's scratch is sized before the first launch: no epoch allocates, and nothing synchronises.  Needs
 * fe_mode == TSFF_FE_PER_LINEOUT and tsff_ats_setup.
 *   spec (HOST): the deck and the optimiser, below;
 *   leaves (device [NP + n_table], in/out): the normalised leaves of the one plasma condition, then the generator's;
 *   gen_data (device): the generator's constants, by generator below;
 *   e_data, noise_e (device [rows][nJ]), wcol (device [nJ]: blue / red masks over rows x mask count, halved when both are
 *   fitted), e_amps (device [rows]);
 *   moments (device [2 n] Adam (mu | nu), [n] RMSProp, n = n_active + n_table; in/out): the active scalar slots in the order
 *   of active_slots, then the generator's leaves;
 *   best (device [1 + NP + n_table], in/out): [best loss | the leaves after the update of the best epoch]; start at 100;
 *   ctl (device int32 [8], in/out, zeros to start): [0] status (0 running, 1 ended: later epochs change nothing), [1] the
 *   epoch the fit ended after, [2] g_wait, [3] b_wait (the reference's counters), [4] 1 once a best exists;
 *   loss_hist (device [n_epochs] or NULL): each epoch's loss (NaN after the end);
 *   best_hist (device [n_epochs][NP + tail] or NULL): the best leaves after each epoch (save_state), untouched while none exists.
 * The generators (spec.generator; nv = spec.nv, n_gen = spec.n_gen):
 *   generator         f_e      n_table  f_e built by                       chained back by                       adjoint returns  tail   m a   gen_data
 *                                                                                                                d loss / d f_e          leaf
 *   TSFF_ANG_TABLE2D  [nv][nv] 0        nothing: gen_data is the table     nothing                               no               0      no    the table [nv][nv]
 *   TSFF_ANG_DLM      [nv]     0        k_ang_leaves                       k_ang_chain (dot with d f_e / d m)    when m is a leaf 0      yes   [nv][31] DLM table | [31] m axis
 *   TSFF_ANG_ARB2V    [nv][nv] nv^2     k_ang_leaves                       k_ang_chain (the Arbitrary2V VJP)     yes              0      no    unused (may be NULL)
 *   TSFF_ANG_SPH      [nv][nv] n_gen    k_ang_leaves, k_sph_table          k_ang_chain, k_sph_vjp                yes              n_gen  no    the constants below
 *   TSFF_ANG_ARB1V    [nv]     nv       k_ang_leaves, k_arb1v_matvec,      k_ang_chain, k_arb1v_point,           yes              nv     no    S[nv][nv] | S^T[nv][nv]
 *                                       k_arb1v_point                      k_arb1v_matvec
 * 1-D generators (f_e [nv]) need nv == the handle's nvx and run tsff_form_factor and its adjoint, 2-D ones (nv = 4 .. 256) the
 * saving tsff_form_factor_2d and its adjoint from the saved records.  The scratch of k_sph.inc and k_arb1v.inc is part of the
 * fit's.  TSFF_ANG_DLM: tsadar_amd.distribution.dlm_table, M_AXIS.
 * TSFF_ANG_SPH (a trained SphericalHarmonics generator, k_sph.inc): its leaves are in the order of SphericalHarmonics.get_params()
 * (per harmonic (l, m), sorted: log_10_LT for TSFF_SPH_MORA_YAHI, flm_sign[nvr] then flm_mag[nvr] for TSFF_SPH_ARBITRARY; then
 * normed_m).  Its gen_data holds everything that does not depend on the trained parameters (doubles, integers stored as
 * doubles; n2 = nv^2, H = n_harm; tsadar_amd.distribution.sph_gen_data packs it):
 *   vr[nvr] | cell[n2] | wt[n2] | inside[n2] | Y[H][n2]       the radial axis; per grid point the radial cell, the weight in it and
 *                                                             1 inside the axis (np.interp), Re Y_l^m per harmonic and point;
 *   | M[nvr][nvr] | ptr[nvr + 1] | pt[2 n2] | cw[2 n2]        TSFF_SPH_ARBITRARY only: the smoothing matrix and, for the transposed
 *                                                             interpolation, per radial node k the grid points pt[e] and weights
 *                                                             cw[e] that reach it, e in [ptr[k], ptr[k + 1]) (unused tail: zeros).
 * TSFF_ANG_ARB1V (a trained free-form 1-D f_e, the reference's Arbitrary1V; k_arb1v.inc): f_e = normalise(10^-(7 S fval)^2) with S
 * the constant forward-backward Butterworth matrix, row-major (tsadar_amd.distribution.arb1v_gen_data), and d loss / d f_e
 * chained to fval exactly.  The spec has no field of its own for it.
 * Chunks: epoch0 = the epochs done so far (Adam's bias correction); a fit in chunks is bit for bit one call.
 * Refusals, in this order: a null pointer -1; an unknown generator -2; a 1-D generator's nv other than the handle's nvx -1;
 * nv outside 4 .. 256 for 2-D tables -2; gen_data missing -1; TSFF_ANG_SPH: an unknown radial type, n_harm != 2 for Mora-Yahi
 * (l = 1 only) or outside 1 .. 64, nvr < 2, or n_gen other than n_harm + 1 (Mora-Yahi) / 2 n_harm nvr + 1 (free radial
 * functions) -2; an unknown optimiser or loss method -2; a slot out of range or repeated -1, TSFF_P_M where m is no leaf -2, an
 * ion's A slot -3; nothing to train -1; too little LDS -2 (TSFF_ERR_LDS for the 1-D adjoint). */
enum { TSFF_ANG_TABLE2D = 0, TSFF_ANG_DLM = 1, TSFF_ANG_ARB2V = 2, TSFF_ANG_SPH = 3, TSFF_ANG_ARB1V = 4 };
enum { TSFF_SPH_MORA_YAHI = 0, TSFF_SPH_ARBITRARY = 1 }; /* flm_type of a SphericalHarmonics generator */
enum { TSFF_ANG_ADAM = 0, TSFF_ANG_RMSPROP = 1 };
typedef struct {
  int32_t generator;            /* TSFF_ANG_* */
  int32_t nv;                   /* velocity points per axis (DLM, ARB1V: the handle's nvx) */
  int32_t learn_log;            /* TSFF_ANG_ARB2V: fval^2 is -log10 f */
  int32_t n_active;             /* trained scalar slots */
  const int32_t *active_slots;  /* HOST [n_active] */
  int32_t loss_method;          /* TSFF_LOSS_* */
  double un;                    /* e_norm^2 (l1, l2) */
  double ud_angle, va_angle;    /* degrees (2-D) */
  double dvx;                   /* vx[1] - vx[0] of the velocity grid */
  int32_t method;               /* TSFF_ANG_ADAM or TSFF_ANG_RMSPROP */
  double lr, b1, b2, eps;       /* Adam: optax's (b1, b2, eps); RMSProp: eps */
  double decay;                 /* RMSProp */
  int32_t n_epochs, epoch0;
  int32_t sph_type;             /* TSFF_ANG_SPH: TSFF_SPH_* */
  int32_t n_harm, nvr, n_gen;   /* TSFF_ANG_SPH: harmonics (l, m), radial nodes, trained generator parameters */
} tsff_angular_spec;
int tsff_angular_fit(tsff_handle *h, const tsff_angular_spec *spec, double *leaves, const double *gen_data, const double *e_data,
                     const double *noise_e, const double *wcol, const double *e_amps, double *moments, double *best, int32_t *ctl,
                     double *loss_hist, double *best_hist);

/* The SphericalHarmonics generator on its own (k_sph.inc; the kernels of TSFF_ANG_SPH), asynchronous on the handle's stream:
 *   tsff_sph_table:     theta (device [n_gen], get_params() order) -> fe (device [nv][nv]) = SphericalHarmonics.__call__();
 *   tsff_sph_table_vjp: theta, fe_bar (device [nv][nv]) = d loss / d fe -> grad (device [n_gen]) = d loss / d theta, exact (no
 *   finite differences) and bit-reproducible from run to run (every sum in a fixed order, no atomics).
 * sph_type, n_harm, nvr, n_gen and gen_data as for TSFF_ANG_SPH; dvx = vx[1] - vx[0]; nv = 2 .. 4096.  The scratch is the handle's
 * and is sized on the first call at a given size: later calls allocate nothing.  Refusals as for TSFF_ANG_SPH; a null pointer -1. */
int tsff_sph_table(tsff_handle *h, int32_t sph_type, int32_t n_harm, int32_t nv, int32_t nvr, int32_t n_gen, double dvx,
                   const double *theta, const double *gen_data, double *fe);
int tsff_sph_table_vjp(tsff_handle *h, int32_t sph_type, int32_t n_harm, int32_t nv, int32_t nvr, int32_t n_gen, double dvx,
                       const double *theta, const double *gen_data, const double *fe_bar, double *grad);

/* The free-form 1-D generator on its own (k_arb1v.inc; the kernels of TSFF_ANG_ARB1V), asynchronous on the handle's stream:
 *   tsff_arb1v_table:     fval (device [nv]) -> fe (device [nv]) = Arbitrary1V.__call__() (distribution.arbitrary_1v);
 *   tsff_arb1v_table_vjp: fval, fe_bar (device [nv]) = d loss / d fe -> grad (device [nv]) = d loss / d fval
 *   (distribution.arbitrary_1v_vjp), bit-reproducible from run to run (every sum in a fixed order, no atomics).
 * gen_data (device): S[nv][nv] | S^T[nv][nv]; dvx = vx[1] - vx[0]; nv = 4 .. 4096 (need not be the handle's nvx).  The matrix
 * products run one wavefront per row on (nv + 3) / 4 workgroups.  The scratch (2 nv doubles) is the handle's and is sized on the
 * first call at a given size: later calls allocate nothing.  Refusals: a null pointer -1, nv outside 4 .. 4096 -2. */
int tsff_arb1v_table(tsff_handle *h, int32_t nv, double dvx, const double *fval, const double *gen_data, double *fe);
int tsff_arb1v_table_vjp(tsff_handle *h, int32_t nv, double dvx, const double *fval, const double *gen_data, const double *fe_bar,
                         double *grad);

/* Exact per-lineout Hessian of the fit loss: LossFunction._loss_for_hess_fn_ / h_loss_wrt_params
 * (inverse/loss_function.py:170-188, equinox.filter_hessian) for every lineout b, with respect to the normalised leaves
 * of the slots active_slots (HOST [n_active], ravel order).  The loss uses the denominators |data| + 1e-10 of
 * loss_function.py:183 for l1 / l2, WHATEVER TSFF_OPT_DENOM_MODE says, sum reduce and the deck's loss_method.
 *   weights (HOST [3]): as tsff_loss_grad (w_iaw, w_blue, w_red; w_blue = w_red = 1/2 halves e_error when both EPW ranges
 *   are fitted, loss_function.py:262-264);
 *   loss_terms (device [3]): un-weighted masked sums S_iaw, S_blue, S_red over the B lineouts;
 *   grad (device [B][n_active]) and hess (device [B][n_active][n_active], symmetric): of sum_k weights[k] S_k.
 * active_slots takes exactly the slots tsff_loss_grad takes in grad_mask: a slot out of range or repeated returns -1,
 * TSFF_P_M without fe_mode == TSFF_FE_DLM -2, an ion's A slot -3; -2 as well when the tables of the path exceed the LDS
 * of a workgroup (large nvx).  With TSFF_P_M active the second m-derivatives of the DLM tables are built per lineout
 * (base.py:277-294: linear in m inside a cell, divided by its own sum).  Second-order forward mode (hyper-dual numbers)
 * per (lineout, pair of active leaves): a fixed set of launches whatever n_active. */
int tsff_loss_hess(tsff_handle *h, const double *params, const double *fe, const double *e_data, const double *i_data,
                   const double *e_amps, const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                   const double *weights, const int32_t *active_slots, int32_t n_active, double *loss_terms,
                   double *grad, double *hess);

/* Exact Hessian of the angular (ARTS) loss: LossFunction._loss_for_hess_fn_ / h_loss_wrt_params (inverse/loss_function.py:170-188,
 * which process_angular_data -> recalculate_with_chosen_weights calls after an angular fit, postprocess.py:131-135) on an
 * angular_full deck with a 1-D f_e: value, gradient and full second derivative of
 *   loss = sum_j wcol[column of j] l(e_data_j, t_j),   t = ThryE + noise_e,
 * w.r.t. the normalised leaves of the slots active_slots (HOST [n_active], ravel order; TSFF_P_M included on a DLM handle), in one
 * stream-ordered call.  l is the functional of tsff_loss_hess with its denominators (|d| + 1e-10 for l2 and l1) for loss_method
 * (TSFF_LOSS_*, whatever the handle's own); wcol (device [npts / lam_step]) carries the blue / red masks of the resolution-unit axis.
 *   leaves (device [NP]): the normalised leaf row of the one plasma condition; fe (device [nvx]) as the handle's fe_mode says
 *   (PER_LINEOUT: the table; SHARED / DLM: NULL, the DLM table is built from the leaves);
 *   e_data, noise_e (device [rows][npts / lam_step]; noise_e may be NULL = 0), e_amps (device [rows]);
 *   loss (device [1]), grad (device [n]), hess (device [n][n], symmetric, both triangles written),
 *   gn (device [n][n]) = sum_j w_j l''(d_j, t_j) t_a t_c, the Gauss-Newton part of hess on its own;
 *   optional outputs (device, NULL to skip): E [rows][nJ] the model image (bit for bit tsff_ats_spectrum of tsff_form_factor at the
 *   physical parameters `phys`), E1 [n][rows][nJ] its first and E2 [n (n + 1) / 2][rows][nJ] its second derivatives, the pairs
 *   (a <= c) row-major over the upper triangle; phys [NP] the physical parameters of the leaves.
 * Second-order forward mode: k_ffhess evaluates the raw form factor in hyper-dual arithmetic, one task per pair of leaves that
 * reach it (a pair with amp1, amp2 or amp3 has a vanishing second derivative of P and launches none), with tsff_loss_hess's table
 * convention (the Z' and W lookups carry their slope and no curvature, the Hermite ln f_e lookup its true derivatives, the DLM
 * table piecewise linear in m before its normalisation); the linear stages of the ARTS chain run on every derivative image and the
 * two row normalisations take their second derivative at the arg-max of the value.  Every sum runs in a fixed order, no atomics:
 * two calls give bit-identical output.  Nothing synchronises inside the call; its workspace is the handle's and grows only when a
 * call needs more than the last one (refused with -2 inside graph capture, as tsff_reserve describes).
 * Refusals, each with a tsff_last_error message and nothing enqueued: a null pointer, n_active < 1 or an unknown loss_method -1;
 * a slot out of range or repeated -1, TSFF_P_M without fe_mode == TSFF_FE_DLM -2, an ion's A slot -3; fe missing on a PER_LINEOUT
 * handle (among them the handles of 2-D f_e decks, which this call does not serve) -2; tsff_ats_setup not called -2; the tables
 * of k_ffhess beyond the LDS of a workgroup (large nvx) -2. */
int tsff_angular_loss_hess(tsff_handle *h, const double *leaves, const double *fe, const int32_t *active_slots, int32_t n_active,
                           const double *e_data, const double *noise_e, const double *e_amps, const double *wcol, int32_t loss_method,
                           double *loss, double *grad, double *hess, double *gn, double *E, double *E1, double *E2, double *phys);

/* Jacobian of the model spectra w.r.t. the normalised leaves of the slots active_slots (HOST [n_active], ravel order), for every
 * lineout b:  jac_f[b][a][j] = d Thry_f[b][j] / d x[b][a], Thry_f what tsff_forward returns for the same arguments without the
 * additive noise (jax.jacfwd of ThomsonScatteringDiagnostic.__call__; the reference has no such call).
 *   jac_e, jac_i (device [B][n_active][1024] each): either may be NULL (that feature is then not evaluated and nothing of it is
 *   written); asking for the Jacobian of a feature that is not loaded returns -1, as does asking for neither.
 * The chain and table convention of tsff_loss_hess (Z' and W lookups carry their slope, the Hermite ln f_e lookup its true
 * derivative), in one of two forms that tsff_last_launch names as k_jac_sweep<n_ion, W, rows>:
 *   rows (1-2 ion species, one gradient point, TSFF_P_M not a leaf, both features through their instrument response): per point
 *     the value and the reverse of the pair-sweep kernels give each sample's row w.r.t. the lineout scalars, which is contracted
 *     with the scalars' tangents w.r.t. the leaves -- about two forward calls whatever n_active;
 *   tangents (everything else): first-order forward mode, a value and a group of W tangents side by side per point, the groups of
 *     leaves one after the other.  W = 3; W = 1 for a single leaf or when the spectrum with three tangents exceeds the LDS (e.g.
 *     5 points per pixel) -- one full sweep per leaf then, no faster than central differences.
 * Slots: as tsff_loss_hess (-1 out of range or repeated, -2 TSFF_P_M without TSFF_FE_DLM, -3 an ion's A slot); -2 when the
 * tables and the spectrum of the narrowest group exceed the LDS of a workgroup.  Every sum runs in a fixed order: two calls give
 * bit-identical output. */
int tsff_spectrum_jacobian(tsff_handle *h, const double *params, const double *fe, const double *e_amps, const double *i_amps,
                           int32_t B, const int32_t *active_slots, int32_t n_active, double *jac_e, double *jac_i);

/* Gauss-Newton curvature of the loss of tsff_loss_hess (denominators |data| + 1e-10 for l2 whatever TSFF_OPT_DENOM_MODE says,
 * sum reduce), per lineout b, from the Jacobian above without writing it to memory:
 *   gn[b][a][c] = sum_k weights[k] sum_{j in mask_k} l''(d_j, t_j) J[a][j] J[c][j]     (device [B][n_active][n_active], symmetric,
 *                 positive semi-definite; l'' = 2 / (|d| + 1e-10) for l2, sech^2(d - t) for log-cosh, d / t^2 for poisson),
 *   grad[b][a]  = sum_k weights[k] sum_{j in mask_k} dl/dt(d_j, t_j) J[a][j]           (device [B][n_active]; tsff_loss_hess's grad),
 *   loss_terms (device [3]): the un-weighted masked sums S_iaw, S_blue, S_red over the B lineouts.
 * weights (HOST [3]) and the refusals are those of tsff_loss_hess and tsff_spectrum_jacobian; loss_method l1 returns -2 (its
 * l'' is zero: the Gauss-Newton matrix of an l1 fit vanishes). */
int tsff_loss_gauss_newton(tsff_handle *h, const double *params, const double *fe, const double *e_data, const double *i_data,
                           const double *e_amps, const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                           const double *weights, const int32_t *active_slots, int32_t n_active, double *loss_terms,
                           double *grad, double *gn);

/* Every lineout of a 1-D batch fitted on its own by Levenberg-Marquardt (damped Gauss-Newton steps, Nielsen's damping: Madsen,
 * Nielsen and Tingleff, "Methods for Non-Linear Least Squares Problems", 2004, Algorithm 3.16), on the device: n_evals x (the
 * sweep of tsff_loss_gauss_newton -- per lineout b the loss F_b = (w[0] S_iaw[b] + w[1] S_blue[b]) + w[2] S_red[b], its gradient
 * and its Gauss-Newton matrix at params -- then one launch of k_lm_step, one wavefront per lineout), all enqueued on the handle's
 * stream; the call returns once they are enqueued (no synchronisation, allocation or upload between the evaluations).  The
 * reference has no such optimiser; its 1-D loops treat the batch as one joint problem.  The method is restated on the host in
 * tsadar_amd/lm.py, and the device reproduces that restatement bit for bit (ordered sums, nothing fused; k_lm.inc).
 *   params (device [B][NP], in/out): normalised leaves; k_lm_step writes each lineout's next trial point into the active slots,
 *   and its accepted point once the lineout's status is terminal;
 *   fe, e_data .. noise_i, B, weights, active_slots, n_active: as tsff_loss_gauss_newton, with its refusals (a slot out of range
 *   or repeated -1, TSFF_P_M without fe_mode == TSFF_FE_DLM -2, an ion's A slot -3, loss_method l1 -2, the LDS budget -2).  The
 *   loss is the fit loss: with TSFF_OPT_DENOM_MODE 0 the l2 denominators are constants that the weights carry (e = r^2; the
 *   Gauss-Newton matrix is then the exact Hessian of the quadratic model), with mode 2 they are |d| + 1e-10 per sample, as in
 *   tsff_loss_gauss_newton; log-cosh and poisson have none;
 *   opts (HOST [7]): tau (> 0: the first damping is tau max_a H[a][a]), gtol, ftol, xtol (>= 0), maxiter, maxfun (whole
 *   numbers >= 0), lambda_max (> 0), all finite;
 *   state (device [n_state], in/out), n_state >= tsff_lm_state_size(B, n_active), else -1:
 *     [status int32 x B, padded to a whole double | B records], the record of lineout b being
 *     [f, lam, nu, pred, nit, nfev, 0, 0 | x[n_active] | g[n_active] | A[n_active][n_active]]
 *     -- the accepted point with its loss, gradient and Gauss-Newton matrix, the damping and its growth factor, the reduction the
 *     model predicts for the trial point now in params, and the counts (whole numbers held as doubles).  All zeros starts a fit
 *     at params.  status: 0 running, 1 max|g| <= gtol, 2 a step accepted with f_old - F <= ftol f_old, 3 ||delta|| <= xtol
 *     (||x|| + xtol), 4 nit >= maxiter or nfev >= maxfun, 5 no acceptable step (lam > lambda_max, or lam no longer positive), 6 the first F is not finite.
 *     A lineout whose status is not 0 is passed over by every later evaluation (its status word is the sweep's skip flag) and
 *     nothing of it changes.  Chunks of 5 + 4 + 3 evaluations on one state are bit for bit one call of 12;
 *   x_hist (device [n_evals][B][n_active] or NULL): the point each evaluation ran at;
 *   eval_hist (device [n_evals][B][1 + n_active + n_active^2] or NULL): its F | G | H.  Both hold NaN for a lineout that was
 *   terminal before the evaluation.
 * n_evals == 0 returns 0 and enqueues nothing; n_evals < 0, a null params, weights, active_slots, opts or state, a bad option
 * or a short state returns -1. */
int tsff_lm_state_size(int32_t B, int32_t n_active, int64_t *n_doubles);
int tsff_lm_fit(tsff_handle *h, double *params, const double *fe, const double *e_data, const double *i_data, const double *e_amps,
                const double *i_amps, const double *noise_e, const double *noise_i, int32_t B, const double *weights,
                const int32_t *active_slots, int32_t n_active, int32_t n_evals, const double *opts, double *state, int64_t n_state,
                double *x_hist, double *eval_hist);


/* The same plus the gradient w.r.t. the tabulated distribution function itself: grad_fe [B][nvx] (device) =
 * d loss / d fe[b][i], for fe_mode == TSFF_FE_PER_LINEOUT.  This is what equinox.filter_value_and_grad returns for the
 * leaves of a free-form distribution (Arbitrary1V.fval, core/modules/distribution_functions/base.py:157-204, filter
 * spec :462-471) before the generator's own chain rule, which stays on the host.  The adjoint runs through both uses of
 * f_e: the Hermite interpolant of ln f_e at the phase velocity (form_factor.py:256) and the Re(chi_e) table
 * (form_factor.py:263-268, ratintn.py) via one transposed GEMM with the constant log-ratio table. */
int tsff_loss_grad_fe(tsff_handle *h, const double *params, const double *fe, const double *e_data, const double *i_data,
                      const double *e_amps, const double *i_amps, const double *noise_e, const double *noise_i, int32_t B,
                      const double *weights, const uint8_t *grad_mask, double *loss_terms, double *grad, double *grad_fe,
                      double *ThryE, double *ThryI);

/* The packed buffer of a free-form f_e fit step from the outputs of tsff_loss_grad_fe (all device pointers):
 * packed = [loss_terms[0..3) | rows x B_global], rows = the n_active scalar leaves (grad[b][active_slots[k]]) followed by the
 * nvx values d loss / d fe[b][i] -- the ravel order of the optimiser's flat vector before the generator's chain rule (which
 * stays on the host) --, this rank's columns [b_offset, b_offset + B) filled and every other column ZERO, so that the buffer
 * is all-reduced in place like the one of tsff_loss_grad_packed (inverse/loops.py:40-54; form_factor.py:431-447 for the sharding). */
int tsff_pack_fe_rows(tsff_handle *h, const double *loss_terms, const double *grad, const double *grad_fe, int32_t B,
                      const int32_t *active_slots, int32_t n_active, int64_t B_global, int64_t b_offset, double *packed);

/* LossFunction.array_loss: per-lineout masked sums with the theory spectrum as denominator
 * ((d-t)^2/t, loss_function.py:320-321).  sums [B][3] = S_iaw, S_blue, S_red per lineout;
 * sqdev_e / sqdev_i [B][1024] (may be NULL) = nan_to_num'ed error arrays (:238,250,264). */
int tsff_array_loss(tsff_handle *h, const double *params, const double *fe, const double *e_data,
                    const double *i_data, const double *e_amps, const double *i_amps,
                    const double *noise_e, const double *noise_i, int32_t B, double *sums,
                    double *sqdev_e, double *sqdev_i, double *ThryE, double *ThryI);

/* HIP-event timing of the main kernel of tsff_forward / tsff_loss_grad(_packed, _fe) / tsff_array_loss (k_spectrum or
 * k_spectrum_fused) and of tsff_form_factor_2d(_range, _save) (k_form_factor_2d) on the handle's stream.  tsff_enable_timing(h, ring) keeps one event pair per
 * launch in a ring of `ring` entries (0 disables); tsff_kernel_times returns the durations [ms] of
 * the most recent min(ring, launches, max_n) launches, oldest first, and synchronises on them. */
int tsff_enable_timing(tsff_handle *h, int32_t ring);
int tsff_kernel_times(tsff_handle *h, float *ms, int32_t max_n, int32_t *n_out);

/* micro-benchmark: sustained FP64 vector FMA rate of this device in TFLOP/s (the roof the path is bound by;
 * AMD's datasheet figure for MI355X is 78.6).  Synchronous. */
int tsff_fp64_fma_peak(tsff_handle *h, double *tflops);
/* the same on the FP64 matrix cores (v_mfma_f64_16x16x4_f64), the roof of k_wgemm */
int tsff_fp64_mfma_peak(tsff_handle *h, double *tflops);
/* micro-benchmark: sustained read rate of the vector L1 (every wavefront re-reads a 16 KB window with 16-byte loads) in
 * TB/s over the whole device -- the roof of the 2-D sampler when its table is read through L1/L2 (nv > 128) */
int tsff_l1_read_peak(tsff_handle *h, double *tbps);

#ifdef __cplusplus
}
#endif
#endif /* TSFF_H */
