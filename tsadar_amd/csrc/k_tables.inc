// k_tables.inc -- distribution-function tables: Hermite ln f_e table, Re(chi_e) table W (direct and as an FP64 MFMA GEMM), their adjoints.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).

// ------------------------------------------------------------------------------------------
// The numerical steps of the table builders (k_fe_prepare, k_fe_vectors, fe_direction_rows, k_hess_mtab; k_fe_adjoint walks them
// backwards), each stated once
// ------------------------------------------------------------------------------------------
// A kernel's Tables on the handle's vx grid: the tables it has (nullptr: none), no m-tangents, no adjoints, polynomial exp
__device__ __forceinline__ Tables make_tables(const KStatic& S, const double2* zp, const double* Wt, const double2* ht, const double2* hc) {
  Tables T;
  T.zp = zp; T.W = Wt; T.ht = ht; T.hc = hc; T.hcm = nullptr; T.Wm = nullptr; T.Wb = T.Hy = T.Hs = nullptr; T.etab = nullptr;
  tables_set_grid(T, S.vx0, S.dv, S.nvx);
  return T;
}

// slope at node i of the nodal array y [n] with spacing dv: mean of the adjacent secants, one-sided at the ends (interpax _approx_df)
__device__ __forceinline__ double node_slopes(const double* y, int i, int n, double dv) {
  const double dl = i > 0 ? (y[i] - y[i - 1]) / dv : 0.0, dr = i < n - 1 ? (y[i + 1] - y[i]) / dv : 0.0;
  return i == 0 ? dr : (i == n - 1 ? dl : 0.5 * (dl + dr));
}

// ratdf = gradient(ratmod, dxi1) (form_factor.py:264): central differences on the uniform xi1 grid, one-sided at the ends.
// All threads; no barrier.
__device__ __forceinline__ void ratdf_central(const double* xi1, const double* rat, double* rdf) {
  const double h1 = xi1[1] - xi1[0];
  for (int i = threadIdx.x; i < kNXi1; i += kThreads) {
    double g;
    if (i == 0) g = (rat[1] - rat[0]) / h1;
    else if (i == kNXi1 - 1) g = (rat[i] - rat[i - 1]) / h1;
    else g = (rat[i + 1] - rat[i - 1]) / (2.0 * h1);
    rdf[i] = g;
  }
}

// interval i of the xi1 grid as the W-table GEMM sees it: 1 / h_i and the midpoint (ratintn drops the last interval: i < 1022)
__device__ __forceinline__ void xi1_cell(const double* xi1, int i, double& ih, double& mid) {
  const double x0 = xi1[i], x1 = xi1[i + 1];
  ih = 1.0 / (x1 - x0); mid = 0.5 * (x1 + x0);
}

// ratdf -> the (A, s) rows of the W-table GEMM, XA / XB [1024] zero padded: s_i = fdif_i / h_i, A_i = fav_i - xi1mid_i s_i.  All
// threads; returns this thread's part of sum fdif (the caller block_sums it); no barrier.
__device__ __forceinline__ double ratdf_rows(const double* xi1, const double* rdf, double* __restrict__ XA, double* __restrict__ XB) {
  double c = 0.0;
  for (int i = threadIdx.x; i < kNXi1; i += kThreads) {
    double A = 0.0, Bs = 0.0;
    if (i < kNXi1 - 2) {
      double ih, mid;
      xi1_cell(xi1, i, ih, mid);
      const double fd = rdf[i + 1] - rdf[i], fa = 0.5 * (rdf[i + 1] + rdf[i]);
      Bs = fd * ih; A = fa - mid * Bs;
      c += fd;
    }
    XA[i] = A; XB[i] = Bs;
  }
  return c;
}

// DLM1V.__call__ (base.py:277-294) interpolates in the order m over m_ax = linspace(2, 5, 31): the cell of lineout xpar's m, the
// weight t in it, and whether m lies inside the axis (jnp.interp clamps outside: zero slope there)
struct DlmCell { int k; double t; bool inside; };
template <int NI>
__device__ __forceinline__ DlmCell dlm_cell(const KStatic& S, const double* __restrict__ xpar) {
  Phys<NI> p;
  load_phys<NI>(xpar, S.p_scale, S.p_shift, S.p_sig, S.ti_same, true, p);
  const double m = p.m;
  double u = (m - 2.0) * 10.0;
  int k = (int)u;
  k = k < 0 ? 0 : (k > TSFF_DLM_NM - 2 ? TSFF_DLM_NM - 2 : k);
  double t = (m - (2.0 + 0.1 * k)) * 10.0;
  t = m < 2.0 ? 0.0 : (m > 5.0 ? 1.0 : t);
  return DlmCell{k, t, m >= 2.0 && m <= 5.0};
}
// node i of the un-normalised f_e in that cell and its derivative w.r.t. m
__device__ __forceinline__ void dlm_node(const KStatic& S, const DlmCell& c, int i, double& f, double& df) {
  const double a = S.dlm_table[i * TSFF_DLM_NM + c.k], b = S.dlm_table[i * TSFF_DLM_NM + c.k + 1];
  f = a + c.t * (b - a);
  df = c.inside ? (b - a) * 10.0 : 0.0;
}

// ------------------------------------------------------------------------------------------
// k_fe_prepare: distribution function -> Hermite table of ln fe and the Re(chi_e) table W
// grid (slots, qsplit), 256 threads.   reference: form_factor.py:263-268, ratintn.py:4-52,
// base.py:277-294 (DLM), interpax _approx_df (node slopes)
// ------------------------------------------------------------------------------------------
template <int NI>
__global__ __launch_bounds__(kThreads) void k_fe_prepare(KStatic S, const double* __restrict__ fe_in, int fe_mode,
                                                         const double* __restrict__ params, double2* __restrict__ ht_out,
                                                         double* __restrict__ W_out, double* __restrict__ fe_out) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* lnfe = reinterpret_cast<double*>(smem);  // [nvx]
  double* slope = lnfe + S.nvx;                    // [nvx]
  double* ratmod = slope + S.nvx;                  // [1024]
  double* ratdf = ratmod + kNXi1;                  // [1024]
  double* xi1 = ratdf + kNXi1;                     // [1024]
  double* red = xi1 + kNXi1;                       // [8]
  double2* ht = reinterpret_cast<double2*>(red + 8);  // [nvx]

  const int slot = blockIdx.x, tid = threadIdx.x;
  const int nvx = S.nvx;

  // ---- fe on the vx grid ----
  if (fe_mode == TSFF_FE_DLM) {
    // DLM1V.__call__ (base.py:277-294): interp in m, then /sum/dv
    const DlmCell cell = dlm_cell<NI>(S, params + (size_t)slot * S.NP);
    double part = 0.0;
    for (int i = tid; i < nvx; i += kThreads) {
      double f, df;
      dlm_node(S, cell, i, f, df);
      lnfe[i] = f;
      part += f;
    }
    const double tot = block_sum(part, red);
    for (int i = tid; i < nvx; i += kThreads) {
      const double f = lnfe[i] / tot / S.dv;
      if (fe_out && blockIdx.y == 0) fe_out[(size_t)slot * nvx + i] = f;
      lnfe[i] = log(f);
    }
  } else {
    for (int i = tid; i < nvx; i += kThreads) lnfe[i] = log(fe_in[(size_t)slot * nvx + i]);
  }
  for (int i = tid; i < kNXi1; i += kThreads) xi1[i] = S.xi1[i];
  __syncthreads();
  // ---- node slopes ----
  for (int i = tid; i < nvx; i += kThreads) {
    const double s = node_slopes(lnfe, i, nvx, S.dv);
    slope[i] = s;
    ht[i] = make_double2(lnfe[i], s);
    if (blockIdx.y == 0) ht_out[(size_t)slot * nvx + i] = make_double2(lnfe[i], s);
  }
  __syncthreads();
  const Tables T = make_tables(S, nullptr, nullptr, ht, nullptr);
  // ---- ratmod = exp(H(xi1)) (form_factor.py:263) ----
  for (int i = tid; i < kNXi1; i += kThreads) {
    double H, dH;
    hermite_lookup(T, xi1[i], H, dH);
    ratmod[i] = exp(H);
  }
  __syncthreads();
  ratdf_central(xi1, ratmod, ratdf);
  __syncthreads();
  // ---- W[q] = ratintn(ratdf, xi1 - xi2[q], xi1): one wavefront per q, lanes stride the 1022
  //      intervals, xor-shuffle reduction (ratintn.py:21, 41-52; the last interval is dropped) ----
  const int lane = tid & 63, wave = tid >> 6;
  const int qper = (kNXi2 + gridDim.y - 1) / gridDim.y;
  const int q0 = blockIdx.y * qper, q1 = min(kNXi2, q0 + qper);
  for (int q = q0 + wave; q < q1; q += kThreads / 64) {
    const double x2 = S.xi2[q];
    double acc = 0.0;
    for (int i = lane; i < kNXi1 - 2; i += 64) {
      const double f0 = ratdf[i], f1 = ratdf[i + 1];
      const double g0 = xi1[i] - x2, g1 = xi1[i + 1] - x2;
      const double fdif = f1 - f0, gdif = g1 - g0;
      const double fav = 0.5 * (f1 + f0), gav = 0.5 * (g1 + g0);
      const double tmp = fav * gdif - gav * fdif;
      double r;
      if (fabs(gdif) < 1.0e-4 * fabs(gav)) r = fav / gav + tmp * gdif / (12.0 * gav * gav * gav);
      else r = fdif / gdif + tmp * log(fabs((gav + 0.5 * gdif) / (gav - 0.5 * gdif))) / (gdif * gdif);
      acc += r * (xi1[i + 1] - xi1[i]);
    }
    acc = wave_sum(acc);
    if (lane == 0) W_out[(size_t)slot * kNXi2 + q] = acc;
  }
}

// ------------------------------------------------------------------------------------------
// Per-lineout distribution functions (fe_mode DLM / PER_LINEOUT).  The Re(chi_e) table is linear in
// ratdf: with h_i = xi1[i+1]-xi1[i], s_i = fdif_i/h_i, A_i = fav_i - xi1mid_i s_i,
//   W[q] = sum_i fdif_i + sum_i Lg[q][i] (A_i + xi2[q] s_i),   Lg[q][i] = log|(gav+gdif/2)/(gav-gdif/2)|
// (ratintn.py:41-52 with gdif = zdif; the small-gdif branch never triggers on this grid).  Lg is a
// constant 1640x1022 table, so the 1.68 M logarithms per f_e of k_fe_prepare become two matrix-vector
// products per lineout, done for the whole batch by k_wgemm.  The derivative with respect to the DLM
// order m rides along as a second pair of vectors (tangent of f_e -> ln f_e -> ratmod -> ratdf).
//
// k_fe_vectors: grid B, 256 threads.  Outputs ht/htm [B][nvx], X [B][4][1024] = (A, s, dA/dm, ds/dm) zero
// padded, cst [B][2] = (sum fdif, d/dm).
// ------------------------------------------------------------------------------------------
// fe_direction_rows: the tangent of a lineout's tables along one direction of ln f_e, given at the nodes (dln [nvx], LDS) -- the
// DLM order m for k_fe_vectors, any direction of f_e for k_fe_direction.  All threads; T: the lineout's own ln f_e table (hc filled),
// rat [1024]: ratmod = exp(H(xi1)) of the lineout.  Leaves (d ln f_e, its node slope) in htm / htm_out and their Hermite
// coefficients in hcm, ratmod' = ratmod H'(xi1) (zero outside the grid) and its central differences in ratm / rdfm, the (A, s) rows
// of the W-table GEMM in XA / XB [1024], and returns this thread's part of sum fdif' (the caller block_sums it).  Ends without a barrier.
__device__ __forceinline__ double fe_direction_rows(const KStatic& S, const Tables& T, const double* dln, const double* rat, double2* htm,
                                                    double2* hcm, double* ratm, double* rdfm, double2* __restrict__ htm_out,
                                                    double* __restrict__ XA, double* __restrict__ XB) {
  const int tid = threadIdx.x, nvx = S.nvx;
  for (int i = tid; i < nvx; i += kThreads) {
    htm[i] = make_double2(dln[i], node_slopes(dln, i, nvx, S.dv));
    htm_out[i] = htm[i];
  }
  __syncthreads();
  for (int i = tid; i < nvx - 1; i += kThreads) hermite_coeffs(htm[i], htm[i + 1], S.dv, hcm[2 * i], hcm[2 * i + 1]);
  __syncthreads();
  Tables Tm = T;
  Tm.hc = hcm;
  for (int i = tid; i < kNXi1; i += kThreads) {
    const double x = S.xi1[i];
    double Hm, dHm;
    hermite_lookup_c(Tm, x, Hm, dHm);
    const bool out = x < T.vx0 || x > T.vxlast;
    ratm[i] = out ? 0.0 : rat[i] * Hm;
  }
  __syncthreads();
  ratdf_central(S.xi1, ratm, rdfm);
  __syncthreads();
  return ratdf_rows(S.xi1, rdfm, XA, XB);
}

template <int NI>
__global__ __launch_bounds__(kThreads) void k_fe_vectors(KStatic S, const double* __restrict__ fe_in, int fe_mode,
                                                         const double* __restrict__ params, double2* __restrict__ ht_out,
                                                         double2* __restrict__ htm_out, double* __restrict__ X,
                                                         double* __restrict__ cst) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* ht = reinterpret_cast<double2*>(smem);         // [nvx]
  double2* htm = ht + S.nvx;                              // [nvx]
  double2* hc = htm + S.nvx;                              // [2 nvx]
  double2* hcm = hc + 2 * S.nvx;                          // [2 nvx]
  double* lnfe = reinterpret_cast<double*>(hcm + 2 * S.nvx);  // [nvx]
  double* dln = lnfe + S.nvx;                             // [nvx]
  double* rat = dln + S.nvx;                              // [1024] ratmod -> ratdf
  double* ratm = rat + kNXi1;                             // [1024]
  double* rdf = ratm + kNXi1;                             // [1024]
  double* rdfm = rdf + kNXi1;                             // [1024]
  double* red = rdfm + kNXi1;                             // [8]
  const int b = blockIdx.x, tid = threadIdx.x, nvx = S.nvx;

  if (fe_mode == TSFF_FE_DLM) {
    const DlmCell cell = dlm_cell<NI>(S, params + (size_t)b * S.NP);
    double part = 0.0, dpart = 0.0;
    for (int i = tid; i < nvx; i += kThreads) {
      double f, df;
      dlm_node(S, cell, i, f, df);
      lnfe[i] = f;
      dln[i] = df;
      part += f;
      dpart += df;
    }
    const double tot = block_sum(part, red);
    const double dtot = block_sum(dpart, red);
    for (int i = tid; i < nvx; i += kThreads) {
      const double f = lnfe[i];
      dln[i] = dln[i] / f - dtot / tot;               // d ln fe / dm
      lnfe[i] = log(f / tot / S.dv);                  // base.py:293
    }
  } else {
    for (int i = tid; i < nvx; i += kThreads) { lnfe[i] = log(fe_in[(size_t)b * nvx + i]); dln[i] = 0.0; }
  }
  __syncthreads();
  for (int i = tid; i < nvx; i += kThreads) {
    ht[i] = make_double2(lnfe[i], node_slopes(lnfe, i, nvx, S.dv));
    ht_out[(size_t)b * nvx + i] = ht[i];
  }
  __syncthreads();
  for (int i = tid; i < nvx - 1; i += kThreads) hermite_coeffs(ht[i], ht[i + 1], S.dv, hc[2 * i], hc[2 * i + 1]);
  __syncthreads();
  const Tables T = make_tables(S, nullptr, nullptr, ht, hc);
  for (int i = tid; i < kNXi1; i += kThreads) {
    double H, dH;
    hermite_lookup_c(T, S.xi1[i], H, dH);
    rat[i] = exp(H);
  }
  __syncthreads();
  ratdf_central(S.xi1, rat, rdf);
  double* Xb = X + (size_t)b * 4 * kNXi1;
  // the m direction (its barriers publish rdf as well)
  double c1 = fe_direction_rows(S, T, dln, rat, htm, hcm, ratm, rdfm, htm_out + (size_t)b * nvx, Xb + 2 * kNXi1, Xb + 3 * kNXi1);
  double c0 = ratdf_rows(S.xi1, rdf, Xb, Xb + kNXi1);
  c0 = block_sum(c0, red);
  c1 = block_sum(c1, red);
  if (tid == 0) { cst[2 * b] = c0; cst[2 * b + 1] = c1; }
}

// k_fe_direction: the table tangents of tsff_form_factor_jvp.  grid (n_dir * B), 256 threads; workgroup d * B + b takes direction d of
// lineout b: d ln f_e = fe_dot / fe at the nodes, then fe_direction_rows, the body k_fe_vectors runs for the DLM order.  Outputs, all
// indexed by r = d * B + b: htd [r][nvx] = (d ln f_e, its node slope), X [r][4][1024] = (A', s', 0, 0) and cst [r][2] = (sum fdif', 0)
// -- the layout of the GEMM without m-tangents (k_wgemm<2>), which returns W' [r][1640] in place of W.
__global__ __launch_bounds__(kThreads) void k_fe_direction(KStatic S, const double* __restrict__ fe, const double* __restrict__ fe_dot,
                                                           const double2* __restrict__ ht_in, int B, double2* __restrict__ htd_out,
                                                           double* __restrict__ X, double* __restrict__ cst) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* ht = reinterpret_cast<double2*>(smem);         // [nvx]   (the layout of k_fe_vectors)
  double2* htm = ht + S.nvx;                              // [nvx]
  double2* hc = htm + S.nvx;                              // [2 nvx]
  double2* hcm = hc + 2 * S.nvx;                          // [2 nvx]
  double* lnfe = reinterpret_cast<double*>(hcm + 2 * S.nvx);  // [nvx] (unused here)
  double* dln = lnfe + S.nvx;                             // [nvx]
  double* rat = dln + S.nvx;                              // [1024]
  double* ratm = rat + kNXi1;                             // [1024]
  double* rdf = ratm + kNXi1;                             // [1024] (unused here)
  double* rdfm = rdf + kNXi1;                             // [1024]
  double* red = rdfm + kNXi1;                             // [8]
  const int r = blockIdx.x, b = r % B, tid = threadIdx.x, nvx = S.nvx;
  for (int i = tid; i < nvx; i += kThreads) {
    ht[i] = ht_in[(size_t)b * nvx + i];
    dln[i] = fe_dot[(size_t)r * nvx + i] / fe[(size_t)b * nvx + i];
  }
  __syncthreads();
  for (int i = tid; i < nvx - 1; i += kThreads) hermite_coeffs(ht[i], ht[i + 1], S.dv, hc[2 * i], hc[2 * i + 1]);
  __syncthreads();
  const Tables T = make_tables(S, nullptr, nullptr, ht, hc);
  for (int i = tid; i < kNXi1; i += kThreads) {
    double H, dH;
    hermite_lookup_c(T, S.xi1[i], H, dH);
    rat[i] = exp(H);
  }
  __syncthreads();
  double* Xr = X + (size_t)r * 4 * kNXi1;
  double c1 = fe_direction_rows(S, T, dln, rat, htm, hcm, ratm, rdfm, htd_out + (size_t)r * nvx, Xr, Xr + kNXi1);
  for (int i = tid; i < kNXi1; i += kThreads) { Xr[2 * kNXi1 + i] = 0.0; Xr[3 * kNXi1 + i] = 0.0; }
  c1 = block_sum(c1, red);
  if (tid == 0) { cst[2 * r] = c1; cst[2 * r + 1] = 0.0; }
}

// k_wgemm: W[b][q] = c0_b + sum_i Lg[q][i] (A_b[i] + xi2[q] s_b[i]) and the same for d/dm: the GEMM
// C[v][q] = sum_k X[v][k] Lg[q][k] (v = 4 vectors per lineout, M = 4B, N = 1640, K = 1024) on the FP64 matrix
// cores (v_mfma_f64_16x16x4_f64).  256 threads = 2 x 2 wavefronts, 64 x 64 per wavefront (4 x 4 MFMA tiles, 64
// accumulator doubles per lane), 128 (vectors = 32 lineouts) x 128 (q) per workgroup, K in chunks of 16 staged
// K-major in LDS with the next chunk prefetched into registers.  Inside every 16-row MFMA tile the rows are ordered
// (component, lineout): a lane's four accumulators (rows (lane>>4) + 4 reg) are then (A, s, dA/dm, ds/dm)·Lg of ONE
// lineout and 16 consecutive q sit on 16 consecutive lanes, so the epilogue needs no shuffle and writes 128-B runs.
constexpr int kGM = 128, kGN = 128, kGK = 16, kGP = 132;  // kGP: LDS row pitch in doubles
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
// NC = 4: (A, s, dA/dm, ds/dm), 4 lineouts per 16-row tile.  NC = 2: no tangents (explicit f_e tables), 8 lineouts per
// tile, rows (component, lineout): a lane then holds (A, A', s, s') of lineouts fk and fk + 4.
// [klo, khi): the window of the K axis (xi1 index) outside which every X row is EXACTLY zero -- ratmod = exp(-50) is constant
// where xi1 and its neighbours lie outside the vx grid, so its central difference and with it A, s and their m-tangents
// vanish identically (tsff_create computes the window: 768 of the 1024 columns for the vx grid (-6, 6)); multiples of kGK.
template <int NC>
__global__ __launch_bounds__(kThreads, 2) void k_wgemm(const double* __restrict__ Lg, const double* __restrict__ X,
                                                    const double* __restrict__ cst, const double* __restrict__ xi2,
                                                    int B, double* __restrict__ W, double* __restrict__ Wm, int klo, int khi) {
  __shared__ double Xs[2][kGK][kGP];  // double-buffered: one barrier per K chunk
  __shared__ double Ls[2][kGK][kGP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order: workgroup L runs on XCD L % 8; the 13 q-tiles that share one X tile (and every Lg tile) are
  // given to the same XCD so that X is fetched into one L2 only.  Grid = 8 * ceil(nM / 8) * nQ workgroups.
  constexpr int nQ = (kNXi2 + kGN - 1) / kGN;
  const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
  const int mtile = xcd + 8 * (jx / nQ), qtile = jx % nQ;
  constexpr int LPT = 16 / NC;  // lineouts per 16-row MFMA tile
  if (mtile * (kGM / NC) >= B) return;
  const int q0 = qtile * kGN, b0 = mtile * (kGM / NC);
  // staging: thread -> LDS row lr, kGK/2 consecutive k starting at lk
  const int lr = tid >> 1, lk = (tid & 1) * (kGK / 2);
  constexpr int kPF = kGK / 4;  // double2 loads per thread and operand
  const int sb = b0 + (lr >> 4) * LPT + (lr & (LPT - 1)), sc = (lr & 15) / LPT;  // lineout / component of X row lr
  const double* __restrict__ xrow = X + ((size_t)min(sb, B - 1) * 4 + sc) * kNXi1 + lk;
  const double* __restrict__ lrow = Lg + (size_t)min(q0 + lr, kNXi2 - 1) * kNXi1 + lk;
  mfma_d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
  double2 px[kPF], pl[kPF];
#pragma unroll
  for (int j = 0; j < kPF; ++j) {
    px[j] = *reinterpret_cast<const double2*>(xrow + klo + 2 * j);
    pl[j] = *reinterpret_cast<const double2*>(lrow + klo + 2 * j);
  }
#pragma unroll
  for (int j = 0; j < kPF; ++j) {
    Xs[0][lk + 2 * j][lr] = px[j].x; Xs[0][lk + 2 * j + 1][lr] = px[j].y;
    Ls[0][lk + 2 * j][lr] = pl[j].x; Ls[0][lk + 2 * j + 1][lr] = pl[j].y;
  }
  __syncthreads();
  const int fr = lane & 15, fk = lane >> 4;
  int cur = 0;
  for (int k0 = klo; k0 < khi; k0 += kGK, cur ^= 1) {
    const bool more = k0 + kGK < khi;
    if (more) {
#pragma unroll
      for (int j = 0; j < kPF; ++j) {
        px[j] = *reinterpret_cast<const double2*>(xrow + k0 + kGK + 2 * j);
        pl[j] = *reinterpret_cast<const double2*>(lrow + k0 + kGK + 2 * j);
      }
    }
#pragma unroll
    for (int ks = 0; ks < kGK; ks += 4) {
      double a[4], c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = Xs[cur][ks + fk][wm * 64 + i * 16 + fr];
        c[i] = Ls[cur][ks + fk][wn * 64 + i * 16 + fr];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], c[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
#pragma unroll
      for (int j = 0; j < kPF; ++j) {
        Xs[cur ^ 1][lk + 2 * j][lr] = px[j].x; Xs[cur ^ 1][lk + 2 * j + 1][lr] = px[j].y;
        Ls[cur ^ 1][lk + 2 * j][lr] = pl[j].x; Ls[cur ^ 1][lk + 2 * j + 1][lr] = pl[j].y;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int u = 0; u < (NC == 4 ? 1 : 2); ++u) {
      const int bb = b0 + (wm * 4 + i) * LPT + fk + 4 * u;
      if (bb >= B) continue;
      const double c0 = cst[2 * bb], c1 = cst[2 * bb + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = q0 + wn * 64 + j * 16 + fr;
        if (q < kNXi2) {
          const double x2 = xi2[q];
          if (NC == 4) {
            W[(size_t)bb * kNXi2 + q] = c0 + acc[i][j][0] + x2 * acc[i][j][1];
            Wm[(size_t)bb * kNXi2 + q] = c1 + acc[i][j][2] + x2 * acc[i][j][3];
          } else {
            W[(size_t)bb * kNXi2 + q] = c0 + acc[i][j][u] + x2 * acc[i][j][2 + u];
          }
        }
      }
    }
  }
}

// k_wgemm_w: the same GEMM (NC = 4: with the m-tangents) tiled 128 x 144 per workgroup.  With 128 x 128 tiles the grid is
// 128 x 13 = 1664 workgroups at B = 4096 -- 3.25 rounds of the 512 that fit the device (two per CU), i.e. four rounds with the last one a
// quarter full: 19 % of the kernel is tail.  144 columns make 12 column tiles and 1536 workgroups = exactly three rounds (whatever
// B, the number of rounds is a multiple of 3/4 of what it was, never more).  Four wavefronts side by side along M, 32 x 144 each
// (2 x 9 MFMA tiles, 72 accumulator doubles per lane).  LDS rows of 144 doubles: a half wavefront reads two K rows x 16 columns, and
// 144 = 16 (mod 32) puts the second row into the other half of the banks.  Results are k_wgemm's bit for bit (same K order per element).
constexpr int kGNw = 144, kGPw = 144, kNTw = kGNw / 16;
constexpr size_t kWgemmWSmem = sizeof(double) * 4 * kGK * kGPw;
__global__ __launch_bounds__(kThreads, 2) void k_wgemm_w(const double* __restrict__ Lg, const double* __restrict__ X,
                                                      const double* __restrict__ cst, const double* __restrict__ xi2,
                                                      int B, double* __restrict__ W, double* __restrict__ Wm, int klo, int khi) {
  extern __shared__ __align__(16) unsigned char smem_w[];   // 2 x 2 x 16 x 144 doubles = 72 KB (dynamic: above the 64 KB of static LDS)
  typedef double (*stage_t)[kGK][kGPw];
  stage_t Xs = reinterpret_cast<stage_t>(smem_w);
  stage_t Ls = reinterpret_cast<stage_t>(smem_w + sizeof(double) * 2 * kGK * kGPw);
  constexpr int NC = 4, LPT = 16 / NC;
  const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
  constexpr int nQ = (kNXi2 + kGNw - 1) / kGNw;
  const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
  const int mtile = xcd + 8 * (jx / nQ), qtile = jx % nQ;   // (the q tiles that share one X tile on one XCD, as in k_wgemm)
  if (mtile * (kGM / NC) >= B) return;
  const int q0 = qtile * kGNw, b0 = mtile * (kGM / NC);
  // staging: rows 0..127 of both operands as in k_wgemm (thread -> row tid / 2, 8 consecutive k); rows 128..143 of Lg by threads 0..127
  const int lr = tid >> 1, lk = (tid & 1) * (kGK / 2);
  constexpr int kPF = kGK / 4;
  const int sb = b0 + (lr >> 4) * LPT + (lr & (LPT - 1)), sc = (lr & 15) / LPT;
  const double* __restrict__ xrow = X + ((size_t)min(sb, B - 1) * 4 + sc) * kNXi1 + lk;
  const double* __restrict__ lrow = Lg + (size_t)min(q0 + lr, kNXi2 - 1) * kNXi1 + lk;
  const int er = 128 + (tid >> 3), ek = (tid & 7) * 2;   // extra rows (tid < 128)
  const double* __restrict__ erow = Lg + (size_t)min(q0 + er, kNXi2 - 1) * kNXi1 + ek;
  const bool extra = tid < 128;
  mfma_d4 acc[2][kNTw];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < kNTw; ++j) acc[i][j] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
  double2 px[kPF], pl[kPF], pe = make_double2(0.0, 0.0);
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < kPF; ++j) {
      px[j] = *reinterpret_cast<const double2*>(xrow + k0 + 2 * j);
      pl[j] = *reinterpret_cast<const double2*>(lrow + k0 + 2 * j);
    }
    if (extra) pe = *reinterpret_cast<const double2*>(erow + k0);
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kPF; ++j) {
      Xs[buf][lk + 2 * j][lr] = px[j].x; Xs[buf][lk + 2 * j + 1][lr] = px[j].y;
      Ls[buf][lk + 2 * j][lr] = pl[j].x; Ls[buf][lk + 2 * j + 1][lr] = pl[j].y;
    }
    if (extra) { Ls[buf][ek][er] = pe.x; Ls[buf][ek + 1][er] = pe.y; }
  };
  fetch(klo);
  stage(0);
  __syncthreads();
  const int fr = lane & 15, fk = lane >> 4;
  const int njt = min(kNTw, (kNXi2 - q0 + 15) / 16);   // MFMA column tiles of this workgroup that hold table columns
  int cur = 0;
  for (int k0 = klo; k0 < khi; k0 += kGK, cur ^= 1) {
    const bool more = k0 + kGK < khi;
    if (more) fetch(k0 + kGK);
#pragma unroll
    for (int ks = 0; ks < kGK; ks += 4) {
      double a[2], c[kNTw];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = Xs[cur][ks + fk][wm * 32 + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < kNTw; ++j) c[j] = Ls[cur][ks + fk][j * 16 + fr];
#pragma unroll
      for (int j = 0; j < kNTw; ++j)
        if (j < njt) {   // (workgroup-uniform: the last column tile of the table holds 56 of its 144 columns)
#pragma unroll
          for (int i = 0; i < 2; ++i) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], c[j], acc[i][j], 0, 0, 0);
        }
    }
    if (more) stage(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int bb = b0 + (wm * 2 + i) * LPT + fk;
    if (bb >= B) continue;
    const double c0 = cst[2 * bb], c1 = cst[2 * bb + 1];
#pragma unroll
    for (int j = 0; j < kNTw; ++j) {
      const int q = q0 + j * 16 + fr;
      if (q < kNXi2) {
        const double x2 = xi2[q];
        W[(size_t)bb * kNXi2 + q] = c0 + acc[i][j][0] + x2 * acc[i][j][1];
        Wm[(size_t)bb * kNXi2 + q] = c1 + acc[i][j][2] + x2 * acc[i][j][3];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Gradient w.r.t. the distribution function itself (fe_mode PER_LINEOUT, SURVEY 8f-1 "free-form f_e").
// k_spectrum<.., GM = 2> leaves per lineout the adjoints of its tables: Wb[1640] (Re chi_e table) and Hy/Hs[nvx]
// (ln fe node values / slopes).  The W table is W = c0 + Lg (A + xi2 s), so its adjoint is the transposed GEMM
//   Y[b][0][i] = sum_q Wb[b][q] Lg[q][i]            (adjoint of A)
//   Y[b][1][i] = sum_q xi2[q] Wb[b][q] Lg[q][i]     (adjoint of s)
// done by k_wgemm_t on the FP64 matrix cores (M = 2B vectors, N = 1024, K = 1640), and k_fe_adjoint walks
// k_fe_vectors backwards (X construction, central differences, exp, Hermite evaluation at xi1, node slopes, ln).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads, 2) void k_wgemm_t(const double* __restrict__ Lg, const double* __restrict__ Wb,
                                                         const double* __restrict__ xi2, int B, double* __restrict__ Y) {
  __shared__ double Vs[kGK][kGP];   // [k][vector]
  __shared__ double Ls[kGK][kGP];   // [k][i]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int v0 = blockIdx.y * kGM, i0 = blockIdx.x * kGN;
  // staging of V: thread -> vector row lr, 8 consecutive q starting at lk; of Lg: row (q) sk, 8 consecutive i at sn
  const int lr = tid >> 1, lk = (tid & 1) * 8;
  const int vb = (v0 + lr) >> 1, vc = (v0 + lr) & 1;
  const double* __restrict__ vrow = Wb + (size_t)min(vb, B - 1) * kNXi2 + lk;
  const int sk = tid >> 4, sn = (tid & 15) * 8;
  const double* __restrict__ lrow = Lg + (size_t)sk * kNXi1 + i0 + sn;
  mfma_d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (mfma_d4){0.0, 0.0, 0.0, 0.0};
  const int fr = lane & 15, fk = lane >> 4;
  for (int k0 = 0; k0 < kNXi2; k0 += kGK) {
    double pv[8];
    double2 pl[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = k0 + lk + j;
      const double w = q < kNXi2 ? vrow[k0 + j] : 0.0;
      pv[j] = vc ? w * (q < kNXi2 ? xi2[q] : 0.0) : w;
    }
    const bool lok = k0 + sk < kNXi2;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      pl[j] = lok ? *reinterpret_cast<const double2*>(lrow + (size_t)k0 * kNXi1 + 2 * j) : make_double2(0.0, 0.0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) Vs[lk + j][lr] = pv[j];
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<double2*>(&Ls[sk][sn + 2 * j]) = pl[j];
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kGK; ks += 4) {
      double a[4], c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = Vs[ks + fk][wm * 64 + i * 16 + fr];
        c[i] = Ls[ks + fk][wn * 64 + i * 16 + fr];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], c[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D layout: col = lane & 15 (i), row = (lane >> 4) + 4 reg (vector inside the 16-row tile)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int v = v0 + wm * 64 + i * 16 + fk + 4 * r;
      if (v >= 2 * B) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) Y[(size_t)v * kNXi1 + i0 + wn * 64 + j * 16 + fr] = acc[i][j][r];
    }
}

// k_fe_adjoint: grid B, 256 threads.  In: ht [B][nvx] (ln fe, slope) of the forward pass, Y [B][2][1024], Wb [B][1640]
// (for the adjoint of c0 = sum_q Wb), Hy/Hs [B][nvx] from k_spectrum.  Out: dfe [B][nvx] = d loss / d f_e.
__global__ __launch_bounds__(kThreads) void k_fe_adjoint(KStatic S, const double2* __restrict__ ht_in,
                                                         const double* __restrict__ Y, const double* __restrict__ Wb,
                                                         const double* __restrict__ Hy_in, const double* __restrict__ Hs_in,
                                                         double* __restrict__ dfe) {
  extern __shared__ __align__(16) unsigned char smem[];
  double2* ht = reinterpret_cast<double2*>(smem);   // [nvx]
  double2* hc = ht + S.nvx;                         // [2 nvx]
  double* rat = reinterpret_cast<double*>(hc + 2 * S.nvx);  // [1024]
  double* fdb = rat + kNXi1;                        // [1024] adjoint of fdif, later of rat
  double* fab = fdb + kNXi1;                        // [1024] adjoint of fav
  double* rdb = fab + kNXi1;                        // [1024] adjoint of ratdf
  double* yb = rdb + kNXi1;                         // [nvx]
  double* sb = yb + S.nvx;                          // [nvx]
  double* red = sb + S.nvx;                         // [8]
  const int b = blockIdx.x, tid = threadIdx.x, nvx = S.nvx;
  for (int i = tid; i < nvx; i += kThreads) {
    ht[i] = ht_in[(size_t)b * nvx + i];
    yb[i] = Hy_in[(size_t)b * nvx + i];
    sb[i] = Hs_in[(size_t)b * nvx + i];
  }
  double part = 0.0;
  for (int q = tid; q < kNXi2; q += kThreads) part += Wb[(size_t)b * kNXi2 + q];
  const double c0b = block_sum(part, red);  // (contains the barrier that publishes ht)
  for (int i = tid; i < nvx - 1; i += kThreads) hermite_coeffs(ht[i], ht[i + 1], S.dv, hc[2 * i], hc[2 * i + 1]);
  __syncthreads();
  Tables T = make_tables(S, nullptr, nullptr, ht, hc);
  T.Hy = yb; T.Hs = sb;
  const double* Ab = Y + (size_t)b * 2 * kNXi1;
  const double* Sb = Ab + kNXi1;
  for (int i = tid; i < kNXi1; i += kThreads) {
    double H, dH;
    hermite_lookup_c(T, S.xi1[i], H, dH);
    rat[i] = exp(H);
    // X construction (ratdf_rows): Bs = fd ih, A = fa - mid Bs, c0 += fd   for i < 1022
    double fd = 0.0, fa = 0.0;
    if (i < kNXi1 - 2) {
      double ih, mid;
      xi1_cell(S.xi1, i, ih, mid);
      fa = Ab[i];
      fd = (Sb[i] - mid * fa) * ih + c0b;
    }
    fdb[i] = fd;
    fab[i] = fa;
  }
  __syncthreads();
  // fd_i = rdf[i+1] - rdf[i], fa_i = (rdf[i+1] + rdf[i]) / 2
  for (int j = tid; j < kNXi1; j += kThreads) {
    double v = 0.0;
    if (j < kNXi1 - 2) v += -fdb[j] + 0.5 * fab[j];
    if (j >= 1 && j <= kNXi1 - 2) v += fdb[j - 1] + 0.5 * fab[j - 1];
    rdb[j] = v;
  }
  __syncthreads();
  // rdf = gradient(rat, h1): central inside, one-sided at the ends
  const double ih1 = 1.0 / (S.xi1[1] - S.xi1[0]);
  const int n = kNXi1;
  for (int j = tid; j < n; j += kThreads) {
    double v = 0.0;
    if (j + 1 >= 1 && j + 1 <= n - 2) v -= 0.5 * ih1 * rdb[j + 1];
    if (j - 1 >= 1 && j - 1 <= n - 2) v += 0.5 * ih1 * rdb[j - 1];
    if (j == 1) v += ih1 * rdb[0];
    if (j == 0) v -= ih1 * rdb[0];
    if (j == n - 1) v += ih1 * rdb[n - 1];
    if (j == n - 2) v -= ih1 * rdb[n - 1];
    fdb[j] = v * rat[j];  // adjoint of H(xi1_j)  (rat = exp H)
  }
  __syncthreads();
  {  // scatter to the nodes: each thread walks consecutive xi1 points, so the run-length accumulators rarely flush
    FeAcc fa;
    fe_acc_init(fa);
    const int per = (kNXi1 + kThreads - 1) / kThreads;
    for (int j = tid * per; j < min((tid + 1) * per, kNXi1); ++j) fe_add_h(fa, T, S.xi1[j], fdb[j]);
    fe_flush_h(fa, yb, sb);
  }
  __syncthreads();
  // node slopes: mean of the adjacent secants, one-sided at the ends (k_fe_vectors)
  for (int j = tid; j < nvx; j += kThreads) {
    double v = yb[j];
    const double idv = 1.0 / S.dv;
    if (j >= 1) v += sb[j - 1] * (j - 1 == 0 ? idv : 0.5 * idv);        // s_{j-1} reads y_j with +
    if (j + 1 <= nvx - 1) v -= sb[j + 1] * (j + 1 == nvx - 1 ? idv : 0.5 * idv);  // s_{j+1} reads y_j with -
    if (j == 0) v -= sb[0] * idv;
    if (j == nvx - 1) v += sb[nvx - 1] * idv;
    dfe[(size_t)b * nvx + j] = v * exp(-ht[j].x);  // y = ln fe
  }
}
