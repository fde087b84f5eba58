// k_form_factor_2d.inc -- 2-D distribution functions: rotate-and-project sampler, its adjoint and the table adjoint.
// Part of the single translation unit tsff_kernels.hip (included inside namespace tsff).

// ------------------------------------------------------------------------------------------
// k_form_factor_2d: FormFactor.calc_in_2D (form_factor.py:449-587) for a 2-D distribution function
// fe2d[nv][nv] (first index = v_x): one workgroup per (lineout, gradient point, wavelength, angle).
//   1. point scalars: vector k = k_s - k_L, omega_d, xi_i, chi_i, vector xi_e -> (|xi_e|, beta)   (:515-558)
//   2. rotate(fe2d, beta) + column sum (:300-324, 371): thread iy evaluates the bicubic interpolant along the
//      rotated line {R_beta (vx[ix], vx[iy])}, ix = 0..nv-1.  interpax's "cubic" 2-D interpolant (bicubic Hermite
//      patch, derivative estimates = mean of adjacent secants, one-sided at the edges, extrap=True) is the tensor
//      product of the 1-D Hermite interpolants, i.e. a 4 x 4 stencil with separable weights (Catmull-Rom in the
//      interior, modified in the first/last cell).
//   3. gradient of the projection, the two linear interpolations at |xi_e| and the rationally-centred integral
//      over the nv-2 intervals (:372-387), spectrum assembly (:560-585).
// k_form_factor_2d_adj repeats all of that before it reverses it.  What the two kernels have in common is defined once, below:
//   sizes and slots   parts2d, nvp2d, group2d_doubles / group2d_adj_doubles, smem2d_doubles / smem2d_adj_doubles (the host sizes the
//                     dynamic LDS from the same functions), the SC_* slots of the per-group scalar scratch sc[]
//   shared steps      stage_table_2d, point_id_2d / point_setup_2d, project_point_2d, column_sums_2d, gradient_2d,
//                     assemble_point_2d; catmull_rom_d for the samplers that are not hand-scheduled
// Each kernel keeps its own point loop and barrier sequence, and its own form of the ratintn interval (see the shared steps).
// ------------------------------------------------------------------------------------------
// interior-cell (Catmull-Rom) weights of the four nodes c-1..c+2
__device__ __forceinline__ void catmull_rom(double t, double w[4]) {
  // w0 = -t^3/2 + t^2 - t/2, w1 = 3t^3/2 - 5t^2/2 + 1, w2 = -3t^3/2 + 2t^2 + t/2, w3 = t^3/2 - t^2/2: eleven instructions
  // (round 2: thirteen, through the Hermite basis functions h10, h11)
#pragma clang fp contract(off)   // (the same roundings wherever this is inlined: point ranges and sampler variants agree bit for bit)
  const double a = t * t, b = a * t, ht = 0.5 * t, ha = 0.5 * a;
  w[0] = __builtin_fma(-0.5, b, a - ht);
  w[1] = __builtin_fma(1.5, b, __builtin_fma(-2.5, a, 1.0));
  w[2] = __builtin_fma(-1.5, b, __builtin_fma(2.0, a, ht));
  w[3] = __builtin_fma(0.5, b, -ha);
}
// their derivatives in t, for the samplers that are not hand-scheduled (project_rolling keeps a Horner form of its own, with pinned
// roundings, next to its window arithmetic)
__device__ __forceinline__ void catmull_rom_d(double t, double d[4]) {
  d[0] = -0.5 * (3.0 * t * t - 4.0 * t + 1.0); d[1] = 4.5 * t * t - 5.0 * t;
  d[2] = -4.5 * t * t + 4.0 * t + 0.5;         d[3] = 1.5 * t * t - t;
}

// One bicubic sample at (xq, yq) of a table that carries one GHOST row / column on every side, filled by linear
// extrapolation (f[-1] = 2 f[0] - f[1], f[n] = 2 f[n-1] - f[n-2]; corners by both).  With those ghosts the Catmull-Rom
// weights of an interior cell reproduce interpax's edge cells exactly -- its one-sided node slope f[1] - f[0] IS the
// central slope (f[1] - f[-1]) / 2 of the extended sequence -- and its extrapolation (edge-cell polynomial continued
// outside the grid, extrap=True) is the same formula with the cell index clamped and t left free.  Every sample then
// takes one straight-line path: 4 x 4 consecutive entries, no index clamps, no divergence between lanes.
// Fp points at the ghost corner; pitch = row pitch in doubles of the padded table.
// (u, v): the sample position in CELL units, u = (xq - vx[0]) / dv.  Along a rotated line the callers advance it as
// u = u0 + ix cos(beta), v = v0 + ix sin(beta) -- one FMA per axis instead of rotating, shifting and scaling every sample.
__device__ __forceinline__ void cell_of(double u, int nv, int& c, double& t) {
  // (clamped as a double and converted once: floor, max, min, subtract, convert -- the integer form converted to int, clamped with
  //  two compares and selects and converted back for the subtraction; the same c and t)
  const double cd = fmin(fmax(floor(u), 0.0), (double)(nv - 2));
  c = (int)cd;
  t = u - cd;   // free outside the grid: the edge-cell polynomial continued (extrap=True)
}
__device__ __forceinline__ double bicubic_sample(const double* __restrict__ Fp, int nv, int pitch, double u, double v) {
  int cx, cy;
  double tx, ty, wx[4], wy[4];
  cell_of(u, nv, cx, tx);
  cell_of(v, nv, cy, ty);
  catmull_rom(tx, wx);
  catmull_rom(ty, wy);
  const double* __restrict__ q0 = Fp + (size_t)cx * pitch + cy;  // padded index of node (cx - 1, cy - 1)
  double r = 0.0;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const double* __restrict__ row = q0 + (size_t)m * pitch;
    r += wx[m] * (wy[0] * row[0] + wy[1] * row[1] + wy[2] * row[2] + wy[3] * row[3]);
  }
  return r;
}
// the same for a table in LDS with ONE ds_read_b64 per stencil entry: the compiler pairs neighbouring entries into
// ds_read2_b64, which moves 128 B per clock and CU where ds_read_b64 moves 256 (MI355X_MICROARCH.md, LDS table: 8 cycles
// per wavefront instruction against 2) -- and the sampler is bound by the LDS pipe (17.3 -> 12.7 ms at the ARTS size).
// volatile on an explicit LDS (address space 3) pointer keeps the reads apart.
typedef const volatile double __attribute__((address_space(3))) lds_cvdouble;
__device__ __forceinline__ double bicubic_sample_lds(const double* Fp, int nv, int pitch, double u, double v) {
  int cx, cy;
  double tx, ty, wx[4], wy[4];
  cell_of(u, nv, cx, tx);
  cell_of(v, nv, cy, ty);
  catmull_rom(tx, wx);
  catmull_rom(ty, wy);
  lds_cvdouble* q0 = (lds_cvdouble*)Fp + (cx * pitch + cy);
  double V[16];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    lds_cvdouble* row = q0 + m * pitch;
    V[4 * m] = row[0]; V[4 * m + 1] = row[1]; V[4 * m + 2] = row[2]; V[4 * m + 3] = row[3];
  }
  double r = 0.0;
#pragma unroll
  for (int m = 0; m < 4; ++m) r += wx[m] * (wy[0] * V[4 * m] + wy[1] * V[4 * m + 1] + wy[2] * V[4 * m + 2] + wy[3] * V[4 * m + 3]);
  return r;
}
// Rolling 4 x 4 window of table VALUES along a rotated line (tables read through L1/L2).  From one sample to the next the
// cell index moves by at most one on each axis (|cos|, |sin| <= 1; the clamp of cell_of is monotone), so the next stencil shares
// 9 to 16 of its entries with the current one: per step only the row and the column that may enter are requested (8 loads
// where the plain sampler issues 16 -- the sampler at 256^2 sat at 0.59 of the vector-L1 read rate; a sampler that requested all
// 16 entries of the next sample ahead of the contraction took 190 ms at 256^2, DESIGN.md section 4.3) and the window is shifted in
// place.  SX / SY = direction of the cell walk on each axis, the same for every sample of a point (wavefront-uniform), ix always
// ascending: the sum is taken in the same order, over the same values and weights, as the plain sampler takes it -- bit-identical
// results.  Entering column first (rows of the CURRENT window), then the entering row at the columns of the NEXT window: no
// corner case.
// TR: F is the TRANSPOSED padded table (entry (cx, cy) at F[cy * pitch + cx]).  The lanes of a wavefront are neighbouring lines,
// (-sin, cos) apart in cell units: where |sin| > |cos| they spread along the FIRST table axis, 64 lanes touch 64 different rows
// of the table and the 8 wavefronts of a CU overrun its 32 KB L1; read from the transposed copy they lie along its contiguous
// axis again.  The window stays W[m][n] = table(cx + m, cy + n) and the contraction is unchanged: same bits either way.
// VG: also the sums over the samples of d sample / d cos(beta), d sample / d sin(beta) (ds1, ds2: the record of a SAVE pass and the
// adjoint's projection pass), from the same window, in the arithmetic of bicubic_sample_vg.
//
// Round 3: the walk is INCREMENTAL.  The sampler was bound by its instruction issue (87 % VALU busy at 113 VALU instructions per
// sample, of which 52 are the arithmetic of the sample); per sample it recomputed the cell of the next position from scratch
// (floor, two clamps, convert), rebuilt six 64-bit load addresses from the cell indices (multiply, clamps of the entering row /
// column, shifts and adds) and renamed (t, cx, cy) with moves.  Now a lane carries the cell index as a double, the fractions and
// ONE byte offset of its window; "the cell moves by at most one per axis and step, in a direction that is the same for the whole
// point" turns cell_of into a subtraction and two comparisons (the clamp at the table's edges is the second one), and everything
// that changes with a shift -- the 16 window moves, cd, t and the offset -- changes inside the one exec-masked block.  The loads
// take a wavefront-uniform base (SGPR pair: table + row / column of the entering line) plus the lane's 32-bit byte offset; the
// entering line one step outside the table (never selected: the cell index stops at the edge) is read from the margin k_pad2d
// leaves around the padded pair instead of being clamped.  The fractions are the same doubles as cell_of's (u - c is exact for
// an integer c <= 254 next to u, and so is the +-1 of a shift), so the samples are the same bits.
//
// The entering COLUMN is requested by the lanes that will shift along that axis only (exec = my; it is the minor axis of the walk:
// |step| <= 0.71 cells, on average 0.37 of the lanes).  Its four entries lie a table row apart (in the orientation the point
// reads), so every request touches as many cache lines as the wavefront's lanes span rows -- the four of them cost 25 ms of a
// 124 ms image against 9 ms for the two contiguous row requests (profiles/r03m_ab_cfg4_exp.txt) -- and a lane that does not shift
// never looks at what it would have fetched.  The requests are written out (the compiler cannot put a load under a scalar mask it
// did not make itself); the values are consumed by window_shift_w only, behind its s_waitcnt.
// The shifts are 64-bit moves under the lanes' own condition (16 v_mov_b64 per axis where selects take 32 v_cndmask_b32; written
// out because the compiler turns the conditional form into copies of the whole window and sinks the requests behind a wait).
//
// The requests run TWO DEEP.
// With the instruction count down the sampler stopped being issue-bound: 30 % of the wavefront cycles were spent at the wait in
// front of the shifts (SQ_WAIT_INST_ANY), because the entering line is requested at the top of the iteration that consumes it and
// two wavefronts per SIMD cannot cover an L2 round trip (more wavefronts overrun the 32 KB L1: 3 per SIMD 130 ms, 4: 137 ms).
// Here the requests run ONE SAMPLE AHEAD of the window: an address cursor (cell index, byte offset, fractions: the same exec-masked
// updates as before, without the window) steps to sample k + 2 and requests the lines of the transition k + 1 -> k + 2 while the
// window is still at sample k; the shift k -> k + 1 at the end of the iteration consumes what the PREVIOUS iteration requested.
// Two sets of request registers, masks and fractions alternate (the loop is unrolled by two: renamed, not moved).  Every request
// is written out (global_load with an SGPR base, under the exec mask of the lanes that will shift on that axis), so the compiler
// counts none of them; the first shift of an iteration waits for vmcnt(6): the six requests just issued may stay in flight.
typedef double dbl2_t __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) char* gptr2d_t;
// four entries 8 bytes apart from one base, in the lanes of m
__device__ __forceinline__ void request4_contig(unsigned long long m, unsigned off, gptr2d_t b0, double (&o)[4]) {
  unsigned long long sv;
  dbl2_t c01, c23;
  asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t"
               "global_load_dwordx4 %[c01], %[off], %[b0]\n\t"
               "global_load_dwordx4 %[c23], %[off], %[b0] offset:16\n\t"
               "s_mov_b64 exec, %[sv]"
               : [sv] "=&s"(sv), [c01] "=&v"(c01), [c23] "=&v"(c23)
               : [m] "s"(m), [off] "v"(off), [b0] "s"(b0)
               : "scc", "memory");
  o[0] = c01[0]; o[1] = c01[1]; o[2] = c23[0]; o[3] = c23[1];
}
// four entries from four bases (a table row apart), in the lanes of m
__device__ __forceinline__ void request4_strided(unsigned long long m, unsigned off, gptr2d_t b0, gptr2d_t b1, gptr2d_t b2, gptr2d_t b3,
                                                 double (&o)[4]) {
  unsigned long long sv;
  asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\t"
               "global_load_dwordx2 %[n0], %[off], %[b0]\n\t"
               "global_load_dwordx2 %[n1], %[off], %[b1]\n\t"
               "global_load_dwordx2 %[n2], %[off], %[b2]\n\t"
               "global_load_dwordx2 %[n3], %[off], %[b3]\n\t"
               "s_mov_b64 exec, %[sv]"
               : [sv] "=&s"(sv), [n0] "=&v"(o[0]), [n1] "=&v"(o[1]), [n2] "=&v"(o[2]), [n3] "=&v"(o[3])
               : [m] "s"(m), [off] "v"(off), [b0] "s"(b0), [b1] "s"(b1), [b2] "s"(b2), [b3] "s"(b3)
               : "scc", "memory");
}
// the cursor one cell on in the lanes of m: cd += DIR, t -= DIR, off8 += d8
template <int DIR>
__device__ __forceinline__ void cursor_step(unsigned long long m, double& cd, double& t, unsigned& off8, int d8) {
  unsigned long long sv;
  if (DIR > 0)
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\tv_add_f64 %[cd], %[cd], 1.0\n\tv_add_f64 %[t], %[t], -1.0\n\tv_add_u32 %[off], %[d8], %[off]\n\ts_mov_b64 exec, %[sv]"
                 : [sv] "=&s"(sv), [cd] "+v"(cd), [t] "+v"(t), [off] "+v"(off8) : [m] "s"(m), [d8] "s"(d8) : "scc");
  else
    asm volatile("s_and_saveexec_b64 %[sv], %[m]\n\tv_add_f64 %[cd], %[cd], -1.0\n\tv_add_f64 %[t], %[t], 1.0\n\tv_add_u32 %[off], %[d8], %[off]\n\ts_mov_b64 exec, %[sv]"
                 : [sv] "=&s"(sv), [cd] "+v"(cd), [t] "+v"(t), [off] "+v"(off8) : [m] "s"(m), [d8] "s"(d8) : "scc");
}
// four chains a0 <- a1 <- a2 <- a3 <- n in the lanes of m; WAIT >= 0: first wait until at most WAIT requests are in flight
template <int WAIT>
__device__ __forceinline__ void window_shift_w(unsigned long long m, double& a0, double& a1, double& a2, double& a3, double an, double& b0,
                                               double& b1, double& b2, double& b3, double bn, double& c0, double& c1, double& c2, double& c3,
                                               double cn, double& d0, double& d1, double& d2, double& d3, double dn) {
  unsigned long long sv;
  asm volatile(
      "s_waitcnt vmcnt(%[w])\n\t"
      "s_and_saveexec_b64 %[sv], %[m]\n\t"
      "v_mov_b64 %[a0], %[a1]\n\tv_mov_b64 %[a1], %[a2]\n\tv_mov_b64 %[a2], %[a3]\n\tv_mov_b64 %[a3], %[an]\n\t"
      "v_mov_b64 %[b0], %[b1]\n\tv_mov_b64 %[b1], %[b2]\n\tv_mov_b64 %[b2], %[b3]\n\tv_mov_b64 %[b3], %[bn]\n\t"
      "v_mov_b64 %[c0], %[c1]\n\tv_mov_b64 %[c1], %[c2]\n\tv_mov_b64 %[c2], %[c3]\n\tv_mov_b64 %[c3], %[cn]\n\t"
      "v_mov_b64 %[d0], %[d1]\n\tv_mov_b64 %[d1], %[d2]\n\tv_mov_b64 %[d2], %[d3]\n\tv_mov_b64 %[d3], %[dn]\n\t"
      "s_mov_b64 exec, %[sv]"
      : [sv] "=&s"(sv), [a0] "+v"(a0), [a1] "+v"(a1), [a2] "+v"(a2), [a3] "+v"(a3), [b0] "+v"(b0), [b1] "+v"(b1), [b2] "+v"(b2),
        [b3] "+v"(b3), [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [d0] "+v"(d0), [d1] "+v"(d1), [d2] "+v"(d2),
        [d3] "+v"(d3)
      : [m] "s"(m), [an] "v"(an), [bn] "v"(bn), [cn] "v"(cn), [dn] "v"(dn), [w] "n"(WAIT)
      : "scc");
}
struct RollVG { double idv, dv, v0, y, ds1, ds2; };
template <int SX, int SY, bool TR, bool VG = false>
__device__ __forceinline__ double project_rolling(const double* __restrict__ F, int nv, int pitch, double cb, double sb,
                                                  double ul, double vl, int ix0, int ix1, RollVG* vg = nullptr) {
#pragma clang fp contract(off)
  double xi_d = (double)ix0, xs_d = xi_d, W[4][4], acc = 0.0, ds1 = 0.0, ds2 = 0.0, cdx, cdy, wx[4], wy[4], dx[4], dy[4];
  double t0x, t0y, t1x = 0.0, t1y = 0.0;
  unsigned off8;
  {
    int cx, cy;
    cell_of(__builtin_fma(xi_d, cb, ul), nv, cx, t0x);
    cell_of(__builtin_fma(xi_d, sb, vl), nv, cy, t0y);
    cdx = (double)cx; cdy = (double)cy;
    const unsigned o = (unsigned)(TR ? cy * pitch + cx : cx * pitch + cy);
    off8 = o * 8u;
    const double* __restrict__ q0 = F + o;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 4; ++n) W[m][n] = q0[(unsigned)(TR ? n * pitch + m : m * pitch + n)];
  }
  const int px8 = (TR ? 1 : pitch) * 8, py8 = (TR ? pitch : 1) * 8;
  auto sptr = [](const char* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<gptr2d_t>(((unsigned long long)hi << 32) | lo);
  };
  const char* Fc = reinterpret_cast<const char*>(F);
  gptr2d_t bc[4], br[4];   // entering column: rows cx + m of the window it enters; entering row: columns of the window AFTER the column shift
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    bc[m] = sptr(Fc + (SY > 0 ? 4 : -1) * py8 + m * px8);
    br[m] = sptr(Fc + (SX > 0 ? 4 : -1) * px8 + m * py8);
  }
  const unsigned dyv = (unsigned)(SY * py8);
  double cmax = (double)(nv - 2);
  auto weights = [&](double tx, double ty) {
    catmull_rom(tx, wx);
    catmull_rom(ty, wy);
    if (VG) {   // derivatives of the weights: -(3 t^2 - 4 t + 1) / 2, (9 t^2 - 10 t) / 2, (-9 t^2 + 8 t + 1) / 2, (3 t^2 - 2 t) / 2
      dx[0] = __builtin_fma(__builtin_fma(-1.5, tx, 2.0), tx, -0.5); dx[1] = __builtin_fma(4.5, tx, -5.0) * tx;
      dx[2] = __builtin_fma(__builtin_fma(-4.5, tx, 4.0), tx, 0.5);  dx[3] = __builtin_fma(1.5, tx, -1.0) * tx;
      dy[0] = __builtin_fma(__builtin_fma(-1.5, ty, 2.0), ty, -0.5); dy[1] = __builtin_fma(4.5, ty, -5.0) * ty;
      dy[2] = __builtin_fma(__builtin_fma(-4.5, ty, 4.0), ty, 0.5);  dy[3] = __builtin_fma(1.5, ty, -1.0) * ty;
    }
  };
  // the address cursor: from its cell (cdx, cdy, off8) to the next sample -- fractions against the current cell, shift masks, the
  // requests of that transition (column at the rows of the current window, row at the columns after the column shift), then the step
  auto cursor = [&](double& tx, double& ty, unsigned long long& mx, unsigned long long& my, double (&NC)[4], double (&NR)[4]) {
    xi_d += 1.0;
    tx = __builtin_fma(xi_d, cb, ul) - cdx;
    ty = __builtin_fma(xi_d, sb, vl) - cdy;
    unsigned long long ex, ey;
    if (SX > 0) { asm("v_cmp_le_f64 %0, 1.0, %1" : "=s"(mx) : "v"(tx)); asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(ex) : "v"(cdx), "v"(cmax)); }
    else { asm("v_cmp_gt_f64 %0, 0, %1" : "=s"(mx) : "v"(tx)); asm("v_cmp_lt_f64 %0, 0, %1" : "=s"(ex) : "v"(cdx)); }
    if (SY > 0) { asm("v_cmp_le_f64 %0, 1.0, %1" : "=s"(my) : "v"(ty)); asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(ey) : "v"(cdy), "v"(cmax)); }
    else { asm("v_cmp_gt_f64 %0, 0, %1" : "=s"(my) : "v"(ty)); asm("v_cmp_lt_f64 %0, 0, %1" : "=s"(ey) : "v"(cdy)); }
    mx &= ex; my &= ey;
    unsigned offr;
    asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(offr) : "v"(dyv), "s"(my));
    offr += off8;
    if (TR) request4_contig(my, off8, bc[0], NC);
    else request4_strided(my, off8, bc[0], bc[1], bc[2], bc[3], NC);
    if (TR) request4_strided(mx, offr, br[0], br[1], br[2], br[3], NR);
    else request4_contig(mx, offr, br[0], NR);
    cursor_step<SY>(my, cdy, ty, off8, SY * py8);
    cursor_step<SX>(mx, cdx, tx, off8, SX * px8);
  };
  auto dot4 = [](const double (&w)[4], const double (&v)[4]) {
    return __builtin_fma(w[3], v[3], __builtin_fma(w[2], v[2], __builtin_fma(w[1], v[1], w[0] * v[0])));
  };
  constexpr int kReqPerSample = 6;   // request instructions of one cursor step: what may stay in flight at a shift
  // one sample: cursor to sample k + 2 (requests of k + 1 -> k + 2 into the `n` set), sample k from the window, weights of sample
  // k + 1, shift k -> k + 1 with the `c` set (requested one iteration ago)
  auto body = [&](double& tcx, double& tcy, unsigned long long& mcx, unsigned long long& mcy, double (&NCc)[4], double (&NRc)[4],
                  double& tnx, double& tny, unsigned long long& mnx, unsigned long long& mny, double (&NCn)[4], double (&NRn)[4], double keep) {
    cursor(tnx, tny, mnx, mny, NCn, NRn);
    __builtin_amdgcn_sched_barrier(0);   // keep the requests ahead of the arithmetic on the current sample
    if (!VG) {
      double rr[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) rr[m] = dot4(wy, W[m]);
      acc = __builtin_fma(dot4(wx, rr), keep, acc);   // (keep = 1: the addition itself, bit for bit; 0: the sample past the end of an odd line)
    } else {
      double rr[4], rd[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) { rr[m] = dot4(wy, W[m]); rd[m] = dot4(dy, W[m]); }
      const double val = dot4(wx, rr), sx = dot4(dx, rr), sy = dot4(wx, rd);
      const double Sx = sx * vg->idv, Sy = sy * vg->idv, x = __builtin_fma(xs_d, vg->dv, vg->v0);
      acc = __builtin_fma(val, keep, acc);
      ds1 = __builtin_fma(__builtin_fma(Sy, vg->y, Sx * x), keep, ds1);
      ds2 = __builtin_fma(__builtin_fma(-Sx, vg->y, Sy * x), keep, ds2);
      xs_d += 1.0;
    }
    weights(tcx, tcy);   // (of the NEXT sample: its fractions were finished by the cursor one iteration ago)
    if (SY > 0) window_shift_w<kReqPerSample>(mcy, W[0][0], W[0][1], W[0][2], W[0][3], NCc[0], W[1][0], W[1][1], W[1][2], W[1][3], NCc[1],
                                  W[2][0], W[2][1], W[2][2], W[2][3], NCc[2], W[3][0], W[3][1], W[3][2], W[3][3], NCc[3]);
    else window_shift_w<kReqPerSample>(mcy, W[0][3], W[0][2], W[0][1], W[0][0], NCc[0], W[1][3], W[1][2], W[1][1], W[1][0], NCc[1],
                           W[2][3], W[2][2], W[2][1], W[2][0], NCc[2], W[3][3], W[3][2], W[3][1], W[3][0], NCc[3]);
    if (SX > 0) window_shift_w<kReqPerSample>(mcx, W[0][0], W[1][0], W[2][0], W[3][0], NRc[0], W[0][1], W[1][1], W[2][1], W[3][1], NRc[1],
                                  W[0][2], W[1][2], W[2][2], W[3][2], NRc[2], W[0][3], W[1][3], W[2][3], W[3][3], NRc[3]);
    else window_shift_w<kReqPerSample>(mcx, W[3][0], W[2][0], W[1][0], W[0][0], NRc[0], W[3][1], W[2][1], W[1][1], W[0][1], NRc[1],
                           W[3][2], W[2][2], W[1][2], W[0][2], NRc[2], W[3][3], W[2][3], W[1][3], W[0][3], NRc[3]);
  };
  double NC0[4], NR0[4], NC1[4], NR1[4];
  unsigned long long m0x, m0y, m1x = 0, m1y = 0;
  // (the first window is in before the loop, and the compiler is TOLD so: its own bookkeeping of the sixteen loads above would
  //  otherwise put waits for them in front of the window's first uses inside the loop -- down to vmcnt(0), every iteration, which
  //  drains the requests it knows nothing about.  vmcnt(0), expcnt and lgkmcnt left alone: 0x0f70)
  __builtin_amdgcn_s_waitcnt(0x0f70);
  weights(t0x, t0y);                       // sample 0
  cursor(t0x, t0y, m0x, m0y, NC0, NR0);    // -> fractions of sample 1, requests of 0 -> 1
  // The registers of a request set hold nothing until the data arrives, and the compiler does not know: it must never COPY them
  // between a request and the shift that waits for it.  Inside the loop the two sets are loop-carried values that the allocator keeps
  // in place (checked in the assembly, and by tests that fail within a few runs otherwise); a separate tail for an odd number of
  // samples was NOT safe -- the values leaving the loop went through copies in front of the tail's wait, and odd tables gave wrong
  // projections two runs out of three (scripts/nv_sweep_2d.py).  So there is no tail: an odd line takes one more sample, past its
  // end (a valid evaluation: the walk stays inside the padded table), with weight `keep` = 0.  And the first set is complete before
  // the loop is entered (once per line), so that copies in the preheader are harmless too.
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(NC0[0]), "+v"(NC0[1]), "+v"(NC0[2]), "+v"(NC0[3]), "+v"(NR0[0]), "+v"(NR0[1]), "+v"(NR0[2]), "+v"(NR0[3]));
  const int nstep = __builtin_amdgcn_readfirstlane(ix1 - ix0);   // (the part of the line is the same for the lanes of a wavefront)
  for (int it = 0; it < nstep; it += 2) {
    body(t0x, t0y, m0x, m0y, NC0, NR0, t1x, t1y, m1x, m1y, NC1, NR1, 1.0);
    body(t1x, t1y, m1x, m1y, NC1, NR1, t0x, t0y, m0x, m0y, NC0, NR0, it + 1 < nstep ? 1.0 : 0.0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the last requests -- beyond the end of the line, never used -- before their registers are reused)
  if (VG) { vg->ds1 = ds1; vg->ds2 = ds2; }
  return acc;
}
// the orientation of the table and of the cell walk: uniform over the point (see project_rolling); Fp = padded table followed
// by its transpose (k_pad2d)
template <bool VG>
__device__ __forceinline__ double project_rolling_any(const double* __restrict__ Fp, int nv, int pitch, double cb, double sb,
                                                      double ul, double vl, int ix0, int ix1, RollVG* vg = nullptr) {
  const double* __restrict__ Ft = Fp + (size_t)(nv + 2) * pitch;
  if (fabs(sb) > fabs(cb)) {
    if (cb >= 0.0) return sb >= 0.0 ? project_rolling<1, 1, true, VG>(Ft, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg) : project_rolling<1, -1, true, VG>(Ft, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg);
    return sb >= 0.0 ? project_rolling<-1, 1, true, VG>(Ft, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg) : project_rolling<-1, -1, true, VG>(Ft, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg);
  }
  if (cb >= 0.0) return sb >= 0.0 ? project_rolling<1, 1, false, VG>(Fp, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg) : project_rolling<1, -1, false, VG>(Fp, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg);
  return sb >= 0.0 ? project_rolling<-1, 1, false, VG>(Fp, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg) : project_rolling<-1, -1, false, VG>(Fp, nv, pitch, cb, sb, ul, vl, ix0, ix1, vg);
}
// cell coordinates of sample (ix, iy) of the grid rotated by (cb, sb): u = ix cb + u0, v = ix sb + v0
__device__ __forceinline__ void line_origin(double cb, double sb, double y, double vx0, double idv, double& u0, double& v0c) {
#pragma clang fp contract(off)   // (the same bits in every kernel that walks the line: forward, adjoint, table-adjoint scatter)
  u0 = (vx0 * cb - y * sb - vx0) * idv;
  v0c = (vx0 * sb + y * cb - vx0) * idv;
}

// ghost cells of a padded table P[(nv + 2)][pitch] whose interior [1..nv][1..nv] is filled: rows first, then columns
// (which also makes the corners).  Called by all threads of a workgroup (LDS) or of a grid (global copy).
__device__ __forceinline__ void ghost_rows(double* __restrict__ P, int nv, int pitch, int tid, int nthr) {
  for (int c = tid; c < nv; c += nthr) {
    P[c + 1] = 2.0 * P[pitch + c + 1] - P[2 * pitch + c + 1];
    P[(size_t)(nv + 1) * pitch + c + 1] = 2.0 * P[(size_t)nv * pitch + c + 1] - P[(size_t)(nv - 1) * pitch + c + 1];
  }
}
__device__ __forceinline__ void ghost_cols(double* __restrict__ P, int nv, int pitch, int tid, int nthr) {
  for (int r = tid; r < nv + 2; r += nthr) {
    double* row = P + (size_t)r * pitch;
    row[0] = 2.0 * row[1] - row[2];
    row[nv + 1] = 2.0 * row[nv] - row[nv - 1];
  }
}

// padded copy in global memory for tables that do not fit LDS, followed by its transpose (project_rolling): one workgroup per
// table, pad2d_doubles(nv) doubles each -- [margin | padded (nv + 2)^2 | its transpose | margin]; the consumers get a pointer to the
// padded table (P + pad2d_margin).  The margins (zero) are what project_rolling reads when the line that WOULD enter its window lies
// one row / column outside the padded table (never selected, so never clamped).
__host__ __device__ inline size_t pad2d_margin(int nv) { return (size_t)nv + 2 + 8; }
__host__ __device__ inline size_t pad2d_doubles(int nv) { return 2 * (size_t)(nv + 2) * (nv + 2) + 2 * pad2d_margin(nv); }
__global__ __launch_bounds__(kThreads) void k_pad2d(const double* __restrict__ F, int nv, double* __restrict__ P) {
  const int pitch = nv + 2, mg = (int)pad2d_margin(nv);
  const double* __restrict__ Fb = F + (size_t)blockIdx.x * nv * nv;
  double* __restrict__ Pb = P + (size_t)blockIdx.x * pad2d_doubles(nv) + mg;
  for (int i = threadIdx.x; i < mg; i += kThreads) { Pb[i - mg] = 0.0; Pb[2 * (size_t)pitch * pitch + i] = 0.0; }
  for (int i = threadIdx.x; i < nv * nv; i += kThreads) Pb[(size_t)(i / nv + 1) * pitch + (i % nv + 1)] = Fb[i];
  __syncthreads();
  ghost_rows(Pb, nv, pitch, threadIdx.x, kThreads);
  __syncthreads();
  ghost_cols(Pb, nv, pitch, threadIdx.x, kThreads);
  __syncthreads();
  double* __restrict__ Tb = Pb + (size_t)pitch * pitch;
  for (int i = threadIdx.x; i < pitch * pitch; i += kThreads) Tb[i] = Pb[(size_t)(i % pitch) * pitch + i / pitch];
}

// LDS: true -> the nv x nv table is staged once per (persistent) workgroup in LDS (nv <= 128: 128 KB); false -> the
// table is read through L1/L2 (any nv).  A workgroup is kG2 = 4 groups of 256 threads that work on four different
// points at once and share the table: 4 wavefronts per SIMD hide the latency of the 16 table reads per sample (one
// 256-thread workgroup per CU, all the 128 KB table allows, leaves one wavefront per SIMD waiting on LDS).  The
// per-point scalars are computed by one thread per group and passed through LDS so that the sampling loop stays
// within the 128 registers of a 1024-thread workgroup.  One table per launch (the host loops over lineouts when every
// lineout has its own).
#ifndef TSFF_2D_GROUPS_LDS
#define TSFF_2D_GROUPS_LDS 4
#endif
#ifndef TSFF_2D_GROUPS_L2
#define TSFF_2D_GROUPS_L2 1
#endif
// Row pitch of the padded (nv + 2)^2 table.  In LDS it is made odd: with an even (worse: power-of-two) pitch the rows
// start in the same banks and the lanes of a wavefront (neighbouring points of a rotated line) collide whenever the line
// runs along the first table axis.
__host__ __device__ inline int pitch2d(int nv, bool lds) {
  if (!lds) return nv + 2;
  // LDS bank model: the 32 lanes of a half wavefront read one double each; doubles a != b collide when a = b (mod 32).
  // The lanes are neighbouring samples of a rotated line, i.e. a digital straight line of cells, and with
  // bank = (pitch cx + cy) mod 32 the passes per read depend on pitch mod 32 (simulated over all directions / measured
  // by SQ_LDS_BANK_CONFLICT): 1 -> 1.49, 2 -> 1.78 / 1.8, 3 -> 1.97 / 1.96, growing to 2.4 at 10.  1 where the LDS
  // budget allows it (nv <= 96), else 2.
  const int r = nv <= 96 ? 1 : 2;
  return nv + 2 + ((r - (nv + 2) % 32) + 32) % 32;
}
// ---- sizes and scratch slots of the two point kernels (k_form_factor_2d, k_form_factor_2d_adj): defined HERE, read by both
// kernels and by the host (form_factor_2d_prepare, form_factor_2d_adj_prepare) ----
// thread -> (column iy = gt % nvp2d, part gt / nvp2d of the column's ix range): nvp2d = nv rounded up to 64, 128 or 256, parts2d =
// 256 / nvp2d; above 256 a thread owns several whole columns
__host__ __device__ inline int parts2d(int nv) { return nv <= 64 ? 4 : (nv <= 128 ? 2 : 1); }
__host__ __device__ inline int nvp2d(int nv) { return nv <= 64 ? 64 : (nv <= 128 ? 128 : 256); }
constexpr int kSc2 = 40;  // doubles of per-group scalar scratch, forward
constexpr int kScA = 96;  // the same of the adjoint: [0, SC_ACC) point scalars and adjoints, [SC_ACC, SC_ACC + NLB] running sums and their tag
// per-group scratch of the forward: f1, d1 [nv], part [parts2d][nv], red [8], sc [kSc2]
__host__ __device__ inline size_t group2d_doubles(int nv) { return (2 + (size_t)parts2d(nv)) * nv + 8 + kSc2; }
// ... of the adjoint: f1, d1 [nv], part [parts2d][nv], c0, c1 [nv], red [16], sc [kScA]
__host__ __device__ inline size_t group2d_adj_doubles(int nv) { return (2 + (size_t)parts2d(nv)) * nv + 2 * (size_t)nv + 16 + kScA; }
// dynamic LDS of a workgroup of ng point groups: the groups' scratch, then the padded table (LDS variant)
__host__ __device__ inline size_t table2d_doubles(int nv, bool lds) { return lds ? (size_t)(nv + 2) * pitch2d(nv, true) : 0; }
__host__ __device__ inline size_t smem2d_doubles(int nv, bool lds, int ng) { return (size_t)ng * group2d_doubles(nv) + table2d_doubles(nv, lds); }
__host__ __device__ inline size_t smem2d_adj_doubles(int nv, bool lds, int ng) { return (size_t)ng * group2d_adj_doubles(nv) + table2d_doubles(nv, lds); }
// Slots of sc[]: what thread 0 of a point group leaves for the group, and for itself later in the point.
constexpr int kNLB2 = 8;  // lineout-scalar adjoints: wpe2, wL, kL, ivTe, a_e, pref, Ud, Vd, + 3 per ion: ixi, a_i, cs
enum {
  SC_CB = 0, SC_SB, SC_XMAG, SC_K2, SC_K, SC_WD, SC_WS, SC_AE, SC_IVTE, SC_WL, SC_PREF,         // point scalars (point_setup_2d), both kernels
  SC_KX, SC_KY, SC_AA, SC_XEX, SC_XEY, SC_KS, SC_VX, SC_VY, SC_UX, SC_UY, SC_CT, SC_ST, SC_BG,      // ... adjoint only; SC_BG = b G + g
  SC_ION = 24,                                                                                  // [3 s + 0, 1, 2] = ixi, a_i, cs of species s, both kernels
  SC_RB = 36, SC_FEVB, SC_DFEB, SC_IL, SC_T, SC_XMAGB, SC_WDB, SC_WLB,                          // the adjoint's reverse of the assembly
  SC_IONB = 44,                                                                                 // [3 s + 0, 1, 2] = adjoints of ixi, a_i, cs
  SC_PREFB = 56, SC_IVTEB, SC_AEB, SC_K2B,
  SC_ACC = 64                                                                                   // [NLB] running sums per (b, g); [NLB]: the (b, g) they belong to
};
static_assert(SC_BG < SC_ION && SC_ION + 3 * TSFF_MAX_ION <= SC_RB && SC_IONB + 3 * TSFF_MAX_ION <= SC_PREFB && SC_K2B < SC_ACC, "sc[] slots overlap");
// value and both first derivatives from ONE read of the stencil (the adjoint's projection pass carries the derivative
// sums along: they do not depend on the seed, so the separate derivative sweep -- a second full round of LDS reads, the
// resource this kernel is bound by -- is not needed)
template <bool LDSV = false>
__device__ __forceinline__ double bicubic_sample_vg(const double* __restrict__ Fp, int nv, int pitch, double idv, double u,
                                                    double v, double& Sx, double& Sy) {
  int cx, cy;
  double tx, ty;
  cell_of(u, nv, cx, tx);
  cell_of(v, nv, cy, ty);
  double wx[4], wy[4], dx[4], dy[4];
  catmull_rom(tx, wx);
  catmull_rom(ty, wy);
  catmull_rom_d(tx, dx);
  catmull_rom_d(ty, dy);
  const double* __restrict__ q0 = Fp + (size_t)cx * pitch + cy;
  double val = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const double* __restrict__ row = q0 + (size_t)m * pitch;
    double r0, r1, r2, r3;
    if (LDSV) {   // (one ds_read_b64 per entry, see bicubic_sample_lds)
      lds_cvdouble* rl = (lds_cvdouble*)Fp + ((cx + m) * pitch + cy);
      r0 = rl[0]; r1 = rl[1]; r2 = rl[2]; r3 = rl[3];
    } else {
      r0 = row[0]; r1 = row[1]; r2 = row[2]; r3 = row[3];
    }
    const double r = wy[0] * r0 + wy[1] * r1 + wy[2] * r2 + wy[3] * r3;
    const double rd = dy[0] * r0 + dy[1] * r1 + dy[2] * r2 + dy[3] * r3;
    val += wx[m] * r;
    sx += dx[m] * r;
    sy += wx[m] * rd;
  }
  Sx = sx * idv;
  Sy = sy * idv;
  return val;
}

// doubles per point of the projection record a SAVE pass leaves for the adjoint: f1[nv], then the per-thread partial
// derivative sums ds1[nparts][nv], ds2[nparts][nv] (nv <= 256 only)
__host__ __device__ inline size_t proj2d_doubles(int nv) { return (size_t)nv * (1 + 2 * parts2d(nv)); }
template <class T>
__device__ __forceinline__ T* proj2d_record(T* proj, long point, int nv) { return proj + (size_t)point * proj2d_doubles(nv); }
// SAVE: the fit loop will reverse this very evaluation next (tsff_form_factor_2d_grad with use_saved): the projection f1
// and the derivative sums of every point go to `proj` (proj2d_doubles per point), so that the adjoint does no sampling.
#ifndef TSFF_2D_WAVES
#define TSFF_2D_WAVES 2   // wavefronts per SIMD the register allocation leaves room for (measured at 256^2 with the rolling window: 2 -> 147 ms, 3 -> 182, 4 -> 200: more wavefronts overrun the L1)
#endif
// Point scalars of the 2-D path (form_factor.py:515-558): vector k = k_s - k_L, omega_d, vector xi_e -> (|xi_e|, cos / sin of its
// direction beta).  ONE function with pinned roundings for the forward and the adjoint kernels: the rotated sample positions -- and
// with them the projection f1 -- are then the same bits in both, so that the adjoint that samples for itself and the one that reads the
// forward's projection records differ by the order of the table adjoint's LDS atomics only (1e-15; with cos(atan(y / x)) in one
// kernel and x / |xi_e| in the other they differed by 5e-13 ... 5e-11 of the largest table-adjoint entry, depending on the rounding of
// the sample weights: the entries next to the table's edge are sums of extrapolation weights ~ t^3 that cancel to 1e-6).
struct Point2D { double ks, ct, st, kx, ky, k2, k, Vx, Vy, Ux, Uy, wd, aa, xex, xey, xmag, cb, sb; };
template <int NI>
__device__ __forceinline__ void point_scalars_2d(double ws, double th, const LineS<NI>& L, double va_ang, double ud_ang, Point2D& q) {
#pragma clang fp contract(off)
  q.ks = ks_eval(ws, L.wpe2);
  q.ct = cos(th); q.st = sin(th);
  q.kx = q.ct * q.ks - L.kL; q.ky = q.st * q.ks;
  q.k2 = q.kx * q.kx + q.ky * q.ky; q.k = sqrt(q.k2);
  q.Vx = L.Vd * cos(va_ang); q.Vy = L.Vd * sin(va_ang);
  q.Ux = L.Ud * cos(ud_ang); q.Uy = L.Ud * sin(ud_ang);
  q.wd = (ws - L.wL) - (q.kx * q.Vx + q.ky * q.Vy);
  q.aa = q.wd / q.k2;
  q.xex = (q.aa * q.kx - q.Ux) * L.ivTe; q.xey = (q.aa * q.ky - q.Uy) * L.ivTe;
  q.xmag = sqrt(q.xex * q.xex + q.xey * q.xey);
  const double beta = atan(q.xey / q.xex) + (q.xex >= 0.0 ? 0.0 : kPi);   // heaviside(x, 1) = 1 at x == 0  (:552-558)
  q.cb = cos(beta); q.sb = sin(beta);
}
// ------------------------------------------------------------------------------------------
// The steps k_form_factor_2d and its adjoint share, each defined once.  The adjoint repeats the forward up to the point's spectrum,
// and "the same projection, bit for bit" between the saving forward and the adjoint that reads its records rests on both running
// the same text.  Each kernel keeps its point loop and its barrier sequence written out and calls these between the barriers
// (k_pairs.inc: share the steps, not the loop).
//   a. stage_table_2d     the table into LDS, ghost rows and columns
//   b. point_id_2d, point_setup_2d   pid -> (a, j, g, b); thread 0's point scalars into sc[]
//   c. project_point_2d   one point's partial column sums into part[] (plain, with derivative sums, several columns per thread)
//   d. column_sums_2d, gradient_2d   f1 from part, d1 from f1
//   e. assemble_point_2d  thread 0: the interpolations at |xi_e|, chi_e, the ion terms, epsilon, S(k, omega)
// NOT shared: the ratintn interval between d. and e.  The forward takes the small-interval branch as fav / gav + tmp gdif / (12 gav^3),
// the adjoint as fav ig + tmp c with ig = 1 / gav, c = gdif / (12 gav^3), which it needs for the partial derivatives: the same value
// with other roundings, so one definition would change the bits of one of the kernels.
// ------------------------------------------------------------------------------------------
// a. the plain nv x nv table Fg into the padded table Fl in LDS, the ghost cells made here: all nthr threads of the workgroup
__device__ __forceinline__ void stage_table_2d(const double* __restrict__ Fg, double* Fl, int nv, int pitch, int nthr) {
  for (int i = threadIdx.x; i < nv * nv; i += nthr) Fl[(i / nv + 1) * pitch + (i % nv + 1)] = Fg[i];
  __syncthreads();
  ghost_rows(Fl, nv, pitch, threadIdx.x, nthr);
  __syncthreads();
  ghost_cols(Fl, nv, pitch, threadIdx.x, nthr);
}
// b. point of the flat list -> scattering angle a, wavelength j, gradient point g, lineout b
struct PointId2D { int a, j, g, b; };
__device__ __forceinline__ PointId2D point_id_2d(long pid, const KStatic& S) {
  const int NA = S.n_angles, G = S.G, npts = S.npts;
  PointId2D id;
  id.a = (int)(pid % NA); id.j = (int)((pid / NA) % npts); id.g = (int)((pid / ((long)NA * npts)) % G);
  id.b = (int)(pid / ((long)NA * npts * G));
  return id;
}
// ... and its scalars into sc[] (one thread per point group); ADJ: also what the reverse of point_scalars_2d reads
template <int NI, bool ADJ>
__device__ __forceinline__ void point_setup_2d(const KStatic& S, const double* __restrict__ phys, int f, const PointId2D& id, double ud_ang,
                                               double va_ang, double* sc) {
  Phys<NI> p;
  load_phys<NI>(phys + (size_t)id.b * S.NP, S.p_scale, S.p_shift, S.p_sig, S.ti_same, false, p);
  LineS<NI> L;
  make_lines<NI>(p, S.lam_shift[f], id.g, S.G, L);
  // ---- point scalars (form_factor.py:515-558) ----
  const double ws = S.omgs[f][id.j], th = S.sa_rad[id.a];
  Point2D q;
  point_scalars_2d<NI>(ws, th, L, va_ang, ud_ang, q);
  sc[SC_CB] = q.cb; sc[SC_SB] = q.sb; sc[SC_XMAG] = q.xmag;   // cos / sin of beta (atan + heaviside of :552-558)
  sc[SC_K2] = q.k2; sc[SC_K] = q.k; sc[SC_WD] = q.wd; sc[SC_WS] = ws; sc[SC_AE] = L.a_e; sc[SC_IVTE] = L.ivTe; sc[SC_WL] = L.wL; sc[SC_PREF] = L.pref;
  if (ADJ) {
    sc[SC_KX] = q.kx; sc[SC_KY] = q.ky; sc[SC_AA] = q.aa; sc[SC_XEX] = q.xex; sc[SC_XEY] = q.xey; sc[SC_KS] = q.ks; sc[SC_VX] = q.Vx; sc[SC_VY] = q.Vy;
    sc[SC_UX] = q.Ux; sc[SC_UY] = q.Uy; sc[SC_CT] = q.ct; sc[SC_ST] = q.st;
    sc[SC_BG] = (double)((long)id.b * S.G + id.g);
  }
#pragma unroll
  for (int s = 0; s < NI; ++s) { sc[SC_ION + 3 * s] = L.ixi[s]; sc[SC_ION + 1 + 3 * s] = L.a_i[s]; sc[SC_ION + 2 + 3 * s] = L.cs[s]; }
}
// c. rotate + project (:300-324, 371): thread gt's partial column sums of one point into part[parts2d][nv].  VG: also the thread's sums
// of d sample / d cos(beta), d sample / d sin(beta) (one column per thread, nv <= 256; zero otherwise); proj: they also go to record
// `point` of the saving forward (stored here, next to where they are made: a record pointer formed ahead of the sampling stays live
// through it and costs the saving forms a spill).  F: the padded table -- in LDS, or the copy of k_pad2d read through L1/L2.
template <bool LDS, bool VG>
__device__ __forceinline__ void project_point_2d(const double* __restrict__ F, int nv, int pitch, int nvp, int nparts, double cb, double sb,
                                                 double dv, double v0, double idv, int gt, double* part, double& ds1, double& ds2, double* __restrict__ proj = nullptr, long point = 0) {
  if (nv <= 256) {
    const int iy = gt % nvp, pt = gt / nvp;
    if (iy < nv) {
      const int ix0 = (nv * pt) / nparts, ix1 = (nv * (pt + 1)) / nparts;
      const double y = __builtin_fma((double)iy, dv, v0);
      double acc = 0.0, ul, vl, xi_d = (double)ix0;
      line_origin(cb, sb, y, v0, idv, ul, vl);
      if (VG && !LDS) {
        RollVG vg{idv, dv, v0, y, 0.0, 0.0};
        acc = project_rolling_any<true>(F, nv, pitch, cb, sb, ul, vl, ix0, ix1, &vg);
        ds1 = vg.ds1; ds2 = vg.ds2;
      } else if (VG) {
        for (int ix = ix0; ix < ix1; ++ix, xi_d += 1.0) {
          const double x = __builtin_fma(xi_d, dv, v0);
          double Sx, Sy;
          acc += bicubic_sample_vg<LDS>(F, nv, pitch, idv, __builtin_fma(xi_d, cb, ul), __builtin_fma(xi_d, sb, vl), Sx, Sy);
          ds1 += Sx * x + Sy * y;
          ds2 += Sy * x - Sx * y;
        }
      } else if (LDS) {
        for (int ix = ix0; ix < ix1; ++ix, xi_d += 1.0)
          acc += bicubic_sample_lds(F, nv, pitch, __builtin_fma(xi_d, cb, ul), __builtin_fma(xi_d, sb, vl));
      } else {
        acc = project_rolling_any<false>(F, nv, pitch, cb, sb, ul, vl, ix0, ix1);
      }
      if (proj) {
        double* rec = proj2d_record(proj, point, nv) + nv;
        rec[pt * nv + iy] = ds1;
        rec[(nparts + pt) * nv + iy] = ds2;
      }
      part[pt * nv + iy] = acc;
    }
  } else {
    for (int iy = gt; iy < nv; iy += kThreads) {
      const double y = __builtin_fma((double)iy, dv, v0);
      double acc = 0.0, ul, vl, xi_d = 0.0;
      line_origin(cb, sb, y, v0, idv, ul, vl);
      for (int ix = 0; ix < nv; ++ix, xi_d += 1.0)
        acc += bicubic_sample(F, nv, pitch, __builtin_fma(xi_d, cb, ul), __builtin_fma(xi_d, sb, vl));
      part[iy] = acc;
    }
  }
}
// d. the projection f1 = column sums x dv (rec: also into the point's projection record), and its gradient d1: one-sided at the ends
__device__ __forceinline__ void column_sums_2d(const double* part, int nv, int nparts, double dv, int gt, double* f1, double* __restrict__ rec = nullptr) {
  for (int i = gt; i < nv; i += kThreads) {
    double sacc = 0.0;
    for (int q = 0; q < nparts; ++q) sacc += part[q * nv + i];
    f1[i] = sacc * dv;
    if (rec) rec[i] = sacc * dv;
  }
}
__device__ __forceinline__ void gradient_2d(const double* f1, int nv, double idv, int gt, double* d1) {
  for (int i = gt; i < nv; i += kThreads) {
    double gd;
    if (i == 0) gd = (f1[1] - f1[0]) * idv;
    else if (i == nv - 1) gd = (f1[nv - 1] - f1[nv - 2]) * idv;
    else gd = (f1[i + 1] - f1[i - 1]) * (0.5 * idv);
    d1[i] = gd;
  }
}
// e. thread 0: spectrum of the point from R = ratintn sum (red[0..3]), f1, d1 and the scalars in sc[] (:560-585).  Everything the
// adjoint's reverse reads comes back; the forward uses Sv and dop.
template <int NI>
struct Assembly2D {
  int i; bool tin; double t;   // cell and fraction of |xi_e| on the grid; tin: not clamped
  double R, fe_vphi, dfe, ike2, vph, xi[NI], zr[NI], zi[NI], dzr[NI], dzi[NI], gs[NI], iki2[NI];
  double cer, cei, cre, cim, gsum, er, ei, eps2, ce2, ci2, N, Sv, dop;
};
template <int NI, bool REV>
__device__ __forceinline__ void assemble_point_2d(const double2* zp, const double* sc, const double* red, const double* f1, const double* d1,
                                                  int nv, double dv, double v0, double idv, double xmag, Assembly2D<NI>& A) {
  A.R = (red[0] + red[1]) + (red[2] + red[3]);
  const double k2 = sc[SC_K2], k = sc[SC_K], wd = sc[SC_WD], a_e = sc[SC_AE], ivTe = sc[SC_IVTE], wL = sc[SC_WL];
  // jnp.interp(|xi_e|, vx, .): clamps to the end values
  double u = (xmag - v0) * idv;
  int i = (int)u;
  i = i < 0 ? 0 : (i > nv - 2 ? nv - 2 : i);
  double t = (xmag - (v0 + i * dv)) * idv;
  A.tin = t >= 0.0 && t <= 1.0;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  A.i = i; A.t = t;
  A.fe_vphi = f1[i] + t * (f1[i + 1] - f1[i]);
  A.dfe = d1[i] + t * (d1[i + 1] - d1[i]);
  A.ike2 = a_e / k2;
  A.cer = -A.ike2 * A.R; A.cei = kPi * A.ike2 * A.dfe;
  A.cre = 0.0; A.cim = 0.0; A.gsum = 0.0;
  A.vph = wd / k;
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    A.xi[s] = A.vph * sc[SC_ION + 3 * s];
    ion_terms(zp, A.xi[s], A.zr[s], A.zi[s], A.dzr[s], A.dzi[s], A.gs[s]);   // (one thread per point: the Z' table is read from global memory)
    A.iki2[s] = sc[SC_ION + 1 + 3 * s] / k2;
    A.cre -= 0.5 * A.iki2[s] * A.zr[s];
    A.cim -= 0.5 * A.iki2[s] * A.zi[s];
    A.gsum += sc[SC_ION + 2 + 3 * s] * A.gs[s];
  }
  A.er = 1.0 + A.cer + A.cre; A.ei = A.cei + A.cim;
  // Of a sum of two products one is fused into the FMA; which one is written out, so that the result does not depend on the caller
  // (left to the compiler the choice follows the order and the use counts of the code around the call).  The two kernels keep the
  // roundings each of them has always had -- REV (the adjoint): eps2 and ci2 fuse the imaginary part's square, the forward the real
  // part's; ce2 and N are the same in both.
  const double opc = 1.0 + A.cre;
  A.eps2 = REV ? __builtin_fma(A.ei, A.ei, A.er * A.er) : __builtin_fma(A.er, A.er, A.ei * A.ei);
  A.ce2 = __builtin_fma(A.cer, A.cer, A.cei * A.cei);
  A.ci2 = REV ? __builtin_fma(A.cim, A.cim, opc * opc) : __builtin_fma(opc, opc, A.cim * A.cim);
  A.N = __builtin_fma(A.gsum, A.ce2, A.ci2 * A.fe_vphi * ivTe);
  A.Sv = A.N / (k * A.eps2);
  A.dop = 1.0 + 2.0 * wd / wL;
}

template <int NI, bool LDS, int kG2, bool SAVE = false>
__global__ __launch_bounds__(kG2 * kThreads, TSFF_2D_WAVES) void k_form_factor_2d(KStatic S, const double* __restrict__ phys,
                                                                   const double* __restrict__ Fg, int nv,
                                                                   double ud_ang, double va_ang, int f, long pbegin,
                                                                   long pend, double* __restrict__ P,
                                                                   double* __restrict__ proj = nullptr) {
  static_assert(SC_ION + 3 * TSFF_MAX_ION <= kSc2, "the forward's sc[] slots fit kSc2");
  extern __shared__ __align__(16) unsigned char smem[];
  const int grp = threadIdx.x >> 8, gt = threadIdx.x & (kThreads - 1);
  const int nvp = nvp2d(nv), nparts = parts2d(nv);
  double* gbase = reinterpret_cast<double*>(smem) + (size_t)grp * group2d_doubles(nv);
  double* f1 = gbase;              // [nv] projected distribution
  double* d1 = f1 + nv;            // [nv] its gradient
  double* part = d1 + nv;          // [nparts][nv] partial column sums
  double* red = part + nparts * nv;     // [8]
  double* sc = red + 8;            // [kSc2] point scalars
  double* Fl = reinterpret_cast<double*>(smem) + (size_t)kG2 * group2d_doubles(nv);  // padded table (LDS variant)
  const double dv = 12.0 / nv, v0 = -6.0 + 0.5 * dv, idv = 1.0 / dv;  // base.py:333-335
  const int pitch = pitch2d(nv, LDS);
  if (LDS) stage_table_2d(Fg, Fl, nv, pitch, kG2 * kThreads);  // Fg: the plain nv x nv table
  const double* __restrict__ F = LDS ? Fl : Fg;  // (not LDS: Fg is the padded copy made by k_pad2d)
  const long stride = (long)gridDim.x * kG2;
  for (long base = pbegin + (long)blockIdx.x * kG2; base < pend; base += stride) {
    const long pid = base + grp;
    const bool active = pid < pend;  // every group runs the same barrier sequence; idle groups skip the work
    __syncthreads();
    if (active && gt == 0) point_setup_2d<NI, false>(S, phys, f, point_id_2d(pid, S), ud_ang, va_ang, sc);
    __syncthreads();
    const double cb = sc[SC_CB], sb = sc[SC_SB], xmag = sc[SC_XMAG];
    if (active) {
      double ds1 = 0.0, ds2 = 0.0;
      project_point_2d<LDS, SAVE>(F, nv, pitch, nvp, nparts, cb, sb, dv, v0, idv, gt, part, ds1, ds2, SAVE ? proj : nullptr, pid - pbegin);
    }
    __syncthreads();
    if (active) column_sums_2d(part, nv, nparts, dv, gt, f1, SAVE ? proj2d_record(proj, pid - pbegin, nv) : nullptr);
    __syncthreads();
    if (active) gradient_2d(f1, nv, idv, gt, d1);
    __syncthreads();
    // ---- ratintn(df, vx - |xi_e|, vx): nv - 2 intervals (:372-387); the adjoint has its own form of this loop, see above ----
    double psum = 0.0;
    if (active) {
      for (int i = gt; i < nv - 2; i += kThreads) {
        const double f0 = d1[i], f1v = d1[i + 1];
        const double g0 = (v0 + i * dv) - xmag, g1 = (v0 + (i + 1) * dv) - xmag;
        const double fdif = f1v - f0, gdif = g1 - g0, fav = 0.5 * (f1v + f0), gav = 0.5 * (g1 + g0);
        const double tmp = fav * gdif - gav * fdif;
        double r;
        if (fabs(gdif) < 1.0e-4 * fabs(gav)) r = fav / gav + tmp * gdif / (12.0 * gav * gav * gav);
        else r = fdif / gdif + tmp * log(fabs((gav + 0.5 * gdif) / (gav - 0.5 * gdif))) / (gdif * gdif);
        psum += r * dv;
      }
    }
    psum = wave_sum(psum);
    if ((gt & 63) == 0) red[gt >> 6] = psum;
    __syncthreads();
    if (active && gt == 0) {
      Assembly2D<NI> A;
      assemble_point_2d<NI, false>(S.zp, sc, red, f1, d1, nv, dv, v0, idv, xmag, A);
      P[pid] = A.Sv * A.dop * sc[SC_PREF] * sc[SC_WS] * sc[SC_WS];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Adjoint of k_form_factor_2d.  The same workgroup structure and, up to the point's spectrum, the same shared steps (the projection
// with its derivative sums, or read from the records of a saving forward); then, per point:
//   one thread reverses the spectrum assembly (-> adjoints of R, fe(v_phi), dfe and of the point scalars),
//   the group reverses ratintn, the two interpolations and the finite-difference gradient (-> f1bar[iy]),
//   a second sampling sweep with derivative weights gives the adjoint of the rotation (cos beta, sin beta),
//   one thread finishes the chain to the lineout scalars (LineS fields) and adds them to LBacc[b][g][:].
// f1bar is also written to global memory for the table adjoint (k_ff2d_table_adj): the scatter into the table needs the
// sample weights only, not the table, so it runs as a separate pass whose LDS holds the table ADJOINT.
// ------------------------------------------------------------------------------------------
template <int NI, bool LDS, int kG2>
__global__ __launch_bounds__(kG2 * kThreads) void k_form_factor_2d_adj(KStatic S, const double* __restrict__ phys,
                                                                       const double* __restrict__ Fg, int nv, double ud_ang,
                                                                       double va_ang, int f, long pbegin, long pend,
                                                                       const double* __restrict__ Pbar,
                                                                       double* __restrict__ LBacc, double* __restrict__ f1bar_out,
                                                                       const double* __restrict__ proj = nullptr) {
  constexpr int NLB = kNLB2 + 3 * NI;
  static_assert(SC_ACC + kNLB2 + 3 * TSFF_MAX_ION + 1 <= kScA, "the adjoint's sc[] slots fit kScA");
  extern __shared__ __align__(16) unsigned char smem[];
  const int grp = threadIdx.x >> 8, gt = threadIdx.x & (kThreads - 1);
  const int nvp = nvp2d(nv), nparts = parts2d(nv);
  double* gbase = reinterpret_cast<double*>(smem) + (size_t)grp * group2d_adj_doubles(nv);
  double* f1 = gbase;              // [nv] projected distribution, later f1bar
  double* d1 = f1 + nv;            // [nv] its gradient, later d1bar
  double* part = d1 + nv;          // [nparts][nv] partial sums (two values per part in the derivative sweep: reused)
  double* c0 = part + nparts * nv;  // [nv] per-interval adjoint to d1[i]
  double* c1 = c0 + nv;            // [nv] per-interval adjoint to d1[i + 1]
  double* red = c1 + nv;           // [16]
  double* sc = red + 16;           // [kScA] point scalars and adjoints
  double* Fl = reinterpret_cast<double*>(smem) + (size_t)kG2 * group2d_adj_doubles(nv);
  const double dv = 12.0 / nv, v0 = -6.0 + 0.5 * dv, idv = 1.0 / dv;
  const int pitch = pitch2d(nv, LDS);
  if (LDS) stage_table_2d(Fg, Fl, nv, pitch, kG2 * kThreads);
  const double* __restrict__ F = LDS ? Fl : Fg;
  if (gt == 0) sc[SC_ACC + NLB] = -1.0;   // no (lineout, gradient point) accumulated yet (each group's thread 0 owns its slot)
  const int nworker = (int)gridDim.x * kG2, worker = (int)blockIdx.x * kG2 + grp;   // one partial slot per point group
  const long stride = (long)gridDim.x * kG2;
  for (long base = pbegin + (long)blockIdx.x * kG2; base < pend; base += stride) {
    const long pid = base + grp;
    const bool active = pid < pend;
    __syncthreads();
    if (active && gt == 0) point_setup_2d<NI, true>(S, phys, f, point_id_2d(pid, S), ud_ang, va_ang, sc);   // (the forward's own set-up: the same rotation, the same projection, bit for bit)
    __syncthreads();
    const double cb = sc[SC_CB], sb = sc[SC_SB], xmag = sc[SC_XMAG];
    // ---- forward projection; with one column per thread (nv <= 256) also the derivative sums of that column ----
    double ds1 = 0.0, ds2 = 0.0;   // sum over the thread's samples of d sample / d cos(beta), d sample / d sin(beta)
    if (active && proj) {           // the SAVE pass of the forward left both: no sampling here
      const double* rec = proj2d_record(proj, pid - pbegin, nv);
      const int iy = gt % nvp, pt = gt / nvp;
      if (iy < nv) {
        ds1 = rec[nv + pt * nv + iy];
        ds2 = rec[nv + (nparts + pt) * nv + iy];
      }
    } else if (active) {
      project_point_2d<LDS, true>(F, nv, pitch, nvp, nparts, cb, sb, dv, v0, idv, gt, part, ds1, ds2);
    }
    __syncthreads();
    if (active && proj) {
      const double* rec = proj2d_record(proj, pid - pbegin, nv);
      for (int i = gt; i < nv; i += kThreads) f1[i] = rec[i];
    } else if (active)
      column_sums_2d(part, nv, nparts, dv, gt, f1);
    __syncthreads();
    if (active) gradient_2d(f1, nv, idv, gt, d1);
    __syncthreads();
    // ---- ratintn forward (value) and its partial derivatives per interval (the small-interval branch through ig and c, which the
    //      partials reuse: not the forward's roundings, see the shared steps) ----
    double psum = 0.0;
    if (active)
      for (int i = gt; i < nv - 2; i += kThreads) {
        const double f0 = d1[i], f1v = d1[i + 1];
        const double g0 = (v0 + i * dv) - xmag, g1 = (v0 + (i + 1) * dv) - xmag;
        const double fdif = f1v - f0, gdif = g1 - g0, fav = 0.5 * (f1v + f0), gav = 0.5 * (g1 + g0);
        const double tmp = fav * gdif - gav * fdif;
        double r, rfd, rfa, rga;   // r and dr/d(fdif, fav, gav)
        if (fabs(gdif) < 1.0e-4 * fabs(gav)) {
          const double ig = 1.0 / gav, c = gdif / (12.0 * gav * gav * gav);
          r = fav * ig + tmp * c;
          rfd = -gav * c; rfa = ig + gdif * c;
          rga = -fav * ig * ig - fdif * c - 3.0 * tmp * c * ig;
        } else {
          const double lg = log(fabs((gav + 0.5 * gdif) / (gav - 0.5 * gdif))), ig2 = 1.0 / (gdif * gdif);
          r = fdif / gdif + tmp * lg * ig2;
          rfd = 1.0 / gdif - gav * lg * ig2;
          rfa = gdif * lg * ig2;
          rga = (-fdif * lg + tmp * (1.0 / (gav + 0.5 * gdif) - 1.0 / (gav - 0.5 * gdif))) * ig2;
        }
        psum += r * dv;
        c0[i] = (-rfd + 0.5 * rfa) * dv;   // d(sum r dv)/d d1[i]
        c1[i] = (rfd + 0.5 * rfa) * dv;    // d(sum r dv)/d d1[i + 1]
        part[i] = -rga * dv;               // d(sum r dv)/d xmag   (gav = mid - xmag)
      }
    psum = wave_sum(psum);
    if ((gt & 63) == 0) red[gt >> 6] = psum;
    __syncthreads();
    // ---- one thread: forward assembly and its reverse ----
    if (active && gt == 0) {
      const double k2 = sc[SC_K2], k = sc[SC_K], wd = sc[SC_WD], ws = sc[SC_WS], a_e = sc[SC_AE], ivTe = sc[SC_IVTE], wL = sc[SC_WL];
      Assembly2D<NI> A;
      assemble_point_2d<NI, true>(S.zp, sc, red, f1, d1, nv, dv, v0, idv, xmag, A);
      const double Q = sc[SC_PREF] * ws * ws;
      // reverse
      const double Pb = Pbar[pid];
      const double Svb = Pb * A.dop * Q;
      double wdb = Pb * A.Sv * Q * 2.0 / wL;
      double wLb = -Pb * A.Sv * Q * 2.0 * wd / (wL * wL);
      const double prefb = Pb * A.Sv * A.dop * ws * ws;
      const double Nb = Svb / (k * A.eps2);
      double kb = -Svb * A.N / (k * k * A.eps2);
      const double eps2b = -Svb * A.N / (k * A.eps2 * A.eps2);
      const double gsumb = Nb * A.ce2, ce2b = Nb * A.gsum, ci2b = Nb * A.fe_vphi * ivTe;
      const double fevb = Nb * A.ci2 * ivTe;
      double ivTeb = Nb * A.ci2 * A.fe_vphi;
      const double erb = 2.0 * A.er * eps2b, eib = 2.0 * A.ei * eps2b;
      const double cerb = erb + 2.0 * A.cer * ce2b, ceib = eib + 2.0 * A.cei * ce2b;
      const double creb = erb + 2.0 * (1.0 + A.cre) * ci2b, cimb = eib + 2.0 * A.cim * ci2b;
      double ike2b = -cerb * A.R + ceib * kPi * A.dfe;
      const double Rb = -cerb * A.ike2, dfeb = ceib * kPi * A.ike2;
      const double a_eb = ike2b / k2;
      double k2b = -ike2b * a_e / (k2 * k2);
      double vphb = 0.0;
      double* ob = sc + SC_IONB;  // adjoints of the ion scalars: [ixi, a_i, cs] per species
#pragma unroll
      for (int s = 0; s < NI; ++s) {
        const double iki2b = -0.5 * (creb * A.zr[s] + cimb * A.zi[s]);
        const double zrb = -0.5 * A.iki2[s] * creb, zib = -0.5 * A.iki2[s] * cimb;
        const double gsb = gsumb * sc[SC_ION + 2 + 3 * s];
        const double xib = zrb * A.dzr[s] + zib * A.dzi[s] + gsb * A.gs[s] * (-2.0 * A.xi[s]);
        ob[3 * s + 2] = gsumb * A.gs[s];          // cs
        ob[3 * s + 1] = iki2b / k2;               // a_i
        k2b -= iki2b * sc[SC_ION + 1 + 3 * s] / (k2 * k2);
        vphb += xib * sc[SC_ION + 3 * s];
        ob[3 * s] = xib * A.vph;                  // ixi
      }
      wdb += vphb / k;
      kb -= vphb * wd / (k * k);
      k2b += kb / (2.0 * k);
      // the two interpolations at |xi_e| (jnp.interp: zero slope where clamped)
      double xmagb = A.tin ? (fevb * (f1[A.i + 1] - f1[A.i]) + dfeb * (d1[A.i + 1] - d1[A.i])) * idv : 0.0;
      sc[SC_RB] = Rb; sc[SC_FEVB] = fevb; sc[SC_DFEB] = dfeb; sc[SC_IL] = (double)A.i; sc[SC_T] = A.t;
      sc[SC_XMAGB] = xmagb; sc[SC_WDB] = wdb; sc[SC_WLB] = wLb; sc[SC_PREFB] = prefb; sc[SC_IVTEB] = ivTeb; sc[SC_AEB] = a_eb; sc[SC_K2B] = k2b;
    }
    __syncthreads();
    // ---- group: d1bar, xmagbar (ratintn part), f1bar ----
    double xms = 0.0;
    if (active) {
      const double Rb = sc[SC_RB], dfeb = sc[SC_DFEB], t = sc[SC_T];
      const int il = (int)sc[SC_IL];
      for (int i = gt; i < nv - 2; i += kThreads) xms += part[i] * Rb;
      for (int i = gt; i < nv; i += kThreads) {
        double v = 0.0;
        if (i < nv - 2) v += c0[i] * Rb;
        if (i >= 1 && i - 1 < nv - 2) v += c1[i - 1] * Rb;
        if (i == il) v += dfeb * (1.0 - t);
        if (i == il + 1) v += dfeb * t;
        c0[i] = v;   // d1bar, in place: a thread reads c0 only at its own index here, c1 is not written in this loop
      }
    }
    xms = wave_sum(xms);
    if ((gt & 63) == 0) red[8 + (gt >> 6)] = xms;
    __syncthreads();
    if (active) {
      const double fevb = sc[SC_FEVB], t = sc[SC_T];
      const int il = (int)sc[SC_IL];
      for (int i = gt; i < nv; i += kThreads) {   // gradient stencil transposed + the fe(v_phi) interpolation
        double v = 0.0;
        if (i + 1 <= nv - 2 && i + 1 >= 1) v -= 0.5 * idv * c0[i + 1];
        if (i - 1 >= 1 && i - 1 <= nv - 2) v += 0.5 * idv * c0[i - 1];
        if (i == 1) v += idv * c0[0];
        if (i == 0) v -= idv * c0[0];
        if (i == nv - 1) v += idv * c0[nv - 1];
        if (i == nv - 2) v -= idv * c0[nv - 1];
        if (i == il) v += fevb * (1.0 - t);
        if (i == il + 1) v += fevb * t;
        c1[i] = v;   // f1bar
      }
    }
    __syncthreads();
    if (active && f1bar_out)
    {
      for (int i = gt; i < nv; i += kThreads) f1bar_out[(size_t)(pid - pbegin) * (nv + 2) + i] = c1[i];
      if (gt == 0) { f1bar_out[(size_t)(pid - pbegin) * (nv + 2) + nv] = cb; f1bar_out[(size_t)(pid - pbegin) * (nv + 2) + nv + 1] = sb; }
    }
    // ---- adjoint of (cos beta, sin beta): f1bar contracted with the derivative sums (carried from the projection pass, or
    //      by a second sampling sweep when a thread owns several columns) ----
    double acb = 0.0, asb = 0.0;
    if (active) {
      if (nv <= 256) {
        const int iy = gt % nvp;
        if (iy < nv) {
          acb = ds1 * c1[iy] * dv;
          asb = ds2 * c1[iy] * dv;
        }
      } else {
        for (int iy = gt; iy < nv; iy += kThreads) {
          const double y = __builtin_fma((double)iy, dv, v0);
          double s1 = 0.0, s2 = 0.0, ul, vl;
          line_origin(cb, sb, y, v0, idv, ul, vl);
          for (int ix = 0; ix < nv; ++ix) {
            const double x = v0 + ix * dv;
            double Sx, Sy;
            bicubic_sample_vg<false>(F, nv, pitch, idv, __builtin_fma((double)ix, cb, ul), __builtin_fma((double)ix, sb, vl), Sx, Sy);
            s1 += Sx * x + Sy * y;
            s2 += -Sx * y + Sy * x;
          }
          acb += s1 * c1[iy] * dv;
          asb += s2 * c1[iy] * dv;
        }
      }
    }
    acb = wave_sum(acb);
    asb = wave_sum(asb);
    if ((gt & 63) == 0) { red[gt >> 6] = acb; red[4 + (gt >> 6)] = asb; }
    __syncthreads();
    // ---- one thread: chain to the lineout scalars ----
    if (active && gt == 0) {
      const double cbb = (red[0] + red[1]) + (red[2] + red[3]), sbb = (red[4] + red[5]) + (red[6] + red[7]);
      double xmagb = sc[SC_XMAGB] + (red[8] + red[9]) + (red[10] + red[11]);
      double wdb = sc[SC_WDB], wLb = sc[SC_WLB], ivTeb = sc[SC_IVTEB], k2b = sc[SC_K2B];
      const double prefb = sc[SC_PREFB], a_eb = sc[SC_AEB];
      const double k2 = sc[SC_K2], wd = sc[SC_WD], ivTe = sc[SC_IVTE], kx = sc[SC_KX], ky = sc[SC_KY], aa = sc[SC_AA], xex = sc[SC_XEX], xey = sc[SC_XEY];
      const double ks = sc[SC_KS], Vx = sc[SC_VX], Vy = sc[SC_VY], Ux = sc[SC_UX], Uy = sc[SC_UY], ct = sc[SC_CT], st = sc[SC_ST];
      // cb = xex / xmag, sb = xey / xmag, xmag = |(xex, xey)|
      const double xm = sc[SC_XMAG];
      const double xmt = xmagb - (cbb * xex + sbb * xey) / (xm * xm);
      const double xexb = cbb / xm + xmt * xex / xm, xeyb = sbb / xm + xmt * xey / xm;
      // xex = (aa kx - Ux) ivTe
      double aab = (xexb * kx + xeyb * ky) * ivTe;
      double kxb = xexb * aa * ivTe, kyb = xeyb * aa * ivTe;
      const double Uxb = -xexb * ivTe, Uyb = -xeyb * ivTe;
      ivTeb += xexb * (aa * kx - Ux) + xeyb * (aa * ky - Uy);
      // aa = wd / k2
      wdb += aab / k2;
      k2b -= aab * wd / (k2 * k2);
      // wd = ws - wL - (kx Vx + ky Vy)
      wLb -= wdb;
      kxb -= wdb * Vx; kyb -= wdb * Vy;
      const double Vxb = -wdb * kx, Vyb = -wdb * ky;
      // k2 = kx^2 + ky^2
      kxb += 2.0 * kx * k2b; kyb += 2.0 * ky * k2b;
      // kx = ct ks - kL, ky = st ks
      const double ksb = ct * kxb + st * kyb;
      const double kLb = -kxb;
      const double wpe2b = -ksb / (2.0 * kC * kC * ks);
      const double Vdb = Vxb * cos(va_ang) + Vyb * sin(va_ang);
      const double Udb = Uxb * cos(ud_ang) + Uyb * sin(ud_ang);
      // running sums per group in LDS, flushed into the worker's partial slot when the (lineout, gradient point) of the
      // group's points changes and at the end: every point of an ARTS image belongs to the same (b, g), and 250 000 atomic
      // updates of the same eleven addresses had made this the longest phase of the kernel (24 of 28 ms)
      double* accl = sc + SC_ACC;
      const double bg = sc[SC_BG];
      if (accl[NLB] != bg) {
        if (accl[NLB] >= 0.0) {   // (plain stores into this worker's own slot: k_lbacc_reduce sums the workers in a fixed order)
          double* o = LBacc + ((size_t)accl[NLB] * nworker + worker) * NLB;
          for (int k = 0; k < NLB; ++k) o[k] = accl[k];
        }
        for (int k = 0; k < NLB; ++k) accl[k] = 0.0;
        accl[NLB] = bg;
      }
      accl[0] += wpe2b; accl[1] += wLb; accl[2] += kLb; accl[3] += ivTeb;
      accl[4] += a_eb; accl[5] += prefb; accl[6] += Udb; accl[7] += Vdb;
#pragma unroll
      for (int s = 0; s < NI; ++s) { accl[kNLB2 + 3 * s] += sc[SC_IONB + 3 * s]; accl[kNLB2 + 1 + 3 * s] += sc[SC_IONB + 1 + 3 * s]; accl[kNLB2 + 2 + 3 * s] += sc[SC_IONB + 2 + 3 * s]; }
    }
  }
  if (gt == 0 && sc[SC_ACC + NLB] >= 0.0) {   // flush of the last (lineout, gradient point) of this group
    double* o = LBacc + ((size_t)sc[SC_ACC + NLB] * nworker + worker) * NLB;
    for (int k = 0; k < NLB; ++k) o[k] = sc[SC_ACC + k];
  }
}

// LBacc[bg][k] = sum over the workers w of parts[bg][w][k] in a FIXED order (thread t takes w = t, t + 256, ...; then the
// wavefront butterflies and the four wavefront sums in order): the lineout-scalar adjoints of the form-factor adjoints are
// bit-reproducible run to run -- they used to be global atomics.  Grid: one workgroup per (lineout, gradient point).
__global__ __launch_bounds__(kThreads) void k_lbacc_reduce(const double* __restrict__ parts, int nworker, int NLB,
                                                           double* __restrict__ LBacc) {
  __shared__ double red[8];
  const double* p = parts + (size_t)blockIdx.x * nworker * NLB;
  for (int k = 0; k < NLB; ++k) {
    double a = 0.0;
    for (int w = threadIdx.x; w < nworker; w += kThreads) a += p[(size_t)w * NLB + k];
    const double v = block_sum(a, red);
    if (threadIdx.x == 0) LBacc[(size_t)blockIdx.x * NLB + k] = v;
  }
}

// Table adjoint: Fbar[cell entries] += f1bar[point][iy] dv wx[m] wy[n] for every sample of every point.  The scatter needs
// the sample weights only, so the LDS of this pass holds the padded table ADJOINT (LDS atomics, ds_add_f64); each
// persistent workgroup adds its partial table to the global one at the end.  Tables larger than LDS are cut into tiles
// of kTile2 x kTile2 cells (blockIdx.y = tile; a tile of cells touches (kTile2 + 3)^2 padded entries): the workgroups
// of a tile walk ALL points but visit only the samples whose cell lies in their tile -- per column iy that is one
// contiguous run of ix, found from the intersection of the rotated line with the tile rectangle (taken two samples
// wide on each side and then decided per sample by the very floor() every tile evaluates, so that each sample lands in
// exactly one tile).
constexpr int kTile2 = 128;
// indices ix with lo <= c * ix + e < hi (lo_inf / hi_inf: that side is open), widened by two
__device__ __forceinline__ void line_range(double c, double e, double lo, double hi, bool lo_inf, bool hi_inf, int& a, int& b) {
  if (fabs(c) < 1.0e-9) return;   // (almost) parallel to the tile edge: the per-sample test decides
  double x0 = lo_inf ? -1.0e9 : (lo - e) / c, x1 = hi_inf ? 1.0e9 : (hi - e) / c;
  if (c < 0.0) { const double t = x0; x0 = x1; x1 = t; if (lo_inf) x1 = 1.0e9; if (hi_inf) x0 = -1.0e9; }
  x0 = fmin(fmax(x0, -1.0e9), 1.0e9);
  x1 = fmin(fmax(x1, -1.0e9), 1.0e9);
  const int ia = (int)floor(x0) - 2, ib = (int)ceil(x1) + 2;
  a = a > ia ? a : ia;
  b = b < ib ? b : ib;
}
// One line's scatter as a LOCKSTEP walk with a rolling window of SUMS.  The samples of a line that fall into the tile are one run
// (the clamped cell indices are monotone along the line); inside it a 4 x 4 register window follows the cell and only the row /
// column that leaves it goes to LDS (4 atomics per axis step instead of 16 per sample).  Written with per-lane control flow
// (`continue` outside the tile, loops that advance the window) every wavefront executed the union of its lanes' paths, 140
// instructions per sample at 0.63 lane utilisation, and the kernel was bound by that, not by its LDS atomics (plain stores in
// their place: 298 -> 273 ms at 256^2; DESIGN.md section 4.3).  Here all lanes of a wavefront take the
// same steps k = 0 .. n_max - 1 (n_max: the longest chord among them) and everything lane-dependent is an exec mask held in a scalar
// register pair, as in project_rolling: `valid` (k inside the lane's chord), `inside` (the sample's cell inside the tile), `started`
// (the window has seen an inside sample: before that it is all zero and only follows the cell), the two shift masks.  The cell is
// carried incrementally (cell index as a double, fraction, LDS byte address of the window's origin): exact, so every tile decides a
// sample's cell alike.  A shift sends the leaving row / column to LDS (four ds_add_f64 in the lanes that shift AND have started),
// moves the window and steps the cursor inside one masked block.  After the chord the window is flushed (16 ds_add_f64).
// Walk direction: non-decreasing cx (dir = +1 for cos >= 0, else the line is taken backwards), cy then moves one way (SGY).
typedef double __attribute__((address_space(3))) lds_double_t;
template <int SGY, bool WHOLE>
__device__ __forceinline__ void scatter_line_lockstep(double* __restrict__ T, int pitch, int nv, int cx0, int cx1, int cy0, int cy1,
                                                      bool fwd, int ix0, int ix1, double cb, double sb, double ul, double vl, double val) {
#pragma clang fp contract(off)
  const int len = ix1 > ix0 ? ix1 - ix0 : 0;
  int nm = len;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(nm, o, 64); nm = v > nm ? v : nm; }
  const int nmax = __builtin_amdgcn_readfirstlane(nm);
  if (nmax == 0) return;
  const double dir = fwd ? 1.0 : -1.0;
  double x_d = (double)(fwd ? ix0 : ix1 - 1);
  double tx, ty, cdx, cdy;
  unsigned addr;   // LDS byte address of the window's origin entry (meaningful once inside the tile)
  {
    int cx, cy;
    cell_of(__builtin_fma(x_d, cb, ul), nv, cx, tx);
    cell_of(__builtin_fma(x_d, sb, vl), nv, cy, ty);
    cdx = (double)cx; cdy = (double)cy;
    addr = (unsigned)(unsigned long long)((lds_double_t*)T) + (unsigned)(((cx - cx0) * pitch + (cy - cy0)) * 8);
  }
  const int p8 = pitch * 8;
  double cmax = (double)(nv - 2), bx0 = (double)cx0, bx1 = (double)cx1, by0 = (double)cy0, by1 = (double)cy1;
  double A[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) A[m][n] = 0.0;
  unsigned long long started = 0;
  for (int k = 0; k < nmax; ++k) {
    unsigned long long valid, inside;
    asm("v_cmp_gt_i32 %0, %1, %2" : "=s"(valid) : "v"(len), "s"(k));
    if (WHOLE) inside = valid;
    else {
      unsigned long long c0, c1, c2, c3;
      asm("v_cmp_ge_f64 %0, %1, %2" : "=s"(c0) : "v"(cdx), "v"(bx0));
      asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(c1) : "v"(cdx), "v"(bx1));
      asm("v_cmp_ge_f64 %0, %1, %2" : "=s"(c2) : "v"(cdy), "v"(by0));
      asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(c3) : "v"(cdy), "v"(by1));
      inside = valid & c0 & c1 & c2 & c3;
    }
    started |= inside;
    // the sample's contribution (zero outside the tile: each sample lands in exactly one tile)
    {
      double wx[4], wy[4], ve;
      catmull_rom(tx, wx);
      catmull_rom(ty, wy);
      {
        unsigned lo, hi;
        asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(lo) : "v"(__double2loint(val)), "s"(inside));
        asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(hi) : "v"(__double2hiint(val)), "s"(inside));
        ve = __hiloint2double((int)hi, (int)lo);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const double wm = ve * wx[m];
#pragma unroll
        for (int n = 0; n < 4; ++n) A[m][n] = __builtin_fma(wm, wy[n], A[m][n]);
      }
    }
    // the next position against the current cell, the shift masks (only while the lane's chord lasts)
    x_d += dir;
    tx = __builtin_fma(x_d, cb, ul) - cdx;
    ty = __builtin_fma(x_d, sb, vl) - cdy;
    unsigned long long mx, my, ex, ey;
    asm("v_cmp_le_f64 %0, 1.0, %1" : "=s"(mx) : "v"(tx));
    asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(ex) : "v"(cdx), "v"(cmax));
    if (SGY > 0) { asm("v_cmp_le_f64 %0, 1.0, %1" : "=s"(my) : "v"(ty)); asm("v_cmp_lt_f64 %0, %1, %2" : "=s"(ey) : "v"(cdy), "v"(cmax)); }
    else { asm("v_cmp_gt_f64 %0, 0, %1" : "=s"(my) : "v"(ty)); asm("v_cmp_lt_f64 %0, 0, %1" : "=s"(ey) : "v"(cdy)); }
    mx &= ex & valid; my &= ey & valid;
    const unsigned long long fx = mx & started, fy = my & started;
    unsigned long long sv;
    // row 0 leaves (cx grows): T[origin + n] += A[0][n]; rows move up; the cursor steps
    asm volatile(
        "s_and_saveexec_b64 %[sv], %[f]\n\t"
        "ds_add_f64 %[ad], %[a00]\n\tds_add_f64 %[ad], %[a01] offset:8\n\tds_add_f64 %[ad], %[a02] offset:16\n\tds_add_f64 %[ad], %[a03] offset:24\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_and_saveexec_b64 %[sv], %[m]\n\t"
        "v_mov_b64 %[a00], %[a10]\n\tv_mov_b64 %[a10], %[a20]\n\tv_mov_b64 %[a20], %[a30]\n\tv_mov_b64 %[a30], 0\n\t"
        "v_mov_b64 %[a01], %[a11]\n\tv_mov_b64 %[a11], %[a21]\n\tv_mov_b64 %[a21], %[a31]\n\tv_mov_b64 %[a31], 0\n\t"
        "v_mov_b64 %[a02], %[a12]\n\tv_mov_b64 %[a12], %[a22]\n\tv_mov_b64 %[a22], %[a32]\n\tv_mov_b64 %[a32], 0\n\t"
        "v_mov_b64 %[a03], %[a13]\n\tv_mov_b64 %[a13], %[a23]\n\tv_mov_b64 %[a23], %[a33]\n\tv_mov_b64 %[a33], 0\n\t"
        "v_add_f64 %[cd], %[cd], 1.0\n\tv_add_f64 %[t], %[t], -1.0\n\tv_add_u32 %[ad], %[p8], %[ad]\n\t"
        "s_mov_b64 exec, %[sv]"
        : [sv] "=&s"(sv), [a00] "+v"(A[0][0]), [a01] "+v"(A[0][1]), [a02] "+v"(A[0][2]), [a03] "+v"(A[0][3]), [a10] "+v"(A[1][0]),
          [a11] "+v"(A[1][1]), [a12] "+v"(A[1][2]), [a13] "+v"(A[1][3]), [a20] "+v"(A[2][0]), [a21] "+v"(A[2][1]), [a22] "+v"(A[2][2]),
          [a23] "+v"(A[2][3]), [a30] "+v"(A[3][0]), [a31] "+v"(A[3][1]), [a32] "+v"(A[3][2]), [a33] "+v"(A[3][3]), [cd] "+v"(cdx),
          [t] "+v"(tx), [ad] "+v"(addr)
        : [f] "s"(fx), [m] "s"(mx), [p8] "s"(p8)
        : "scc", "memory");
    // one column leaves: the first (cy growing) or the last (cy falling); T[origin + m pitch (+ 3)] += A[m][0 | 3]
    {
      unsigned a1, a2, a3;
      if (SGY > 0)
        asm volatile(
            "s_and_saveexec_b64 %[sv], %[f]\n\t"
            "v_add_u32 %[a1], %[p8], %[ad]\n\tv_add_u32 %[a2], %[p8], %[a1]\n\tv_add_u32 %[a3], %[p8], %[a2]\n\t"
            "ds_add_f64 %[ad], %[a00]\n\tds_add_f64 %[a1], %[a10]\n\tds_add_f64 %[a2], %[a20]\n\tds_add_f64 %[a3], %[a30]\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_and_saveexec_b64 %[sv], %[m]\n\t"
            "v_mov_b64 %[a00], %[a01]\n\tv_mov_b64 %[a01], %[a02]\n\tv_mov_b64 %[a02], %[a03]\n\tv_mov_b64 %[a03], 0\n\t"
            "v_mov_b64 %[a10], %[a11]\n\tv_mov_b64 %[a11], %[a12]\n\tv_mov_b64 %[a12], %[a13]\n\tv_mov_b64 %[a13], 0\n\t"
            "v_mov_b64 %[a20], %[a21]\n\tv_mov_b64 %[a21], %[a22]\n\tv_mov_b64 %[a22], %[a23]\n\tv_mov_b64 %[a23], 0\n\t"
            "v_mov_b64 %[a30], %[a31]\n\tv_mov_b64 %[a31], %[a32]\n\tv_mov_b64 %[a32], %[a33]\n\tv_mov_b64 %[a33], 0\n\t"
            "v_add_f64 %[cd], %[cd], 1.0\n\tv_add_f64 %[t], %[t], -1.0\n\tv_add_u32 %[ad], 8, %[ad]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(sv), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [a00] "+v"(A[0][0]), [a01] "+v"(A[0][1]), [a02] "+v"(A[0][2]),
              [a03] "+v"(A[0][3]), [a10] "+v"(A[1][0]), [a11] "+v"(A[1][1]), [a12] "+v"(A[1][2]), [a13] "+v"(A[1][3]), [a20] "+v"(A[2][0]),
              [a21] "+v"(A[2][1]), [a22] "+v"(A[2][2]), [a23] "+v"(A[2][3]), [a30] "+v"(A[3][0]), [a31] "+v"(A[3][1]), [a32] "+v"(A[3][2]),
              [a33] "+v"(A[3][3]), [cd] "+v"(cdy), [t] "+v"(ty), [ad] "+v"(addr)
            : [f] "s"(fy), [m] "s"(my), [p8] "s"(p8)
            : "scc", "memory");
      else
        asm volatile(
            "s_and_saveexec_b64 %[sv], %[f]\n\t"
            "v_add_u32 %[a1], %[p8], %[ad]\n\tv_add_u32 %[a2], %[p8], %[a1]\n\tv_add_u32 %[a3], %[p8], %[a2]\n\t"
            "ds_add_f64 %[ad], %[a03] offset:24\n\tds_add_f64 %[a1], %[a13] offset:24\n\tds_add_f64 %[a2], %[a23] offset:24\n\tds_add_f64 %[a3], %[a33] offset:24\n\t"
            "s_mov_b64 exec, %[sv]\n\t"
            "s_and_saveexec_b64 %[sv], %[m]\n\t"
            "v_mov_b64 %[a03], %[a02]\n\tv_mov_b64 %[a02], %[a01]\n\tv_mov_b64 %[a01], %[a00]\n\tv_mov_b64 %[a00], 0\n\t"
            "v_mov_b64 %[a13], %[a12]\n\tv_mov_b64 %[a12], %[a11]\n\tv_mov_b64 %[a11], %[a10]\n\tv_mov_b64 %[a10], 0\n\t"
            "v_mov_b64 %[a23], %[a22]\n\tv_mov_b64 %[a22], %[a21]\n\tv_mov_b64 %[a21], %[a20]\n\tv_mov_b64 %[a20], 0\n\t"
            "v_mov_b64 %[a33], %[a32]\n\tv_mov_b64 %[a32], %[a31]\n\tv_mov_b64 %[a31], %[a30]\n\tv_mov_b64 %[a30], 0\n\t"
            "v_add_f64 %[cd], %[cd], -1.0\n\tv_add_f64 %[t], %[t], 1.0\n\tv_add_u32 %[ad], -8, %[ad]\n\t"
            "s_mov_b64 exec, %[sv]"
            : [sv] "=&s"(sv), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [a00] "+v"(A[0][0]), [a01] "+v"(A[0][1]), [a02] "+v"(A[0][2]),
              [a03] "+v"(A[0][3]), [a10] "+v"(A[1][0]), [a11] "+v"(A[1][1]), [a12] "+v"(A[1][2]), [a13] "+v"(A[1][3]), [a20] "+v"(A[2][0]),
              [a21] "+v"(A[2][1]), [a22] "+v"(A[2][2]), [a23] "+v"(A[2][3]), [a30] "+v"(A[3][0]), [a31] "+v"(A[3][1]), [a32] "+v"(A[3][2]),
              [a33] "+v"(A[3][3]), [cd] "+v"(cdy), [t] "+v"(ty), [ad] "+v"(addr)
            : [f] "s"(fy), [m] "s"(my), [p8] "s"(p8)
            : "scc", "memory");
    }
  }
  // the last window of every lane that has been inside the tile
  {
    unsigned long long sv;
    unsigned a1, a2, a3;
    asm volatile(
        "s_and_saveexec_b64 %[sv], %[f]\n\t"
        "v_add_u32 %[a1], %[p8], %[ad]\n\tv_add_u32 %[a2], %[p8], %[a1]\n\tv_add_u32 %[a3], %[p8], %[a2]\n\t"
        "ds_add_f64 %[ad], %[a00]\n\tds_add_f64 %[ad], %[a01] offset:8\n\tds_add_f64 %[ad], %[a02] offset:16\n\tds_add_f64 %[ad], %[a03] offset:24\n\t"
        "ds_add_f64 %[a1], %[a10]\n\tds_add_f64 %[a1], %[a11] offset:8\n\tds_add_f64 %[a1], %[a12] offset:16\n\tds_add_f64 %[a1], %[a13] offset:24\n\t"
        "ds_add_f64 %[a2], %[a20]\n\tds_add_f64 %[a2], %[a21] offset:8\n\tds_add_f64 %[a2], %[a22] offset:16\n\tds_add_f64 %[a2], %[a23] offset:24\n\t"
        "ds_add_f64 %[a3], %[a30]\n\tds_add_f64 %[a3], %[a31] offset:8\n\tds_add_f64 %[a3], %[a32] offset:16\n\tds_add_f64 %[a3], %[a33] offset:24\n\t"
        "s_mov_b64 exec, %[sv]\n\t"
        "s_waitcnt lgkmcnt(0)"
        : [sv] "=&s"(sv), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3)
        : [f] "s"(started), [ad] "v"(addr), [p8] "s"(p8), [a00] "v"(A[0][0]), [a01] "v"(A[0][1]), [a02] "v"(A[0][2]), [a03] "v"(A[0][3]),
          [a10] "v"(A[1][0]), [a11] "v"(A[1][1]), [a12] "v"(A[1][2]), [a13] "v"(A[1][3]), [a20] "v"(A[2][0]), [a21] "v"(A[2][1]),
          [a22] "v"(A[2][2]), [a23] "v"(A[2][3]), [a30] "v"(A[3][0]), [a31] "v"(A[3][1]), [a32] "v"(A[3][2]), [a33] "v"(A[3][3])
        : "scc", "memory");
  }
}
__global__ __launch_bounds__(4 * kThreads) void k_ff2d_table_adj(int nv, const double* __restrict__ f1bar, long npoint,
                                                                  double* __restrict__ parts, size_t slab_doubles) {
  extern __shared__ __align__(16) unsigned char smem[];
  double* T = reinterpret_cast<double*>(smem);
  const int ncell = nv - 1, ntx = (ncell + kTile2 - 1) / kTile2;
  const int cx0 = (blockIdx.y / ntx) * kTile2, cy0 = (blockIdx.y % ntx) * kTile2;
  const int cx1 = cx0 + kTile2 < ncell ? cx0 + kTile2 : ncell, cy1 = cy0 + kTile2 < ncell ? cy0 + kTile2 : ncell;
  const int trow = cx1 - cx0 + 3, tcol = cy1 - cy0 + 3, pitch = tcol | 1;
  const bool whole = ntx == 1;
  for (int i = threadIdx.x; i < trow * pitch; i += blockDim.x) T[i] = 0.0;
  __syncthreads();
  const double dv = 12.0 / nv, v0 = -6.0 + 0.5 * dv, idv = 1.0 / dv;
  // One POINT per wavefront, its lines in rounds of 64 taken from the centre of the tile outwards.  The lines of a point are parallel; a
  // line's chord through the (rectangular) tile shrinks with its distance from the line through the tile's centre, so lines sorted by
  // that distance have nearly equal chords within a round -- the lockstep walk runs as long as the longest chord of its 64 lanes, and
  // with 64 ADJACENT lines per wavefront (the chords of a whole ramp of the trapezoid) 0.63 of the lane-steps did work.
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63, nwv = (int)(blockDim.x >> 6);
  const double Xc = v0 + 0.5 * (cx0 + cx1) * dv, Yc = v0 + 0.5 * (cy0 + cy1) * dv;   // the tile's centre (velocity units)
  for (long pid = (long)blockIdx.x * nwv + wv; pid < npoint; pid += (long)gridDim.x * nwv) {
    const double* fb = f1bar + (size_t)pid * (nv + 2);
    const double cb = fb[nv], sb = fb[nv + 1];
    // the line through the tile's centre: y = -sin X_c + cos Y_c (the lines' perpendicular coordinate); a = first line at or above it
    const double yc = cb * Yc - sb * Xc;
    int a = (int)ceil((yc - v0) * idv);
    a = a < 0 ? 0 : (a > nv ? nv : a);
    const int mside = a < nv - a ? a : nv - a;   // lines available on BOTH sides of the centre
    const bool fwd = cb >= 0.0;
    const bool up = (fwd ? sb : -sb) >= 0.0;   // (uniform over the point)
    for (int r = 0; r < (nv + 63) / 64; ++r) {
      const int j = 64 * r + ln;   // rank of this lane's line in the centre-out order
      int iy;
      if (j < 2 * mside) iy = (j & 1) ? a - 1 - (j >> 1) : a + (j >> 1);
      else iy = a > nv - a ? a - 1 - (j - mside) : a + (j - mside);
      const bool act = j < nv;
      int ix0 = 0, ix1 = nv;
      const double y = __builtin_fma((double)iy, dv, v0), val = act ? fb[iy] * dv : 0.0;
      if (!whole) {
        line_range(cb, (cb * v0 - y * sb - v0) * idv, (double)cx0, (double)cx1, cx0 == 0, cx1 == ncell, ix0, ix1);
        line_range(sb, (sb * v0 + y * cb - v0) * idv, (double)cy0, (double)cy1, cy0 == 0, cy1 == ncell, ix0, ix1);
      }
      if (!act) ix1 = ix0;
      double ul, vl;
      line_origin(cb, sb, y, v0, idv, ul, vl);
      if (whole) {
        if (up) scatter_line_lockstep<1, true>(T, pitch, nv, cx0, cx1, cy0, cy1, fwd, ix0, ix1, cb, sb, ul, vl, val);
        else scatter_line_lockstep<-1, true>(T, pitch, nv, cx0, cx1, cy0, cy1, fwd, ix0, ix1, cb, sb, ul, vl, val);
      } else {
        if (up) scatter_line_lockstep<1, false>(T, pitch, nv, cx0, cx1, cy0, cy1, fwd, ix0, ix1, cb, sb, ul, vl, val);
        else scatter_line_lockstep<-1, false>(T, pitch, nv, cx0, cx1, cy0, cy1, fwd, ix0, ix1, cb, sb, ul, vl, val);
      }
    }
  }
  __syncthreads();
  // the workgroup's partial tile goes to its own slab (plain coalesced stores); k_ff2d_sum_tiles adds the slabs of a tile
  // (hundreds of workgroups adding into the same 17 000 addresses by global atomics is exactly what LDS was used to avoid)
  double* slab = parts + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * slab_doubles;
  for (int i = threadIdx.x; i < trow * tcol; i += blockDim.x) slab[i] = T[(i / tcol) * pitch + i % tcol];
}

// Fbar_pad[tile entries] += sum over the workgroups of tile `tile` of their slabs (fixed order); grid (entries / 256)
__global__ __launch_bounds__(kThreads) void k_ff2d_sum_tiles(int nv, const double* __restrict__ parts, int per_tile,
                                                              size_t slab_doubles, double* __restrict__ Fbar_pad, int tile) {
  const int ncell = nv - 1, ntx = (ncell + kTile2 - 1) / kTile2;
  const int cx0 = (tile / ntx) * kTile2, cy0 = (tile % ntx) * kTile2;
  const int cx1 = cx0 + kTile2 < ncell ? cx0 + kTile2 : ncell, cy1 = cy0 + kTile2 < ncell ? cy0 + kTile2 : ncell;
  const int trow = cx1 - cx0 + 3, tcol = cy1 - cy0 + 3;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= trow * tcol) return;
  const double* p = parts + (size_t)tile * per_tile * slab_doubles + i;
  double acc = 0.0;
  for (int w = 0; w < per_tile; ++w) acc += p[(size_t)w * slab_doubles];
  double* o = Fbar_pad + (size_t)(cx0 + i / tcol) * (nv + 2) + (cy0 + i % tcol);
  *o += acc;   // (the halos of neighbouring tiles overlap by three entries: the host launches the tiles one after another)
}

// adjoint of the ghost cells (ghost_cols was applied last, so it is reversed first), then the interior is copied out
__global__ __launch_bounds__(kThreads) void k_ff2d_fold_ghosts(int nv, double* __restrict__ P, double* __restrict__ out) {
  const int pitch = nv + 2;
  for (int r = threadIdx.x; r < nv + 2; r += kThreads) {
    double* row = P + (size_t)r * pitch;
    row[1] += 2.0 * row[0]; row[2] -= row[0];
    row[nv] += 2.0 * row[nv + 1]; row[nv - 1] -= row[nv + 1];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < nv; c += kThreads) {
    P[pitch + c + 1] += 2.0 * P[c + 1]; P[2 * pitch + c + 1] -= P[c + 1];
    P[(size_t)nv * pitch + c + 1] += 2.0 * P[(size_t)(nv + 1) * pitch + c + 1];
    P[(size_t)(nv - 1) * pitch + c + 1] -= P[(size_t)(nv + 1) * pitch + c + 1];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nv * nv; i += kThreads) out[i] = P[(size_t)(i / nv + 1) * pitch + (i % nv + 1)];
}

// LBacc[b][g][NLB] -> gphys[b][NP]: make_lines_adjoint per gradient point, summed (one thread per lineout)
template <int NI>
__global__ void k_ff2d_lines_adj(KStatic S, const double* __restrict__ phys, int f, int B, const double* __restrict__ LBacc,
                                 double* __restrict__ gphys, int with_m) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  constexpr int NPk = TSFF_NP(NI);
  const int NLB = kNLB2 + 3 * NI + (with_m ? 1 : 0);   // (the 1-D path carries one more slot: the DLM-order tangent)
  Phys<NI> p;
  load_phys<NI>(phys + (size_t)b * S.NP, S.p_scale, S.p_shift, S.p_sig, S.ti_same, false, p);
  double pb[NPk];
#pragma unroll
  for (int s = 0; s < NPk; ++s) pb[s] = 0.0;
  for (int g = 0; g < S.G; ++g) {
    LineS<NI> L, LB;
    make_lines<NI>(p, S.lam_shift[f], g, S.G, L);
    zero_lines<NI>(LB);
    lines_adj_load<NI>(LBacc + ((size_t)b * S.G + g) * NLB, with_m, LB);
    make_lines_adjoint<NI>(p, S.lam_shift[f], g, S.G, L, LB, pb);
  }
  // One species: fr cancels out of fr / Zbar, the only way it enters, so the derivative is identically zero; frb and Zbarb * Z
  // are the same number with opposite signs and what their sum leaves behind (1e-16 of either) is rounding, not a gradient.
  if (NI == 1) pb[TSFF_P_ION0 + TSFF_ION_FRACT] = 0.0;
#pragma unroll
  for (int s = 0; s < NPk; ++s) gphys[(size_t)b * NPk + s] = pb[s];
}
