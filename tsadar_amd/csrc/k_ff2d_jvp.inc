// k_ff2d_jvp.inc -- forward mode of the 2-D form factor (tsff_form_factor_2d_jvp): k_ff2d_project, k_ff2d_jvp.  Part of the single
// translation unit tsff_kernels.hip (included inside namespace tsff, after k_ffjvp.inc).  DESIGN.md section 4.4c.2.
//
// P_dot[d] = dP/dphys . phys_dot[d] + dP/dfe2d . fe2d_dot[d] for ONE shared table, nv <= 256, in three stages:
//   a. the saving forward (k_form_factor_2d<.., SAVE>), unchanged: P and, per point, the projection f1[nv] and the per-thread sums of
//      d sample / d cos(beta), d sample / d sin(beta) (proj2d_doubles(nv) doubles);
//   b. k_ff2d_project, once per table direction: the projection alone -- the forward's shared steps up to column_sums_2d -- applied
//      to the tangent table.  The projection is linear in the table, the ghost cells are linear extrapolations (the padded tangent
//      table is the tangent of the padded table) and the rotated sample positions are stage a's (the same point_setup_2d: the same
//      bits), so its output IS the table part of the projection's tangent;
//   c. k_ff2d_jvp, the tail: W directions per launch on TN<W> -- lineout scalars (make_lines_hd), point scalars, the projection's
//      tangent from the records, ratintn, the two lookups at |xi_e|, the ion sums (point_hd's) and the assembly.
// Every branch and cell index is decided by the value; no atomics; every sum has a fixed order that does not depend on the grid.
//
// Table convention: that of k_fwdmode.inc for the ion terms (Z' carries its slope and no curvature, the asymptote and exp(-xi^2)
// exactly); the two linear lookups at |xi_e| carry their cell's slope where the position is not clamped and none where it is
// (jnp.interp); the half-plane term of beta carries no tangent.

// The ion sums of a point at phase velocity vph = w_d / k: chi_i = sum_s hai_s ik^2 Z'(xi_s) added to opc (real part) and cim
// (imaginary part), and sum_s cs_s exp(-xi_s^2) / sqrt(2 pi) added to gsum.  zp: the full Z' table.  This IS the species loop of
// point_hd (k_fwdmode.inc), written a second time: factored out of point_hd into a function both callers use, six instantiations of
// k_jac_sweep and k_hess_pairs changed their register allocation (AGPR counts; profiles/ff2d_jvp_resources.txt), so point_hd stays
// as it is.
template <int NI, class N>
__device__ __forceinline__ void ion_sums_2d_hd(const N& vph, const N& ik2, const LineT<N, NI>& L, const double2* zp, N& opc, N& cim, N& gsum) {
#pragma unroll
  for (int s = 0; s < NI; ++s) {
    const N xi = vph * L.ixi[s];
    const N hk = L.hai[s] * ik2;
    // Z'(xi): the full table (slope, no curvature) or the asymptote xi^-2 + 0 i outside it
    constexpr double kTop = (double)(kNXi2 - 1) * (1.0 - 1.1102230246251565e-16);
    const double u = __builtin_fma(xi.v, kXi2_ih, -kXi2_0 * kXi2_ih);
    const double uc = fmin(fmax(u, 0.0), kTop);
    N zr, zi;
    if (u != uc) {
      const double r = 1.0 / xi.v, r2 = r * r;
      zr = hd_chain(xi, r2, -2.0 * r2 * r, 6.0 * r2 * r2);
      zi = N::of(0.0);
    } else {
      const double fl = __builtin_floor(uc);
      const double t = uc - fl;
      const int i = (int)fl;
      const double2 za = zp[i], zb = zp[i + 1];
      const double dr = zb.x - za.x, di = zb.y - za.y;
      zr = hd_chain(xi, __builtin_fma(t, dr, za.x), dr * kXi2_ih, 0.0);
      zi = hd_chain(xi, __builtin_fma(t, di, za.y), di * kXi2_ih, 0.0);
    }
    const N gs = hd_exp(-(xi * xi)) * kInvSqrt2Pi;
    opc = opc + hk * zr;
    cim = cim + hk * zi;
    gsum = gsum + L.cs[s] * gs;
  }
}

// flags[d] = 1 when the tangent table of direction d has a non-zero entry, else 0: a direction without a table tangent (a scalar leaf
// among generator leaves) skips its projection and takes the arithmetic of a call without table directions.  One workgroup per
// direction; the host never looks at the flags.
__global__ __launch_bounds__(kThreads) void k_ff2d_tabflags(const double* __restrict__ fe2d_dot, int nv, int* __restrict__ flags) {
  const double* __restrict__ t = fe2d_dot + (size_t)blockIdx.x * nv * nv;
  int any = 0;
  for (int i = threadIdx.x; i < nv * nv; i += kThreads) any |= t[i] != 0.0;
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) flags[blockIdx.x] = any != 0;
}

// b. the projection of a (tangent) table for the points [pbegin, pend): f1tab[point - pbegin][nv].  The workgroup, the LDS layout
// and the barrier sequence are k_form_factor_2d's up to the column sums; F: see there (the plain table, or the padded copy of k_pad2d).
template <int NI, bool LDS, int kG2>
__global__ __launch_bounds__(kG2 * kThreads, TSFF_2D_WAVES) void k_ff2d_project(KStatic S, const double* __restrict__ phys,
                                                                 const double* __restrict__ Fg, int nv, double ud_ang,
                                                                 double va_ang, int f, long pbegin, long pend,
                                                                 double* __restrict__ f1tab, const int* __restrict__ flag) {
  if (*flag == 0) return;   // (no table tangent along this direction: uniform over the grid)
  extern __shared__ __align__(16) unsigned char smem[];
  const int grp = threadIdx.x >> 8, gt = threadIdx.x & (kThreads - 1);
  const int nvp = nvp2d(nv), nparts = parts2d(nv);
  double* gbase = reinterpret_cast<double*>(smem) + (size_t)grp * group2d_doubles(nv);
  double* f1 = gbase;                    // [nv]
  double* part = f1 + 2 * nv;            // [nparts][nv] partial column sums
  double* sc = part + nparts * nv + 8;   // [kSc2] point scalars
  double* Fl = reinterpret_cast<double*>(smem) + (size_t)kG2 * group2d_doubles(nv);
  const double dv = 12.0 / nv, v0 = -6.0 + 0.5 * dv, idv = 1.0 / dv;
  const int pitch = pitch2d(nv, LDS);
  if (LDS) stage_table_2d(Fg, Fl, nv, pitch, kG2 * kThreads);
  const double* __restrict__ F = LDS ? Fl : Fg;
  const long stride = (long)gridDim.x * kG2;
  for (long base = pbegin + (long)blockIdx.x * kG2; base < pend; base += stride) {
    const long pid = base + grp;
    const bool active = pid < pend;
    __syncthreads();
    if (active && gt == 0) point_setup_2d<NI, false>(S, phys, f, point_id_2d(pid, S), ud_ang, va_ang, sc);
    __syncthreads();
    const double cb = sc[SC_CB], sb = sc[SC_SB];
    if (active) {
      double ds1 = 0.0, ds2 = 0.0;
      project_point_2d<LDS, false>(F, nv, pitch, nvp, nparts, cb, sb, dv, v0, idv, gt, part, ds1, ds2);
    }
    __syncthreads();
    if (active) column_sums_2d(part, nv, nparts, dv, gt, f1, f1tab + (size_t)(pid - pbegin) * nv);
  }
}

// one launch of k_ff2d_jvp, passed by value
struct Ff2dJvpArgs {
  int d0, nd;              // this launch: directions [d0, d0 + nd) of the call's n_dir, nd <= W
  int B, nv, feature;
  long pbegin, pend;       // the points of the call; the records and f1tab are indexed by point - pbegin
  double ud_ang, va_ang;   // radians
  const double* phys;      // [B][NP]
  const double* phys_dot;  // [n_dir][B][NP]
  const double* proj;      // the saving forward's records
  const double* f1tab;     // [nd][pend - pbegin][nv] the projections of this launch's table directions, or nullptr (none)
  const int* tabflags;     // f1tab: [nd] which of them have a table tangent at all (k_ff2d_tabflags)
  double* P_dot;           // [n_dir][B][G][npts][NA]
};
constexpr int kFf2dJvpThreads = 64;
// dynamic LDS of a k_ff2d_jvp workgroup: f1 and its W tangents
__host__ __device__ inline size_t ff2d_jvp_smem_doubles(int nv, int W) { return (size_t)(1 + W) * nv; }

// c. the tail.  One WAVEFRONT per point (a workgroup is one wavefront): the work of a point is a stream over its record -- nv (1 + 2
// parts2d) doubles -- with (nv - 2) / 64 <= 4 intervals of ratintn per lane, and a scalar chain that every lane evaluates (uniform
// values, so it costs one lane's time); a 256-thread group would leave three wavefronts idle through that chain and pay six barriers
// per point for sums a wavefront takes in registers.  A workgroup owns a CONTIGUOUS run of points, so that the lineout scalars
// (make_lines_hd, in LDS) are made once per (lineout, gradient point) of its run; a point's result does not depend on the run it is in.
template <int NI, int W>
__global__ __launch_bounds__(kFf2dJvpThreads) void k_ff2d_jvp(KStatic S, Ff2dJvpArgs A) {
  using N = TN<W>;
  constexpr int NPk = TSFF_NP(NI);
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ N ph[kNP_MAX + 1];
  __shared__ LineT<N, NI> Lsh;
  const int nv = A.nv, lane = threadIdx.x, f = A.feature, B = A.B;
  double* f1 = reinterpret_cast<double*>(smem);   // [nv] the projection
  double* f1d = f1 + nv;                          // [W][nv] its tangents
  const int nparts = parts2d(nv);
  const double dv = 12.0 / nv, v0 = -6.0 + 0.5 * dv, idv = 1.0 / dv;
  const double cva = cos(A.va_ang), sva = sin(A.va_ang), cud = cos(A.ud_ang), sud = sin(A.ud_ang);
  const long npoint = A.pend - A.pbegin;
  const long run = (npoint + gridDim.x - 1) / gridDim.x;
  const long lo = A.pbegin + (long)blockIdx.x * run, hi = lo + run < A.pend ? lo + run : A.pend;
  const size_t dstride = (size_t)B * S.G * S.npts * S.n_angles;   // one direction of P_dot
  // d/dx of the uniform gradient of an array in LDS: one-sided at the ends (gradient_2d)
  auto grad_at = [&](const double* a, int i) {
    if (i == 0) return (a[1] - a[0]) * idv;
    if (i == nv - 1) return (a[nv - 1] - a[nv - 2]) * idv;
    return (a[i + 1] - a[i - 1]) * (0.5 * idv);
  };
  bool tab[W];   // lane k carries a table tangent
#pragma unroll
  for (int k = 0; k < W; ++k) tab[k] = A.f1tab && k < A.nd && A.tabflags[k] != 0;
  int cur_b = -1, cur_g = -1;
  for (long pid = lo; pid < hi; ++pid) {
    const PointId2D id = point_id_2d(pid, S);
    __syncthreads();   // (every reader of the previous point's arrays and scalars is done)
    if (id.b != cur_b) {
      // ---- the physical parameters with the group's seeds (load_phys without activation: Ti tying only) ----
      if (lane == 0) {
        const double* __restrict__ xpar = A.phys + (size_t)id.b * S.NP;
        for (int s = 0; s < NPk; ++s) {
          N v = N::of(xpar[s]);
#pragma unroll
          for (int k = 0; k < W; ++k)
            if (k < A.nd) v.d[k] = A.phys_dot[((size_t)(A.d0 + k) * B + id.b) * S.NP + s];
          ph[s] = v;
        }
        for (int s = 1; s < NI; ++s)
          if (S.ti_same[s]) ph[TSFF_P_ION0 + 4 * s + TSFF_ION_TI] = ph[TSFF_P_ION0 + TSFF_ION_TI];
      }
      cur_b = id.b; cur_g = -1;
    }
    if (id.g != cur_g) {
      if (lane == 0) make_lines_hd<NI>(ph, S.lam_shift[f], id.g, S.G, Lsh);
      cur_g = id.g;
    }
    __syncthreads();
    const LineT<N, NI>& L = Lsh;
    // ---- point scalars (point_scalars_2d over N) ----
    const double ws = S.omgs[f][id.j], th = S.sa_rad[id.a];
    const double ct = cos(th), st = sin(th);
    const N ks = hd_sqrt(ws * ws - L.wpe2) * (1.0 / kC);
    const N kx = ct * ks - L.kL, ky = st * ks;
    const N k2 = kx * kx + ky * ky;
    const N ik2 = hd_rcp(k2);
    const N wd = (ws - L.wL) - (kx * (L.Vd * cva) + ky * (L.Vd * sva));
    const N aa = wd * ik2;
    const N xex = (aa * kx - L.Ud * cud) * L.ivTe, xey = (aa * ky - L.Ud * sud) * L.ivTe;
    const N xm2 = xex * xex + xey * xey;
    const N xmag = hd_sqrt(xm2);
    const double beta = atan(xey.v / xex.v) + (xex.v >= 0.0 ? 0.0 : kPi);   // (the half plane carries no tangent)
    const double cb = cos(beta), sb = sin(beta);
    double bd[W];   // the rotation's tangent: (xex d xey - xey d xex) / |xi_e|^2
#pragma unroll
    for (int k = 0; k < W; ++k) bd[k] = (xex.v * xey.d[k] - xey.v * xex.d[k]) / xm2.v;
    // ---- the projection and its tangents: dv beta' sum_part (-sin beta ds1 + cos beta ds2) + the tangent table's projection ----
    {
#pragma clang fp contract(off)   // (the rotation term has the same bits with and without a table term behind it)
      const double* __restrict__ rec = proj2d_record(A.proj, pid - A.pbegin, nv);
      for (int i = lane; i < nv; i += kFf2dJvpThreads) {
        f1[i] = rec[i];
        double rs = 0.0;
        for (int q = 0; q < nparts; ++q) rs += cb * rec[nv + (nparts + q) * nv + i] - sb * rec[nv + q * nv + i];
#pragma unroll
        for (int k = 0; k < W; ++k) {
          double r = (dv * bd[k]) * rs;
          if (tab[k]) r += A.f1tab[((size_t)k * npoint + (size_t)(pid - A.pbegin)) * nv + i];
          f1d[k * nv + i] = k < A.nd ? r : 0.0;
        }
      }
    }
    __syncthreads();
    // ---- ratintn(d1, vx - |xi_e|, vx) over the nv - 2 intervals: each interval's formula in the branch the value takes, with its
    //      partial derivatives w.r.t. d1[i], d1[i + 1] and (through g = vx - |xi_e|) |xi_e| ----
    double R = 0.0, Rd[W];
#pragma unroll
    for (int k = 0; k < W; ++k) Rd[k] = 0.0;
    for (int i = lane; i < nv - 2; i += kFf2dJvpThreads) {
      const double f0 = grad_at(f1, i), f1v = grad_at(f1, i + 1);
      const double g0 = (v0 + i * dv) - xmag.v, g1 = (v0 + (i + 1) * dv) - xmag.v;
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
      R += r * dv;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double a0 = grad_at(f1d + k * nv, i), a1 = grad_at(f1d + k * nv, i + 1);
        Rd[k] += (rfd * (a1 - a0) + rfa * (0.5 * (a1 + a0)) - rga * xmag.d[k]) * dv;   // (d gav = -d |xi_e|)
      }
    }
    N Rn;
    Rn.v = wave_sum(R);
#pragma unroll
    for (int k = 0; k < W; ++k) Rn.d[k] = wave_sum(Rd[k]);
    // ---- the two lookups at |xi_e| (jnp.interp: clamped to the end values, no slope there) ----
    N fev, dfe;
    {
      const double u = (xmag.v - v0) * idv;
      int i = (int)u;
      i = i < 0 ? 0 : (i > nv - 2 ? nv - 2 : i);
      double t = (xmag.v - (v0 + i * dv)) * idv;
      const bool tin = t >= 0.0 && t <= 1.0;
      t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
      const double fa = f1[i], fb = f1[i + 1], da = grad_at(f1, i), db = grad_at(f1, i + 1);
      const double sf = tin ? (fb - fa) * idv : 0.0, sd = tin ? (db - da) * idv : 0.0;
      fev.v = fa + t * (fb - fa);
      dfe.v = da + t * (db - da);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double* fk = f1d + k * nv;
        const double ta = fk[i], tb = fk[i + 1], ga = grad_at(fk, i), gb = grad_at(fk, i + 1);
        fev.d[k] = ta + t * (tb - ta) + sf * xmag.d[k];
        dfe.d[k] = ga + t * (gb - ga) + sd * xmag.d[k];
      }
    }
    // ---- ion sums, assembly and the final factor (assemble_point_2d and the last line of k_form_factor_2d, over N) ----
    const N ik = hd_rcp(hd_sqrt(k2));
    const N vph = wd * ik;
    const N ike2 = L.a_e * ik2;
    N opc = N::of(1.0), cim = N::of(0.0), gsum = N::of(0.0);
    ion_sums_2d_hd<NI>(vph, ik2, L, S.zpf, opc, cim, gsum);
    const N cer = -(ike2 * Rn);
    const N cei = (kPi * ike2) * dfe;
    const N er = opc + cer, ei = cei + cim;
    const N eps2 = er * er + ei * ei;
    const N ce2 = cer * cer + cei * cei;
    const N ci2 = opc * opc + cim * cim;
    const N Nn = gsum * ce2 + ci2 * fev * L.ivTe;
    const N Sv = Nn * ik / eps2;
    const N v = Sv * (1.0 + wd * L.i2wL) * L.pref * (ws * ws);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (k < A.nd) A.P_dot[(size_t)(A.d0 + k) * dstride + (size_t)pid] = v.d[k];
    }
  }
}
