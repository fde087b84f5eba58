// k_adam.inc -- one Adam step of tsff_adam_fit on the packed buffer of tsff_loss_grad_packed (the reference's _1d_adam_loop_,
// inverse/loops.py:59-95: optax.adam's update, eqx.apply_updates and the best-loss tracking), so that a whole fit is enqueued
// at once.
//
// Bit contract: every operation is the one tsadar_amd.tree.Adam.update + apply_updates does in NumPy, in the same order and in
// double, with nothing fused:
//   mu  = b1 * m + (1 - b1) * g
//   nu  = b2 * v + ((1 - b2) * g) * g
//   upd = ((-lr) * (mu / c1)) / (sqrt(nu / c2) + eps)
//   x   = x + upd
// The host passes 1 - b1, 1 - b2, -lr, c1 = 1 - b1**count and c2 = 1 - b2**count as it computes them (glibc pow, the one
// Python's ** calls), so no device pow enters the bits.  Division and sqrt are the correctly rounded IEEE operations, and the
// pragma keeps the compiler from contracting a multiply and an add into an FMA (HIP's default -ffp-contract would).
//
// Best tracking (loops.py:88-93): L = (w0 S0 + w1 S1) + w2 S2 of THIS step's packed sums; if L < best (false for NaN) the best
// loss becomes L and the best parameters take this step's UPDATED iterate -- the reference stores diff_params after
// apply_updates, i.e. the iterate one step past the one whose loss was measured; kept as it is.  Every workgroup decides on the
// previous best, read from best_prev; workgroup 0 publishes the new one to best_next, a different scalar (the caller alternates
// the two by step parity), so no workgroup can read a value another one of the same launch writes.  Only the active slots of
// best_x change; best_loss_out (the last step only) receives the final best loss.

// The update of one element (also k_ang_opt's, k_angular.inc): the moments in place, the step returned.  The pragma is each
// helper's own -- its scope is the compound statement it appears in, so a calling kernel's does not reach an inlined callee.
__device__ __forceinline__ double adam_update(double g, double& m, double& v, double b1, double omb1, double b2, double omb2,
                                              double neg_lr, double c1, double c2, double eps) {
#pragma clang fp contract(off)
  m = b1 * m + omb1 * g;
  v = b2 * v + (omb2 * g) * g;
  return (neg_lr * (m / c1)) / (sqrt(v / c2) + eps);
}
// tree.RMSProp.update, under the same contract: nu = decay * v + ((1 - decay) * g) * g, upd = ((-lr) * g) / sqrt(nu + eps)
__device__ __forceinline__ double rmsprop_update(double g, double& v, double decay, double omd, double neg_lr, double eps) {
#pragma clang fp contract(off)
  v = decay * v + (omd * g) * g;
  return (neg_lr * g) / sqrt(v + eps);
}

__global__ __launch_bounds__(kThreads) void k_adam_step(const double* __restrict__ packed, double w0, double w1, double w2,
                                                         const int* __restrict__ act, int n_act, int B, int NP,
                                                         double* __restrict__ params, double* __restrict__ mu, double* __restrict__ nu,
                                                         double b1, double omb1, double b2, double omb2, double neg_lr, double c1,
                                                         double c2, double eps, double* __restrict__ loss_hist,
                                                         const double* __restrict__ best_prev, double* __restrict__ best_next,
                                                         double* __restrict__ best_loss_out, double* __restrict__ best_x) {
#pragma clang fp contract(off)
  const double L = (w0 * packed[0] + w1 * packed[1]) + w2 * packed[2];
  const double prev = *best_prev;
  const bool improve = L < prev;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (loss_hist) *loss_hist = L;
    const double nb = improve ? L : prev;
    *best_next = nb;
    if (best_loss_out) *best_loss_out = nb;
  }
  const long n = (long)n_act * B;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const long k = i / B, b = i - k * B;
    double m = mu[i], v = nu[i];
    const double upd = adam_update(packed[3 + i], m, v, b1, omb1, b2, omb2, neg_lr, c1, c2, eps);
    const long o = b * NP + act[k];
    const double x = params[o] + upd;
    mu[i] = m;
    nu[i] = v;
    params[o] = x;
    if (improve) best_x[o] = x;
  }
}
