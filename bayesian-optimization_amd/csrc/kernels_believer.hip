// kernels_believer.hip -- one Kriging-believer pass over a chunk of candidates (gfx950).
//
// Believing a point p (Ginsbourger et al. 2010: y = mu(p) at fixed hyper-parameters) leaves the posterior mean of gpr.py:490 as it is and
// takes a rank-one term off the bracket of gpr.py:502-510.  Per candidate row x of the chunk:
//   b(x) = k(x, p) - r(x) . a + u(x) u(p) - sum_k c_k(x) c_k(p),   a = R^-1 r(p),  u = (w . r - 1) / G (ordinary kriging, else 0)
//   c(x) = b(x) / sqrt(pivot),   s(x) <- s(x) - sigma2 c(x)^2     (exactly 0 on the candidate row that IS p)
// and, when the pass stands in front of a step, that step's criterion on (mu, max(0, s)) with the argmax records of k_acquisition's kind
// over the rows that are not winners yet.
// r(x) is the producer's chunk (n-major: lane = candidate, so every load of the dot is coalesced); k(x, p) comes straight from the
// candidate row with the arithmetic of k_batch_corr.  HBM-bound: 8 N bytes per candidate, no MFMA.
// A workgroup serves 64 candidates; its four waves take the quarters of n (a function of N only) and each lane sums its quarter in
// ascending n, the quarters are added in a fixed order: the bits do not depend on the chunk size.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int KERNEL>
__global__ __launch_bounds__(256) void k_believer(BelieverArgs a) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;  // row inside the chunk
  const bool valid = i < a.mcount;
  if (a.update) {
    const int nq = (a.N + 3) / 4;
    const int n0 = wv * nq, n1 = min(a.N, n0 + nq);
    double acc = 0.0;
    if (valid) {
      const double* col = a.rT + i;
      int n = n0;
      for (; n + 8 <= n1; n += 8) {  // eight loads in flight per lane, one accumulation order
        double r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) r[k] = col[(size_t)(n + k) * a.Mc];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = __builtin_fma(r[k], a.avec[n + k], acc);
      }
      for (; n < n1; ++n) acc = __builtin_fma(col[(size_t)n * a.Mc], a.avec[n], acc);
    }
    part[wv][lane] = acc;
    __syncthreads();
  }
  if (wv != 0) return;  // (no barrier below: the epilogue is one wave's)
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    const int64_t g = a.m0 + i;
    double s = a.s[g];
    if (a.update) {
      const double dot = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
      double s2 = dist_init<KERNEL>();
      const double pexp = kernel_exponent<KERNEL>(a.theta, a.d);
      const double* x = a.Xs + (size_t)g * a.d;
      for (int k = 0; k < a.d; ++k) s2 = dist_fold<KERNEL>(a.theta[k], a.pt[k] - x[k], s2, pexp);
      double b = corr_profile<KERNEL>(s2, pexp) - dot;
      if (a.estimate_trend) {
        double wd = 0.0;
        for (int sl = 0; sl < a.S; ++sl) wd += a.w_part[(size_t)sl * a.Mc + i];
        b = __builtin_fma((wd - 1.0) / a.G, a.u_p, b);
      }
      for (int k = 0; k < a.nprev; ++k) b = __builtin_fma(-a.C[(size_t)a.prev_slot[k] * a.M + g], a.prev_c[k], b);
      const double c = b * a.inv_root;
      if (a.c_out) a.c_out[g] = c;
      s = __builtin_fma(-(a.sigma2 * c), c, s);
      if (g == a.self_row) s = 0.0;  // the believed row itself is determined: c(p)^2 = pivot = s(p) exactly, rounding must not leave sd > 0 there
      a.s[g] = s;
    }
    if (a.eval) {
      double mse = s;
      if (mse < 0.0) mse = 0.0;
      const double mu = a.mu[g];
      const double y_hat = a.minimize ? mu : -1 * mu;
      v = acq_value(a.acq_id, a.acq_par, y_hat, sqrt(mse), a.plugin, a.sigma2);
      idx = g;
      a.acq_out[g] = v;
      a.mse_out[g] = mse;
      // a row that already is a winner does not compete again: on its zero variance EpsilonPI is Phi(+-inf) -- exactly 1 whenever its mean is
      // within epsilon |mean| of the plugin, which it is once that mean has become the plugin -- and UCB is its bare mean
      for (int k = 0; k < a.n_taken; ++k)
        if (a.taken[k] == g) {
          v = -INFINITY;
          idx = INT64_MAX;
        }
    }
  }
  if (!a.eval) return;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = shfl_xor_f64(v, off);
    const int64_t oi = shfl_xor_i64(idx, off);
    if (better(ov, oi, v, idx)) {
      v = ov;
      idx = oi;
    }
  }
  if (lane == 0) {
    a.blk_val[a.blk_offset + blockIdx.x] = v;
    a.blk_idx[a.blk_offset + blockIdx.x] = idx;
  }
}

hipError_t launch_believer(int kernel, const BelieverArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 63) / 64);
#define CALL(K) hipLaunchKernelGGL(k_believer<K>, dim3(nblk), 256, 0, st, a)
  switch (kernel) {
    case BOGP_KERNEL_SE: CALL(BOGP_KERNEL_SE); break;
    case BOGP_KERNEL_MATERN12: CALL(BOGP_KERNEL_MATERN12); break;
    case BOGP_KERNEL_MATERN32: CALL(BOGP_KERNEL_MATERN32); break;
    case BOGP_KERNEL_ABSEXP: CALL(BOGP_KERNEL_ABSEXP); break;
    case BOGP_KERNEL_CUBIC: CALL(BOGP_KERNEL_CUBIC); break;
    case BOGP_KERNEL_GENEXP: CALL(BOGP_KERNEL_GENEXP); break;
    case BOGP_KERNEL_MATERN_NU: CALL(BOGP_KERNEL_MATERN_NU); break;
    default: CALL(BOGP_KERNEL_MATERN52); break;
  }
#undef CALL
  return hipGetLastError();
}

}  // namespace bogp
