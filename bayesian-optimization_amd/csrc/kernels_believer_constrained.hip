// kernels_believer_constrained.hip -- the m-target half of a Kriging-believer pass under modelled constraints: per-target variance
// downdate and one feasibility-weighted criterion (gfx950).
//
// Believing a point p leaves the m posterior means as they are and takes ONE rank-one term off the bracket the targets share
// (gpr.py:502-510: MSE_k = sigma2_k (1 - |L^-1 r|^2 + u^2)).  k_believer (kernels_believer.hip) has formed that term in
// correlation units, c(x) = b(x) / sqrt(pivot), for every candidate; per candidate row this kernel then does
//   MSE_k(x) <- MSE_k(x) - sigma2_k c(x)^2  for the m targets   (exactly 0 on the candidate row that IS p)
// and, when the pass stands in front of a step, that step's criterion in k_constrained's expressions and order: target 0 is the
// objective, targets 1 .. m - 1 are constraints feasible in [lo_k, hi_k],
//   P = prod_{k = 1 .. m-1} feasibility(mu_k, MSE_k, sigma2_k, lo_k, hi_k) from 1.0,  value = base P,
//   base = acq_value(id, par, +-mu_0, sqrt(MSE_0), plugin, sigma2_0) without a floor under the root, or 1 for BOGP_ACQ_NONE
// -- given the same moments, the bytes k_constrained leaves -- with the argmax records of k_believer_ehvi's kind (one per 256 rows)
// over the rows that are not winners yet.
// Elementwise in the global row index: one launch serves all M rows behind the chunk loop, so no bit depends on the chunk size.
// Streams 8 (3 + 4 m) bytes per candidate (c, the value and P out, and per target the running variance in and out, the mean and the
// clamped variance); no MFMA, LDS for the block reduction only.
#include "bogp_believer_multi.h"

namespace bogp {

template <int MT>
__global__ __launch_bounds__(256) void k_believer_constrained(BelieverConstrainedArgs a) {
  const BelieverStep& b = a.step;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;  // candidate row
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (g < b.M) {
    double s[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) s[k] = b.s[(size_t)g * MT + k];
    if (b.update) believer_downdate<MT>(b, g, b.c[g], s);
    if (b.eval) {
      double mu[MT], mse[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        mu[k] = b.mu[(size_t)g * MT + k];
        mse[k] = believer_clamped<MT>(b, g, k, s[k]);
      }
      const double y_hat = a.minimize ? mu[0] : -1 * mu[0];
      const double sd = sqrt(mse[0]);
      double P = 1.0;
#pragma unroll
      for (int k = 1; k < MT; ++k) P *= feasibility(mu[k], mse[k], b.sigma2[k], a.lo[k], a.hi[k]);
      const double base = a.acq_id == BOGP_ACQ_NONE ? 1.0 : acq_value(a.acq_id, a.acq_par, y_hat, sd, a.plugin, b.sigma2[0]);
      v = base * P;
      idx = g;
      a.acq_out[g] = v;
      a.pof_out[g] = P;
    }
  }
  if (!b.eval) return;  // (uniform: no barrier is skipped by part of a workgroup)
  believer_tail(b, g, v, idx);
}

hipError_t launch_believer_constrained(const BelieverConstrainedArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.step.M + 255) / 256);
  switch (a.step.m) {
    case 2: hipLaunchKernelGGL(k_believer_constrained<2>, dim3(nblk), 256, 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_believer_constrained<3>, dim3(nblk), 256, 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_believer_constrained<4>, dim3(nblk), 256, 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_believer_constrained<5>, dim3(nblk), 256, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_believer_constrained<6>, dim3(nblk), 256, 0, st, a); break;
    case 7: hipLaunchKernelGGL(k_believer_constrained<7>, dim3(nblk), 256, 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_believer_constrained<8>, dim3(nblk), 256, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
