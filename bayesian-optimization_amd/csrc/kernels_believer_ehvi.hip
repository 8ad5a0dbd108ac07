// kernels_believer_ehvi.hip -- the m-target half of a Kriging-believer pass: per-target variance downdate and EHVI (gfx950).
//
// Believing a point p leaves the m posterior means as they are and takes ONE rank-one term off the bracket the targets share
// (gpr.py:502-510: MSE_k = sigma2_k (1 - |L^-1 r|^2 + u^2)).  k_believer (kernels_believer.hip) has formed that term in
// correlation units, c(x) = b(x) / sqrt(pivot), for every candidate; per candidate row this kernel then does
//   MSE_k(x) <- MSE_k(x) - sigma2_k c(x)^2  for the m targets   (exactly 0 on the candidate row that IS p)
// and, when the pass stands in front of a step, that step's criterion: sd_k = sqrt(max(MSE_k, 1e-9)) (analytic.py:233) and
// ehvi_cells<MT> over the cells of the step's front -- the expressions k_ehvi evaluates -- with the argmax records of k_ehvi's
// kind over the rows that are not winners yet.
// Elementwise in the global row index: one launch serves all M rows behind the chunk loop, so no bit depends on the chunk size.
// Streams 8 (1 + 3 m) bytes per candidate; no MFMA, LDS for the block reduction only.
// The steps around the criterion are those of bogp_believer_multi.h, written out: through that header's helpers, under either field
// order and either place of the exclusion loop, k_believer_ehvi<7> gains branches (profiles/believer_multi_fold.txt section 7).
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int MT>
__global__ __launch_bounds__(256) void k_believer_ehvi(BelieverEhviArgs a) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;  // candidate row
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (g < a.M) {
    double s[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) s[k] = a.s[(size_t)g * MT + k];
    if (a.update) {
      const double c = a.c[g];
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        s[k] = __builtin_fma(-(a.sigma2[k] * c), c, s[k]);
        if (g == a.self_row) s[k] = 0.0;  // the believed row itself is determined: rounding must not leave sd > 0 there
        a.s[(size_t)g * MT + k] = s[k];
      }
    }
    if (a.eval) {
      double mu[MT], sd[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        double mse = s[k];
        if (mse < 0.0) mse = 0.0;
        mu[k] = a.mu[(size_t)g * MT + k];
        a.mse_out[(size_t)g * MT + k] = mse;
        sd[k] = sqrt(fmax(mse, 1e-9));
      }
      v = ehvi_cells<MT>(a.lower, a.upper, a.C, mu, sd);
      idx = g;
      a.ehvi_out[g] = v;
      // a row that already is a winner keeps its value in the outputs and does not compete again
      for (int k = 0; k < a.n_taken; ++k)
        if (a.taken[k] == g) {
          v = -INFINITY;
          idx = INT64_MAX;
        }
    }
  }
  if (!a.eval) return;  // (uniform: no barrier is skipped by part of a workgroup)
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (threadIdx.x == 0) {
    a.blk_val[blockIdx.x] = best.v;
    a.blk_idx[blockIdx.x] = best.i;
  }
}

hipError_t launch_believer_ehvi(const BelieverEhviArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.M + 255) / 256);
  switch (a.m) {
    case 2: hipLaunchKernelGGL(k_believer_ehvi<2>, dim3(nblk), 256, 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_believer_ehvi<3>, dim3(nblk), 256, 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_believer_ehvi<4>, dim3(nblk), 256, 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_believer_ehvi<5>, dim3(nblk), 256, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_believer_ehvi<6>, dim3(nblk), 256, 0, st, a); break;
    case 7: hipLaunchKernelGGL(k_believer_ehvi<7>, dim3(nblk), 256, 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_believer_ehvi<8>, dim3(nblk), 256, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
