// kernels_ehvi.hip -- expected hypervolume improvement of an m-target model over one correlation chunk (gfx950).
//
// Replaces, per candidate row, the reference's EHVI.forward (multi_objective/analytic.py:176-274) on the posterior of
// GaussianProcess.predict (gpr.py:486-510) with several targets:
//   mu_k  = beta + r.gamma_k                       (the chunk's r column; gamma_k the target's column of gamma_base)
//   MSE_k = max(0, (1 - |L^-1 r|^2 + u^2) sigma2_k) (|L^-1 r|^2 from k_contract, shared by every target)
//   sigma_k = sqrt(max(MSE_k, 1e-9))              (analytic.py:233)
// and, for the cells (l_c, u_c) of a partition of the region the front does not dominate (maximised targets),
//   EHVI = sum_c prod_k f_ck,  f_ck = psi(l,l) - psi(l,u) + nu(l,u) = E[(min(Y_k, u_ck) - l_ck)^+]
//        = sigma_k (G(a) - G(b)),  a = (l - mu) / sigma, b = (u - mu) / sigma,  G(z) = phi(z) - z Phi(-z)
// -- the reference's sum over the 2^m subsets of {psi_diff, nu} is the expansion of this product.  An upper bound at
// +inf gives G(b) = 0 exactly (the reference clamps it to 1e10, where its terms vanish).  np.argmax order over the rows
// (first maximum, NaN maximal) into the same per-block records k_argmax_final / the top-k passes read.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int MT>
__global__ __launch_bounds__(256) void k_ehvi(EhviArgs a) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // row inside the chunk
  const bool valid = i < a.mcount;
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    double mu[MT], mse[MT];  // (bogp_device.h: shared with k_constrained and k_ehvi_constrained)
    multi_target_moments<MT>(a, i, mu, mse);
    const int64_t g = a.m0 + i;
    store_moments<MT>(a.mu_out, a.mse_out, g, mu, mse);
    double sd[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) sd[k] = sqrt(fmax(mse[k], 1e-9));
    v = ehvi_cells<MT>(a.lower, a.upper, a.C, mu, sd);  // (bogp_device.h: shared with k_ehvi_constrained, k_believer_ehvi and k_forest_ehvi)
    idx = g;
    a.ehvi_out[g] = v;
  }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (threadIdx.x == 0) {
    a.blk_val[a.blk_offset + blockIdx.x] = best.v;
    a.blk_idx[a.blk_offset + blockIdx.x] = best.i;
  }
}

hipError_t launch_ehvi(const EhviArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 255) / 256);
  switch (a.m) {
    case 2: hipLaunchKernelGGL(k_ehvi<2>, dim3(nblk), 256, 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_ehvi<3>, dim3(nblk), 256, 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_ehvi<4>, dim3(nblk), 256, 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_ehvi<5>, dim3(nblk), 256, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_ehvi<6>, dim3(nblk), 256, 0, st, a); break;
    case 7: hipLaunchKernelGGL(k_ehvi<7>, dim3(nblk), 256, 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_ehvi<8>, dim3(nblk), 256, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
