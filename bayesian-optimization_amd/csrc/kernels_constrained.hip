// kernels_constrained.hip -- feasibility-weighted criteria of an m-target model over one correlation chunk (gfx950).
//
// The reference accepts the values of expensive constraints and drops them (base.py:328, mobo.py:117-118).  Here target 0 of a
// multi-target model is the objective and targets 1 .. m - 1 are the constraints, feasible in [lo_k, hi_k]; per candidate row
//   mu_k, MSE_k   multi_target_moments (bogp_device.h): k_ehvi's expressions in k_ehvi's order, the same bits
//   P             = prod_{k = 1 .. m-1} feasibility(mu_k, MSE_k, sigma2_k, lo_k, hi_k), in this order from 1.0
//   value_c       = base_c P,  base_c = acq_value(id_c, par_c, +-mu_0, sqrt(MSE_0), plugin, sigma2_0) as k_acquisition forms it, or 1 for
//                   BOGP_ACQ_NONE (the probability of feasibility alone, Gelbart et al. 2014)
// and np.argmax over the rows per criterion (first maximum, NaN maximal) into k_acquisition's record layout [q][nblk_total], which
// k_argmax_final / the top-k passes read.  |L^-1 r|^2 from k_contract is shared by every target: the constraints cost the m fmas a
// load of the chunk's column, and the kernel is one coalesced read of 8 N bytes a row: HBM bound (eight loads a lane in flight).
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int MT>
__global__ __launch_bounds__(256) void k_constrained(ConstrainedArgs a) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // row inside the chunk
  const bool valid = i < a.mcount;
  const int64_t g = a.m0 + i;
  double y_hat = 0.0, sd = 0.0, P = 1.0;
  if (valid) {
    double mu[MT], mse[MT];  // (bogp_device.h: shared with k_ehvi and k_ehvi_constrained)
    multi_target_moments<MT, 8>(a, i, mu, mse);
    store_moments<MT>(a.mu_out, a.mse_out, g, mu, mse);
    y_hat = a.minimize ? mu[0] : -1 * mu[0];
    sd = sqrt(mse[0]);
#pragma unroll
    for (int k = 1; k < MT; ++k) P *= feasibility(mu[k], mse[k], a.sigma2[k], a.lo[k], a.hi[k]);
    if (a.pof_out) a.pof_out[g] = P;
  }
  for (int c = 0; c < a.q; ++c) {
    double v = -INFINITY;
    int64_t idx = INT64_MAX;
    if (valid) {
      const double base = a.acq_id[c] == BOGP_ACQ_NONE ? 1.0 : acq_value(a.acq_id[c], a.acq_par[c], y_hat, sd, a.plugin, a.sigma2[0]);
      v = base * P;
      idx = g;
      a.acq_out[(size_t)c * a.M + g] = v;
    }
    const ArgMax best = block_argmax(v, idx, sv, si);
    if (threadIdx.x == 0) {
      a.blk_val[(size_t)c * a.nblk_total + a.blk_offset + blockIdx.x] = best.v;
      a.blk_idx[(size_t)c * a.nblk_total + a.blk_offset + blockIdx.x] = best.i;
    }
    __syncthreads();
  }
}

hipError_t launch_constrained(const ConstrainedArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 255) / 256);
  switch (a.m) {
    case 2: hipLaunchKernelGGL(k_constrained<2>, dim3(nblk), 256, 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_constrained<3>, dim3(nblk), 256, 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_constrained<4>, dim3(nblk), 256, 0, st, a); break;
    case 5: hipLaunchKernelGGL(k_constrained<5>, dim3(nblk), 256, 0, st, a); break;
    case 6: hipLaunchKernelGGL(k_constrained<6>, dim3(nblk), 256, 0, st, a); break;
    case 7: hipLaunchKernelGGL(k_constrained<7>, dim3(nblk), 256, 0, st, a); break;
    case 8: hipLaunchKernelGGL(k_constrained<8>, dim3(nblk), 256, 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
