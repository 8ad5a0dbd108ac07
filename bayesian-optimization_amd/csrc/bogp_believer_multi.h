// bogp_believer_multi.h -- the steps of the m-target half of a Kriging-believer pass that do not depend on the criterion, shared by
// k_believer_constrained (kernels_believer_constrained.hip) and k_believer_ehvi_constrained (kernels_believer_ehvi_constrained.hip):
// one thread per candidate row g, 256 rows a workgroup, all on the BelieverStep that their argument blocks hold as `step` (the struct
// is in bogp_internal.h beside those blocks: believer_run, host code, fills it).  k_believer_ehvi (kernels_believer_ehvi.hip) does the
// same steps in its own text on its own fields.  A kernel loads the row's running variances s[MT] (and c(x) under `update`), then
//   1. believer_downdate   s_k <- fma(-(sigma2_k c), c, s_k), exactly 0 on the believed row itself, stored         (under `update`)
//   2. believer_clamped    max(0, s_k) into mse_out, per target: what the step's criterion sees                    (under `eval`)
//   3. its own criterion and value store
//   4. believer_tail       the winners of earlier steps leave the argmax, block_argmax, one record per 256 rows    (every lane)
// with the uniform `if (!step.eval) return;` of the kernel in front of 4, the only barrier.
#pragma once
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

// 1. s and c are the row's values as the kernel loaded them
template <int MT>
__device__ __forceinline__ void believer_downdate(const BelieverStep& b, int64_t g, double c, double (&s)[MT]) {
#pragma unroll
  for (int k = 0; k < MT; ++k) {
    s[k] = __builtin_fma(-(b.sigma2[k] * c), c, s[k]);
    if (g == b.self_row) s[k] = 0.0;  // the believed row itself is determined: rounding must not leave sd > 0 there
    b.s[(size_t)g * MT + k] = s[k];
  }
}

// 2. target k of row g
template <int MT>
__device__ __forceinline__ double believer_clamped(const BelieverStep& b, int64_t g, int k, double s) {
  double mse = s;
  if (mse < 0.0) mse = 0.0;
  b.mse_out[(size_t)g * MT + k] = mse;
  return mse;
}

// 4. (v, idx) is the row's value and g, or (-inf, INT64_MAX) past the last row.  A row that already is a winner keeps its value in the
// outputs and does not compete again (no row past the last one is a winner).  Every thread of the workgroup calls it (one barrier).
__device__ __forceinline__ void believer_tail(const BelieverStep& b, int64_t g, double v, int64_t idx) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  for (int k = 0; k < b.n_taken; ++k)
    if (b.taken[k] == g) {
      v = -INFINITY;
      idx = INT64_MAX;
    }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (threadIdx.x == 0) {
    b.blk_val[blockIdx.x] = best.v;
    b.blk_idx[blockIdx.x] = best.i;
  }
}

}  // namespace bogp
