// kernels_believer_ehvi_constrained.hip -- the (m + c)-target half of a Kriging-believer pass for a multi-objective run under
// modelled constraints: per-target variance downdate and feasibility-weighted EHVI (gfx950).
//
// Believing a point p leaves the posterior means as they are and takes ONE rank-one term off the bracket the targets share
// (gpr.py:502-510: MSE_k = sigma2_k (1 - |L^-1 r|^2 + u^2)).  k_believer (kernels_believer.hip) has formed that term in
// correlation units, c(x) = b(x) / sqrt(pivot), for every candidate; per candidate row this kernel then does
//   MSE_k(x) <- MSE_k(x) - sigma2_k c(x)^2  for the MT targets   (exactly 0 on the candidate row that IS p; k_believer_ehvi's expressions)
// and, when the pass stands in front of a step, that step's criterion by k_ehvi_constrained's conventions: targets 0 .. MO - 1 are the
// objectives of the step's cells, targets MO .. MT - 1 constraints feasible in [lo_j, hi_j],
//   sd_k  = sqrt(max(MSE_k, 1e-9)) for the objectives,  P = prod_{k = MO .. MT-1} feasibility(mu_k, MSE_k, sigma2_k, lo, hi) from 1.0
//   value = +0.0 where P == 0.0;  otherwise ehvi_cells<MO>(..) P for C >= 1;  otherwise P for C == 0;  a NaN P propagates
// -- given the same moments, cells and bounds, the bytes k_ehvi_constrained leaves -- with one argmax record per 256 rows over the rows
// that are not winners yet.  A wavefront whose rows all have P == 0 skips the cell loop; every lane reaches the block reduction.
// Elementwise in the global row index: one launch serves all M rows behind the chunk loop, so no bit depends on the chunk size.
// Streams 8 (3 + 4 MT) bytes per candidate (c, the value and P out, and per target the running variance in and out, the mean and the
// clamped variance) plus the cell loop; the 2 MT + 1 loads of a row are issued before the first arithmetic that waits for one.
// No MFMA, LDS for the block reduction only.
#include "bogp_believer_multi.h"

namespace bogp {

template <int MO, int MT>
__global__ __launch_bounds__(256) void k_believer_ehvi_constrained(BelieverEhviConstrainedArgs a) {
  static_assert(MO >= 2 && MO < MT && MT <= 8, "objectives 2 .. MT - 1, at least one constraint");
  const BelieverStep& b = a.step;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;  // candidate row
  const bool valid = g < b.M;
  double P = 1.0;
  double mu_o[MO], sd[MO];  // the objectives' moments, all the cell loop reads
#pragma unroll
  for (int k = 0; k < MO; ++k) {
    mu_o[k] = 0.0;
    sd[k] = 1.0;
  }
  if (valid) {
    // every load of the row first: the running variances, c and the means do not depend on one another
    double s[MT], mu[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) s[k] = b.s[(size_t)g * MT + k];
    const double c = b.update ? b.c[g] : 0.0;
#pragma unroll
    for (int k = 0; k < MT; ++k) mu[k] = 0.0;
    if (b.eval) {
#pragma unroll
      for (int k = 0; k < MT; ++k) mu[k] = b.mu[(size_t)g * MT + k];
    }
    if (b.update) believer_downdate<MT>(b, g, c, s);
    if (b.eval) {
      double mse[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) mse[k] = believer_clamped<MT>(b, g, k, s[k]);
#pragma unroll
      for (int k = 0; k < MO; ++k) {
        mu_o[k] = mu[k];
        sd[k] = sqrt(fmax(mse[k], 1e-9));
      }
#pragma unroll
      for (int k = MO; k < MT; ++k) P *= feasibility(mu[k], mse[k], b.sigma2[k], a.lo[k - MO], a.hi[k - MO]);
      a.pof_out[g] = P;
    }
  }
  if (!b.eval) return;  // (uniform: no barrier is skipped by part of a workgroup)
  // k_ehvi_constrained's value rule: the cell loop runs where some lane of the wavefront is live; the others never read E
  const bool live = valid && !(P == 0.0);
  double E = 1.0;
  if (a.C > 0 && __ballot(live) != 0ull) {
    if (live) E = ehvi_cells<MO>(a.lower, a.upper, a.C, mu_o, sd);
  }
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    v = live ? (a.C > 0 ? E * P : P) : 0.0;
    idx = g;
    a.val_out[g] = v;
  }
  believer_tail(b, g, v, idx);
}

template <int MO, int MT>
static void launch_one(const BelieverEhviConstrainedArgs& a, unsigned nblk, hipStream_t st) {
  hipLaunchKernelGGL((k_believer_ehvi_constrained<MO, MT>), dim3(nblk), 256, 0, st, a);
}

// the 21 pairs 2 <= MO < MT <= BOGP_MAX_TARGETS
template <int MT>
static bool launch_objectives(const BelieverEhviConstrainedArgs& a, unsigned nblk, hipStream_t st) {
  switch (a.m_obj) {
    case 2: if constexpr (MT > 2) { launch_one<2, MT>(a, nblk, st); return true; } break;
    case 3: if constexpr (MT > 3) { launch_one<3, MT>(a, nblk, st); return true; } break;
    case 4: if constexpr (MT > 4) { launch_one<4, MT>(a, nblk, st); return true; } break;
    case 5: if constexpr (MT > 5) { launch_one<5, MT>(a, nblk, st); return true; } break;
    case 6: if constexpr (MT > 6) { launch_one<6, MT>(a, nblk, st); return true; } break;
    case 7: if constexpr (MT > 7) { launch_one<7, MT>(a, nblk, st); return true; } break;
    default: break;
  }
  return false;
}

hipError_t launch_believer_ehvi_constrained(const BelieverEhviConstrainedArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.step.M + 255) / 256);
  bool ok = false;
  switch (a.step.m) {
    case 3: ok = launch_objectives<3>(a, nblk, st); break;
    case 4: ok = launch_objectives<4>(a, nblk, st); break;
    case 5: ok = launch_objectives<5>(a, nblk, st); break;
    case 6: ok = launch_objectives<6>(a, nblk, st); break;
    case 7: ok = launch_objectives<7>(a, nblk, st); break;
    case 8: ok = launch_objectives<8>(a, nblk, st); break;
    default: break;
  }
  if (!ok) return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace bogp
