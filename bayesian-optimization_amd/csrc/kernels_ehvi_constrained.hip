// kernels_ehvi_constrained.hip -- feasibility-weighted expected hypervolume improvement of an (m + c)-target model over one
// correlation chunk (gfx950).
//
// The reference leaves expensive constraints of a multi-objective run as a TODO (BaseMOBO.tell, mobo.py:117-118).  Here targets
// 0 .. MO - 1 of a multi-target model are the objectives (maximised as given, as k_ehvi takes them) and targets MO .. MT - 1 are the
// constraints, feasible in [lo_j, hi_j]; per candidate row
//   mu_k, MSE_k   multi_target_moments (bogp_device.h): k_ehvi's / k_constrained's expressions in their order, the same bits
//   P             = prod_{j = MO .. MT-1} feasibility(mu_j, MSE_j, sigma2_j, lo_j, hi_j), in this order from 1.0
//   E             = ehvi_cells<MO>(lower, upper, C, mu_{0..MO-1}, sd_{0..MO-1}),  sd_k = sqrt(max(MSE_k, 1e-9))  (k_ehvi's expressions)
//   value         = +0.0 where P == 0.0;  otherwise E P for C >= 1;  otherwise P for C == 0 (the probability of feasibility alone,
//                   Gelbart et al. 2014: the criterion while no feasible observation exists)
// P == 0 -> +0.0 is part of the definition (not E * 0, which is NaN for an infinite E and -0.0 never): a wavefront whose rows all have
// P == 0 skips the cell loop, which at m = 3 with 1024 cells is about half of the sweep.  A NaN P is not == 0 and propagates.  np.argmax
// over the rows (first maximum, NaN maximal) into k_ehvi's per-block records, which k_argmax_final / the top-k passes read.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int MO, int MT>
__global__ __launch_bounds__(256) void k_ehvi_constrained(ConstrainedEhviArgs a) {
  static_assert(MO >= 2 && MO < MT && MT <= 8, "objectives 2 .. MT - 1, at least one constraint");
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // row inside the chunk
  const bool valid = i < a.mcount;
  const int64_t g = a.m0 + i;
  double P = 1.0;
  double mu_o[MO], sd[MO];  // the objectives' moments, all the cell loop reads
#pragma unroll
  for (int k = 0; k < MO; ++k) {
    mu_o[k] = 0.0;
    sd[k] = 1.0;
  }
  if (valid) {
    double mu[MT], mse[MT];  // (bogp_device.h: shared with k_ehvi and k_constrained)
    // (ConstrainedEhviArgs keeps its own field order, so it does not hold MultiTargetChunk: bogp_internal.h)
    multi_target_moments<MT, 8>(a.rT, a.gamma, a.ld_gamma, a.N, a.ss_part, a.nJ, a.w_part, a.S, a.Mc, i, a.beta, a.G, a.estimate_trend, a.sigma2, mu, mse);
    store_moments<MT>(a.mu_out, a.mse_out, g, mu, mse);
#pragma unroll
    for (int k = 0; k < MO; ++k) {
      mu_o[k] = mu[k];
      sd[k] = sqrt(fmax(mse[k], 1e-9));
    }
#pragma unroll
    for (int k = MO; k < MT; ++k) P *= feasibility(mu[k], mse[k], a.sigma2[k], a.lo[k - MO], a.hi[k - MO]);
    if (a.pof_out) a.pof_out[g] = P;
  }
  // the cell loop runs where some lane of the wavefront is live; the others never read E
  const bool live = valid && !(P == 0.0);
  double E = 1.0;
  if (a.C > 0 && __ballot(live) != 0ull) {
    if (live) E = ehvi_cells<MO>(a.lower, a.upper, a.C, mu_o, sd);  // (bogp_device.h: shared with k_ehvi, k_believer_ehvi and k_forest_ehvi)
  }
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    v = live ? (a.C > 0 ? E * P : P) : 0.0;
    idx = g;
    a.val_out[g] = v;
  }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (threadIdx.x == 0) {
    a.blk_val[a.blk_offset + blockIdx.x] = best.v;
    a.blk_idx[a.blk_offset + blockIdx.x] = best.i;
  }
}

template <int MO, int MT>
static void launch_one(const ConstrainedEhviArgs& a, unsigned nblk, hipStream_t st) {
  hipLaunchKernelGGL((k_ehvi_constrained<MO, MT>), dim3(nblk), 256, 0, st, a);
}

// the 21 pairs 2 <= MO < MT <= BOGP_MAX_TARGETS
template <int MT>
static bool launch_objectives(const ConstrainedEhviArgs& a, unsigned nblk, hipStream_t st) {
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

hipError_t launch_ehvi_constrained(const ConstrainedEhviArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.mcount + 255) / 256);
  bool ok = false;
  switch (a.m) {
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
