// kernels_point_ehvi_constrained.hip -- feasibility-weighted expected hypervolume improvement AND its input gradient at B points of an
// (m + c)-target model (gfx950): the point path of k_ehvi_constrained (kernels_ehvi_constrained.hip), whose conventions it restates.
//
// Targets 0 .. MO - 1 are the objectives (maximised as given), target MO + j is the constraint feasible in [lo_j, hi_j]; per point
//   P     = prod_j F_j,  F_j = feasibility(mu_{MO+j}, MSE_{MO+j}, sigma2_{MO+j}, lo_j, hi_j)   in index order from 1.0
//   E     = EHVI of the objectives over the C cells,  sd_k = sqrt(max(MSE_k, 1e-9))             (k_point_ehvi_finish's expressions)
//   value = +0.0 where P == 0.0;  P where C == 0;  otherwise E P
// k_point_ehvi_constrained_finish<MO, MT, NC> runs behind k_point_rhs + k_point_tri (VALU flavour) in place of k_point_finish, one
// workgroup of 256 threads per point, FP64 VALU only:
//   1.-3. the row-block records, gamma_k . rhs_c and the moments mu_k, MSE_k = max(0, sigma2_k s): bogp_point_multi.h, shared with the
//      two sibling finishes.  Objectives: sd_k = sqrt(max(MSE_k, 1e-9)); constraints: sd_k = sqrt(MSE_k) without a floor;
//   4. the constraints (every thread: at most 6): F_j, dF_j/dmu, dF_j/dsd (feasibility_grad), P, and excl_j = prod_{l != j} F_l from
//      prefix and suffix products, never by division; then the cells, strided over the threads (point_ehvi_cell_sums) and reduced in a
//      fixed order (point_ehvi_reduce).  The cells are read only where C >= 1 and P != 0: a dead point runs ZERO cell iterations and goes
//      through the same reduction, so that no barrier and no shuffle stands under a branch on P (P is formed by every thread from the same
//      LDS values, but a barrier under a branch that one day stops being uniform would hang); its E and dE are 0;
//   5. per input dimension i, strided over the threads:
//        dmu_k/dx_i = gamma_k . dr/dx_i,   dMSE_k/dx_i = sigma2_k 2 (-z . dr/dx_i + mfac w . dr/dx_i)
//        objectives:  dsd_k/dx_i = dMSE_k/dx_i / (2 sd_k) where MSE_k > 1e-9 and exactly 0 otherwise (k_point_ehvi_finish's rule)
//        constraints: dsd_k/dx_i = dMSE_k/dx_i / (2 sd_k)                                           (k_point_constrained_finish's rule)
//        dP/dx_i = sum_j excl_j (dF_j/dmu dmu/dx_i + dF_j/dsd dsd/dx_i),   dE/dx_i = sum_k (dE/dmu_k dmu_k/dx_i + dE/dsd_k dsd_k/dx_i)
//        dvalue/dx_i = 0 where P == 0;  dP/dx_i where C == 0;  otherwise (P != 0 ? P dE/dx_i : 0) + (E != 0 ? E dP/dx_i : 0)
//      with k_point_finish's rule: a zero coefficient times anything (0 / 0 at sd = 0 included) is 0, so a gradient is never NaN where
//      the value is finite.  A NaN P is not == 0 and propagates.
// The record has k_point_finish's layout with q = 1 -- [mu_0, MSE_0, value, dmu_0 (d), dMSE_0 (d), dvalue (d)] -- so k_polish_step
// consumes it unchanged; a second block per point holds P, dP (d), E, dE (d), mu (MT), MSE (MT), dmu (MT x d), dMSE (MT x d) when the
// caller asked for it.  Every sum has a fixed order: the bits of a row depend neither on B nor on the launch.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_point_multi.h"

namespace bogp {

namespace {

template <int MO, int MT, int NC>
__global__ __launch_bounds__(256) void k_point_ehvi_constrained_finish(PointEhviConstrainedArgs a) {
  static_assert(MO >= 2 && MO < MT && MT <= 8, "objectives 2 .. MT - 1, at least one constraint");
  constexpr int NV = 2 * MO + 1;  // E | dE/dmu_k | dE/dsd_k
  constexpr int NCON = MT - MO;
  extern __shared__ double dyn[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x, d = a.d, npass = a.npass;
  double* dots = dyn;                            // [npass][NC][MT] gamma_k . rhs_c
  double* zdr = dots + (size_t)npass * NC * MT;  // [d] z . dr/dx_i
  double* wdr = zdr + d;                         // [d] w . dr/dx_i
  __shared__ double fin[4][NC];
  __shared__ double wpart[4][NC][MT];
  __shared__ double sc[2];  // |V r|^2, w . r
  __shared__ double red[4][NV];
  __shared__ double coef[NV];

  // 1.-3. the sums and the moments
  point_multi_sums<MT, NC>(a, b, dots, zdr, wdr, fin, wpart, sc);
  double mfac;
  double mu[MT], mse[MT], sd[MT];
  point_multi_moments<MT>(a, dots, sc, mu, mse, mfac);
#pragma unroll
  for (int k = 0; k < MT; ++k) sd[k] = k < MO ? sqrt(fmax(mse[k], 1e-9)) : sqrt(mse[k]);

  // 4. the constraints ...
  double F[NCON], fm[NCON], fs[NCON], excl[NCON];
  double P = 1.0;
#pragma unroll
  for (int j = 0; j < NCON; ++j) {
    feasibility_grad(mu[MO + j], mse[MO + j], a.sigma2[MO + j], a.lo[j], a.hi[j], &F[j], &fm[j], &fs[j]);
    excl[j] = P;  // prod_{l < j} F_l
    P *= F[j];
  }
  {
    double suf = 1.0;  // prod_{l > j} F_l
#pragma unroll
    for (int j = NCON - 1; j >= 0; --j) {
      excl[j] *= suf;
      suf *= F[j];
    }
  }
  // ... and the cells: none for a dead point, which takes the same barriers
  const bool dead = P == 0.0;
  double acc[NV];
  point_ehvi_cell_sums<MO, MT>(a.lower, a.upper, dead ? 0 : a.C, mu, sd, acc);
  point_ehvi_reduce<NV>(acc, red, coef);
  const bool cells = a.C > 0;
  const double E = coef[0];  // 0 where the loop did not run

  // 5. the record(s)
  double* out = a.out + (size_t)b * a.rec_stride;  // [mu_0, MSE_0, value, dmu_0 (d), dMSE_0 (d), dvalue (d)]
  // [P, dP (d), E, dE (d), mu (MT), MSE (MT), dmu (MT x d), dMSE (MT x d)]
  double* mom = a.mom ? a.mom + (size_t)b * a.mom_stride : nullptr;
  double* momk = mom ? mom + 2 + 2 * (size_t)d : nullptr;
  if (tid == 0) {
    out[0] = mu[0];
    out[1] = mse[0];
    out[2] = dead ? 0.0 : (cells ? E * P : P);
    if (mom) {
      mom[0] = P;
      mom[1 + d] = E;
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        momk[k] = mu[k];
        momk[MT + k] = mse[k];
      }
    }
  }
  for (int i = tid; i < d; i += 256) {
    const int gg = i / (NC - 1), cc = 1 + (i - gg * (NC - 1));
    const double* dk = dots + ((size_t)gg * NC + cc) * MT;
    const double m2 = 2.0 * (-1.0 * zdr[i] + mfac * wdr[i]);  // ds/dx_i (gpr.py:573-576 without sigma2)
    double dE = 0.0, dP = 0.0;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      const double dmu = dk[k];
      const double dmse = a.sigma2[k] * m2;
      if (k < MO) {
        const double c_mu = coef[1 + k], c_sd = coef[1 + MO + k];
        const bool free_sd = mse[k] > 1e-9;  // otherwise sd is the clamp's constant (or MSE the clip's 0): no sd path
        const double t1 = c_mu != 0.0 ? c_mu * dmu : 0.0;
        const double t2 = (free_sd && c_sd != 0.0) ? c_sd * (dmse / (2.0 * sd[k])) : 0.0;
        dE += t1 + t2;
      } else {
        const int j = k - MO;
        const double dsd = dmse / (2.0 * sd[k]);  // (0 / 0 at sd = 0: only ever multiplied by a coefficient that is 0 there)
        const double t1 = fm[j] != 0.0 ? fm[j] * dmu : 0.0;
        const double t2 = fs[j] != 0.0 ? fs[j] * dsd : 0.0;
        dP += excl[j] != 0.0 ? excl[j] * (t1 + t2) : 0.0;
      }
      if (k == 0) {
        out[3 + i] = dmu;
        out[3 + d + i] = dmse;
      }
      if (mom) {
        momk[2 * MT + (size_t)k * d + i] = dmu;
        momk[2 * MT + (size_t)MT * d + (size_t)k * d + i] = dmse;
      }
    }
    if (mom) {
      mom[1 + i] = dP;
      mom[2 + d + i] = dE;
    }
    double grad = 0.0;
    if (!dead) {
      if (cells) {
        const double g1 = P != 0.0 ? P * dE : 0.0;
        const double g2 = E != 0.0 ? E * dP : 0.0;
        grad = g1 + g2;
      } else {
        grad = dP;
      }
    }
    out[3 + 2 * d + i] = grad;
  }
  // 6. one-point calls: the completion word behind the record in pinned host memory (k_point_finish)
  if (a.done_flag) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <int MO, int MT>
hipError_t launch_one(const PointEhviConstrainedArgs& a, int B, hipStream_t st) {
  const int nc = point_columns_per_pass(a.d);
  const size_t shm = ((size_t)a.npass * nc * MT + 2 * (size_t)a.d) * sizeof(double);
  if (nc == 12) hipLaunchKernelGGL((k_point_ehvi_constrained_finish<MO, MT, 12>), dim3(B), 256, shm, st, a);
  else hipLaunchKernelGGL((k_point_ehvi_constrained_finish<MO, MT, 22>), dim3(B), 256, shm, st, a);
  return hipGetLastError();
}

// the 21 pairs 2 <= MO < MT <= BOGP_MAX_TARGETS, as launch_ehvi_constrained dispatches them
template <int MT>
hipError_t launch_objectives(const PointEhviConstrainedArgs& a, int B, hipStream_t st) {
  switch (a.m_obj) {
    case 2: if constexpr (MT > 2) return launch_one<2, MT>(a, B, st); break;
    case 3: if constexpr (MT > 3) return launch_one<3, MT>(a, B, st); break;
    case 4: if constexpr (MT > 4) return launch_one<4, MT>(a, B, st); break;
    case 5: if constexpr (MT > 5) return launch_one<5, MT>(a, B, st); break;
    case 6: if constexpr (MT > 6) return launch_one<6, MT>(a, B, st); break;
    case 7: if constexpr (MT > 7) return launch_one<7, MT>(a, B, st); break;
    default: break;
  }
  return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_point_ehvi_constrained_finish(const PointEhviConstrainedArgs& a, int B, hipStream_t st) {
  switch (a.m) {
    case 3: return launch_objectives<3>(a, B, st);
    case 4: return launch_objectives<4>(a, B, st);
    case 5: return launch_objectives<5>(a, B, st);
    case 6: return launch_objectives<6>(a, B, st);
    case 7: return launch_objectives<7>(a, B, st);
    case 8: return launch_objectives<8>(a, B, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bogp
