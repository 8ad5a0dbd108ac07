// kernels_point_constrained.hip -- q feasibility-weighted criteria AND their input gradients at B points of an m-target model (gfx950).
//
// Target 0 is the objective, targets 1 .. m - 1 are constraints feasible in [lo_k, hi_k] (k_constrained's convention); per point
//   value_c = base_c P,   base_c = acq_value(id_c, par_c, +-mu_0, sqrt(MSE_0), plugin, sigma2_0) or 1 for BOGP_ACQ_NONE,
//   P = prod_{k = 1 .. m-1} feasibility(mu_k, MSE_k, sigma2_k, lo_k, hi_k)   in index order from 1.0, as k_constrained forms it.
// k_point_constrained_finish<MT, NC> runs behind k_point_rhs + k_point_tri (VALU flavour) in place of k_point_finish, one workgroup of
// 256 threads per point, FP64 VALU only:
//   1.-3. the row-block records, gamma_k . rhs_c and the moments mu_k, MSE_k = max(0, sigma2_k s): bogp_point_multi.h, shared with
//      k_point_ehvi_finish; sd_k = sqrt(MSE_k) without a floor, because k_constrained has none;
//   4. scalar work: F_k, dF_k/dmu, dF_k/dsd (feasibility_grad), P, and excl_k = prod_{j != k} F_j from prefix and suffix products,
//      never by division (an F may be exactly 0); per criterion base_c and the chain-rule coefficients (acq_grad_coef);
//   5. per input dimension i, strided over the threads:
//        dmu_k/dx_i = gamma_k . dr/dx_i,   dMSE_k/dx_i = sigma2_k 2 (-z . dr/dx_i + mfac w . dr/dx_i),   dsd_k/dx_i = dMSE_k/dx_i / (2 sd_k)
//        dP/dx_i    = sum_k excl_k (dF_k/dmu dmu_k/dx_i + dF_k/dsd dsd_k/dx_i)
//        dacq_c/dx_i = P (c_dy (+-dmu_0/dx_i) + c_dsd dsd_0/dx_i) + base_c dP/dx_i
//      with k_point_finish's rule: a zero coefficient times anything (0 / 0 at sd = 0 included) is 0, so P == 0 kills the first term
//      and base_c == 0 the second.  Where sd_0 is exactly 0 the criterion's coefficients are taken as 0 (EpsilonPI is a step there:
//      its coefficients would be 0 / 0), so a gradient is never NaN where the value is finite.
// The record has k_point_finish's layout for q criteria -- [mu_0, MSE_0, acq (q), dmu_0 (d), dMSE_0 (d), dacq (q x d)] -- so k_polish_step
// (q = 1) consumes it unchanged; a second block per point holds P, dP (d), mu (m), MSE (m), dmu (m x d), dMSE (m x d) when the caller
// asked for it.  Every sum has a fixed order: the bits of a row depend neither on B, nor on the launch, nor on the other criteria.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_point_multi.h"

namespace bogp {

namespace {

template <int MT, int NC>
__global__ __launch_bounds__(256) void k_point_constrained_finish(PointConstrainedArgs a) {
  extern __shared__ double dyn[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x, d = a.d, npass = a.npass, q = a.q;
  double* dots = dyn;                            // [npass][NC][MT] gamma_k . rhs_c
  double* zdr = dots + (size_t)npass * NC * MT;  // [d] z . dr/dx_i
  double* wdr = zdr + d;                         // [d] w . dr/dx_i
  __shared__ double fin[4][NC];
  __shared__ double wpart[4][NC][MT];
  __shared__ double sc[2];  // |V r|^2, w . r
  __shared__ double cbase[BOGP_MAX_Q], cdy[BOGP_MAX_Q], cdsd[BOGP_MAX_Q];

  // 1.-3. the sums and the moments
  point_multi_sums<MT, NC>(a, b, dots, zdr, wdr, fin, wpart, sc);
  double mfac;
  double mu[MT], mse[MT], sd[MT];
  point_multi_moments<MT>(a, dots, sc, mu, mse, mfac);
#pragma unroll
  for (int k = 0; k < MT; ++k) sd[k] = sqrt(mse[k]);

  // 4. the constraints (every thread: at most 7, and step 5 reads them from registers) and the criteria (one thread each)
  double F[MT], fm[MT], fs[MT], excl[MT];
  F[0] = 1.0; fm[0] = 0.0; fs[0] = 0.0; excl[0] = 0.0;
  double P = 1.0;
#pragma unroll
  for (int k = 1; k < MT; ++k) {
    feasibility_grad(mu[k], mse[k], a.sigma2[k], a.lo[k], a.hi[k], &F[k], &fm[k], &fs[k]);
    excl[k] = P;  // prod_{1 <= j < k} F_j
    P *= F[k];
  }
  {
    double suf = 1.0;  // prod_{j > k} F_j
#pragma unroll
    for (int k = MT - 1; k >= 1; --k) {
      excl[k] *= suf;
      suf *= F[k];
    }
  }
  const double sign = a.minimize ? 1.0 : -1.0;
  const double y = sign * mu[0];
  if (tid < q) {
    const int id = a.acq_id[tid];
    double base = 1.0, c_dy = 0.0, c_dsd = 0.0;
    if (id != BOGP_ACQ_NONE) {
      base = acq_value(id, a.acq_par[tid], y, sd[0], a.plugin, a.sigma2[0]);
      if (sd[0] > 0.0) acq_grad_coef(id, a.acq_par[tid], y, sd[0], a.plugin, a.sigma2[0], c_dy, c_dsd);
    }
    cbase[tid] = base;
    cdy[tid] = c_dy;
    cdsd[tid] = c_dsd;
  }
  __syncthreads();

  // 5. the record(s)
  double* out = a.out + (size_t)b * a.rec_stride;  // [mu_0, MSE_0, acq (q), dmu_0 (d), dMSE_0 (d), dacq (q x d)]
  double* mom = a.mom ? a.mom + (size_t)b * a.mom_stride : nullptr;  // [P, dP (d), mu (m), MSE (m), dmu (m x d), dMSE (m x d)]
  if (tid == 0) {
    out[0] = mu[0];
    out[1] = mse[0];
    if (mom) {
      mom[0] = P;
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        mom[1 + d + k] = mu[k];
        mom[1 + d + MT + k] = mse[k];
      }
    }
  }
  if (tid < q) out[2 + tid] = cbase[tid] * P;
  for (int i = tid; i < d; i += 256) {
    const int gg = i / (NC - 1), cc = 1 + (i - gg * (NC - 1));
    const double* dk = dots + ((size_t)gg * NC + cc) * MT;
    const double m2 = 2.0 * (-1.0 * zdr[i] + mfac * wdr[i]);  // ds/dx_i (gpr.py:573-576 without sigma2)
    double dP = 0.0, dy0 = 0.0, dsd0 = 0.0;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      const double dmu = dk[k];
      const double dmse = a.sigma2[k] * m2;
      const double dsd = dmse / (2.0 * sd[k]);  // (0 / 0 at sd = 0: only ever multiplied by a coefficient that is 0 there)
      if (k == 0) {
        dy0 = sign * dmu;
        dsd0 = dsd;
        out[2 + q + i] = dmu;
        out[2 + q + d + i] = dmse;
      } else {
        const double t1 = fm[k] != 0.0 ? fm[k] * dmu : 0.0;
        const double t2 = fs[k] != 0.0 ? fs[k] * dsd : 0.0;
        dP += excl[k] != 0.0 ? excl[k] * (t1 + t2) : 0.0;
      }
      if (mom) {
        mom[1 + d + 2 * MT + (size_t)k * d + i] = dmu;
        mom[1 + d + 2 * MT + (size_t)MT * d + (size_t)k * d + i] = dmse;
      }
    }
    if (mom) mom[1 + i] = dP;
    for (int c = 0; c < q; ++c) {
      const double c_dy = cdy[c], c_dsd = cdsd[c], base = cbase[c];
      const double t1 = c_dy != 0.0 ? c_dy * dy0 : 0.0, t2 = c_dsd != 0.0 ? c_dsd * dsd0 : 0.0;
      const double g1 = P != 0.0 ? P * (t1 + t2) : 0.0;
      const double g2 = base != 0.0 ? base * dP : 0.0;
      out[2 + q + 2 * d + (size_t)c * d + i] = g1 + g2;
    }
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

template <int MT>
hipError_t launch_mt(const PointConstrainedArgs& a, int B, hipStream_t st) {
  const int nc = point_columns_per_pass(a.d);
  const size_t shm = ((size_t)a.npass * nc * MT + 2 * (size_t)a.d) * sizeof(double);
  if (nc == 12) hipLaunchKernelGGL((k_point_constrained_finish<MT, 12>), dim3(B), 256, shm, st, a);
  else hipLaunchKernelGGL((k_point_constrained_finish<MT, 22>), dim3(B), 256, shm, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_point_constrained_finish(const PointConstrainedArgs& a, int B, hipStream_t st) {
  switch (a.m) {
    case 2: return launch_mt<2>(a, B, st);
    case 3: return launch_mt<3>(a, B, st);
    case 4: return launch_mt<4>(a, B, st);
    case 5: return launch_mt<5>(a, B, st);
    case 6: return launch_mt<6>(a, B, st);
    case 7: return launch_mt<7>(a, B, st);
    case 8: return launch_mt<8>(a, B, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bogp
