// kernels_point_ehvi.hip -- expected hypervolume improvement AND its input gradient at B points of an m-target model (gfx950).
//
// The one-point path of kernels_point.hip produces everything that does not depend on the target: k_point_rhs writes the
// right-hand sides rhs[b][pass][n][NC] = [ r_n | dr_n/dx_i ], k_point_tri the row-block records of |V r|^2, z . dr/dx_i,
// w . r and w . dr/dx_i.  With several targets the variance bracket s = 1 - |V r|^2 + u^2 is shared (MSE_k = sigma2_k s,
// gpr.py:502-510), so only the means need m dot products per column instead of one.  k_point_ehvi_finish<MT, NC> runs behind
// those two kernels in place of k_point_finish, one workgroup of 256 threads per point, FP64 VALU only:
//   1. the row-block records of every pass, added in k_point_finish's fixed order;
//   2. gamma_k . rhs_c for all m targets and all columns of every pass, straight from the right-hand sides and the m columns
//      of gamma_base, in a fixed order that does not depend on B;
//   3. mu_k = beta + gamma_k . r, MSE_k = max(0, sigma2_k s), sd_k = sqrt(max(MSE_k, 1e-9)) (analytic.py:233) and the
//      gradients  dmu_k/dx_i = gamma_k . dr/dx_i,  dMSE_k/dx_i = sigma2_k ds/dx_i;
//   4. the cells, strided over the 256 threads: with a = (l - mu) / sd, b = (u - mu) / sd, G(z) = phi(z) - z Phi(-z),
//        f = sd (G(a) - G(b)),   df/dmu = Phi(-a) - Phi(-b),   df/dsd = phi(a) - phi(b)      (the b terms are 0 for u = +inf)
//        EHVI = sum_c prod_k f_ck,   dEHVI/dmu_j = sum_c (prod_{k != j} f_ck) df_cj/dmu_j,   likewise for sd_j
//      -- the product over k != j from prefix and suffix products, never by division (an f may be exactly 0) --, then a
//      fixed-order reduction over the workgroup: the bits depend neither on B nor on the launch;
//   5. the chain rule  dEHVI/dx_i = sum_k (dEHVI/dmu_k dmu_k/dx_i + dEHVI/dsd_k dsd_k/dx_i),  dsd_k/dx_i = dMSE_k/dx_i / (2 sd_k)
//      where MSE_k > 1e-9 and exactly 0 where the clamp (or the clip at 0) is active; a zero coefficient times anything is 0,
//      as k_point_finish's guards.  The record has k_point_finish's layout with q = 1 -- [mu_0, MSE_0, EHVI, dmu_0 (d),
//      dMSE_0 (d), dEHVI (d)] -- so k_polish_step consumes it unchanged; a second block per point holds mu (m), MSE (m),
//      dmu (m x d), dMSE (m x d) when the caller asked for them;
//   6. the completion word of one-point calls, as k_point_finish stores it.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_point_multi.h"

namespace bogp {

namespace {

template <int MT, int NC>
__global__ __launch_bounds__(256) void k_point_ehvi_finish(PointEhviArgs a) {
  constexpr int NV = 2 * MT + 1;          // value | dEHVI/dmu_k | dEHVI/dsd_k
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

  // 1.-3. the sums and the moments (bogp_point_multi.h; every thread forms all moments: the cell loop below reads them from registers)
  point_multi_sums<MT, NC>(a, b, dots, zdr, wdr, fin, wpart, sc);
  double mfac;
  double mu[MT], mse[MT], sd[MT];
  point_multi_moments<MT>(a, dots, sc, mu, mse, mfac);
#pragma unroll
  for (int k = 0; k < MT; ++k) sd[k] = sqrt(fmax(mse[k], 1e-9));

  // 4. the cells and their fixed-order reduction (bogp_point_multi.h, shared with k_point_ehvi_constrained_finish)
  double acc[NV];
  point_ehvi_cell_sums<MT, MT>(a.lower, a.upper, a.C, mu, sd, acc);
  point_ehvi_reduce<NV>(acc, red, coef);

  // 5. the record(s)
  double* out = a.out + (size_t)b * a.rec_stride;  // [mu_0, MSE_0, EHVI, dmu_0 (d), dMSE_0 (d), dEHVI (d)]
  double* mom = a.mom ? a.mom + (size_t)b * a.mom_stride : nullptr;  // [mu (m), MSE (m), dmu (m x d), dMSE (m x d)]
  if (tid == 0) {
    out[0] = mu[0];
    out[1] = mse[0];
    out[2] = coef[0];
    if (mom) {
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        mom[k] = mu[k];
        mom[MT + k] = mse[k];
      }
    }
  }
  for (int i = tid; i < d; i += 256) {
    const int gg = i / (NC - 1), cc = 1 + (i - gg * (NC - 1));
    const double* dk = dots + ((size_t)gg * NC + cc) * MT;
    const double m2 = 2.0 * (-1.0 * zdr[i] + mfac * wdr[i]);  // ds/dx_i (gpr.py:573-576 without sigma2)
    double grad = 0.0;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      const double dmu = dk[k];
      const double dmse = a.sigma2[k] * m2;
      const double c_mu = coef[1 + k], c_sd = coef[1 + MT + k];
      const bool free_sd = mse[k] > 1e-9;  // otherwise sd is the clamp's constant (or MSE the clip's 0): no sd path
      const double t1 = c_mu != 0.0 ? c_mu * dmu : 0.0;
      const double t2 = (free_sd && c_sd != 0.0) ? c_sd * (dmse / (2.0 * sd[k])) : 0.0;
      grad += t1 + t2;
      if (k == 0) {
        out[3 + i] = dmu;
        out[3 + d + i] = dmse;
      }
      if (mom) {
        mom[2 * MT + (size_t)k * d + i] = dmu;
        mom[2 * MT + (size_t)MT * d + (size_t)k * d + i] = dmse;
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

template <int MT>
hipError_t launch_mt(const PointEhviArgs& a, int B, hipStream_t st) {
  const int nc = point_columns_per_pass(a.d);
  const size_t shm = ((size_t)a.npass * nc * MT + 2 * (size_t)a.d) * sizeof(double);
  if (nc == 12) hipLaunchKernelGGL((k_point_ehvi_finish<MT, 12>), dim3(B), 256, shm, st, a);
  else hipLaunchKernelGGL((k_point_ehvi_finish<MT, 22>), dim3(B), 256, shm, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_point_ehvi_finish(const PointEhviArgs& a, int B, hipStream_t st) {
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
