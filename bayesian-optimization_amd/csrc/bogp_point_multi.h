// bogp_point_multi.h -- the front half of a finishing kernel of the B-point path for an m-target model, shared by
// k_point_ehvi_finish (kernels_point_ehvi.hip), k_point_constrained_finish (kernels_point_constrained.hip) and
// k_point_ehvi_constrained_finish (kernels_point_ehvi_constrained.hip): one workgroup of 256 threads per point behind k_point_rhs +
// k_point_tri.  `Args` carries part, rhs, gamma, ld_gamma, N, Npp, nRB, npass, d, estimate_trend, beta, G, ftft and sigma2[]
// (PointEhviArgs / PointConstrainedArgs / PointEhviConstrainedArgs, bogp_internal.h).  The two EHVI finishes also share their cell
// loop and its reduction (point_ehvi_cell_sums, point_ehvi_reduce, below).
//   1. the row-block records of every pass, added in k_point_finish's fixed order: sc = [|V r|^2, w . r], zdr, wdr;
//   2. gamma_k . rhs_c for all m targets and all columns of every pass, straight from the right-hand sides and the m columns of
//      gamma_base, in a fixed order that does not depend on B: dots[pass][NC][MT];
//   3. mu_k = beta + gamma_k . r, MSE_k = max(0, sigma2_k s) with the shared bracket s = 1 - |V r|^2 + u^2, and mfac, the factor of
//      w . dr/dx_i in ds/dx_i.
#pragma once
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

template <int MT, int NC, class Args>
__device__ __forceinline__ void point_multi_sums(const Args& a, int b, double* dots, double* zdr, double* wdr, double (&fin)[4][NC],
                                                 double (&wpart)[4][NC][MT], double (&sc)[2]) {
  constexpr int CW = NC <= 16 ? 16 : 32;  // lanes per row slice of the right-hand sides (>= NC); 256 / CW slices walk the rows
  constexpr int NS = 256 / CW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int d = a.d, npass = a.npass;
  // 1. the row-block records (k_point_finish's order: every 4th block per wave, then ((w0 + w1) + w2) + w3)
  for (int gg = 0; gg < npass; ++gg) {
    const double* base = a.part + ((size_t)b * npass + gg) * (a.nRB + 1) * (2 * NC);
    if (lane < NC) {
      double s = 0.0;
#pragma unroll 8
      for (int w2 = 1 + wv; w2 <= a.nRB; w2 += 4) s += base[(size_t)w2 * (2 * NC) + lane];
      fin[wv][lane] = s;
    }
    __syncthreads();
    if (tid < NC) {
      const double tot = ((fin[0][tid] + fin[1][tid]) + fin[2][tid]) + fin[3][tid];
      const double wv2 = base[NC + tid];
      if (tid == 0) {
        if (gg == 0) {
          sc[0] = tot;
          sc[1] = wv2;
        }
      } else {
        const int k = gg * (NC - 1) + tid - 1;
        if (k < d) {
          zdr[k] = tot;
          wdr[k] = wv2;
        }
      }
    }
    __syncthreads();
  }

  // 2. gamma_k . rhs_c: slice s of the rows n = s, s + NS, ... per lane group; the slices of a wave meet by shuffles, the waves in LDS
  {
    const int c = tid & (CW - 1), s = tid / CW;
    for (int gg = 0; gg < npass; ++gg) {
      const double* __restrict__ rhs = a.rhs + ((size_t)b * npass + gg) * (size_t)a.Npp * NC;
      double acc[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k) acc[k] = 0.0;
      if (c < NC) {
#pragma unroll 4
        for (int n = s; n < a.N; n += NS) {
          const double r = rhs[(size_t)n * NC + c];
#pragma unroll
          for (int k = 0; k < MT; ++k) acc[k] = __builtin_fma(a.gamma[(size_t)k * a.ld_gamma + n], r, acc[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        acc[k] += shfl_xor_f64(acc[k], 32);
        if (CW == 16) acc[k] += shfl_xor_f64(acc[k], 16);
      }
      if (lane < CW && c < NC) {
#pragma unroll
        for (int k = 0; k < MT; ++k) wpart[wv][c][k] = acc[k];
      }
      __syncthreads();
      if (tid < NC * MT) {
        const int cc = tid / MT, k = tid - cc * MT;
        dots[((size_t)gg * NC + cc) * MT + k] = ((wpart[0][cc][k] + wpart[1][cc][k]) + wpart[2][cc][k]) + wpart[3][cc][k];
      }
      __syncthreads();
    }
  }
}

// 3. the moments (every thread forms all of them from the staged sums)
template <int MT, class Args>
__device__ __forceinline__ void point_multi_moments(const Args& a, const double* dots, const double (&sc)[2], double (&mu)[MT], double (&mse)[MT],
                                                    double& mfac) {
  double u2 = 0.0;
  mfac = 0.0;
  if (a.estimate_trend) {
    const double u = (sc[1] - 1.0) / a.G;
    u2 = u * u;
    mfac = (sc[1] - 1.0) * (1.0 / a.ftft);
  }
  const double bracket = 1.0 - sc[0] + u2;
#pragma unroll
  for (int k = 0; k < MT; ++k) {
    mu[k] = a.beta + dots[k];
    double v = bracket * a.sigma2[k];
    if (v < 0.0) v = 0.0;
    mse[k] = v;
  }
}

// the sum of v over the 64 lanes in a fixed order, the same bits in every lane
__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_f64(v, m);
  return v;
}

// 4. of the EHVI finishes (k_point_ehvi_finish, k_point_ehvi_constrained_finish): the C cells [C][MO] over the first MO targets, strided
// over the 256 threads, into this thread's partial sums acc = [EHVI | dEHVI/dmu_k (MO) | dEHVI/dsd_k (MO)]; with a = (l - mu) / sd,
// b = (u - mu) / sd, G(z) = phi(z) - z Phi(-z):  f = sd (G(a) - G(b)),  df/dmu = Phi(-a) - Phi(-b),  df/dsd = phi(a) - phi(b)  (the b terms
// are 0 for u = +inf), and the product over k != j from prefix and suffix products, never by division (an f may be exactly 0).
template <int MO, int MT>
__device__ __forceinline__ void point_ehvi_cell_sums(const double* lower, const double* upper, int C, const double (&mu)[MT], const double (&sd)[MT],
                                                     double (&acc)[2 * MO + 1]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int t = 0; t < 2 * MO + 1; ++t) acc[t] = 0.0;
  for (int c = tid; c < C; c += 256) {
    double f[MO], fm[MO], fs[MO];
#pragma unroll
    for (int k = 0; k < MO; ++k) {
      const double l = lower[(size_t)c * MO + k], u = upper[(size_t)c * MO + k];
      const double za = (l - mu[k]) / sd[k];
      const double pa = norm_pdf(za), ca = ndtr(-za);
      double g = pa - za * ca, dm = ca, ds = pa;
      if (!isinf(u)) {
        const double zb = (u - mu[k]) / sd[k];
        const double pb = norm_pdf(zb), cb = ndtr(-zb);
        g -= pb - zb * cb;
        dm -= cb;
        ds -= pb;
      }
      f[k] = sd[k] * g;
      fm[k] = dm;
      fs[k] = ds;
    }
    double pre[MO];  // pre[k] = prod_{j < k} f_j
    pre[0] = 1.0;
#pragma unroll
    for (int k = 1; k < MO; ++k) pre[k] = pre[k - 1] * f[k - 1];
    acc[0] += pre[MO - 1] * f[MO - 1];
    double suf = 1.0;  // prod_{j > k} f_j
#pragma unroll
    for (int k = MO - 1; k >= 0; --k) {
      const double others = pre[k] * suf;
      acc[1 + k] += others * fm[k];
      acc[1 + MO + k] += others * fs[k];
      suf *= f[k];
    }
  }
}

// ... and their fixed-order reduction over the workgroup into coef[2 MO + 1] (LDS): the bits depend neither on B nor on the launch.  Every
// thread of the workgroup calls it (two barriers).
template <int NV>
__device__ __forceinline__ void point_ehvi_reduce(const double (&acc)[NV], double (&red)[4][NV], double (&coef)[NV]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int t = 0; t < NV; ++t) {
    const double s = wave_sum_fixed(acc[t]);
    if (lane == 0) red[wv][t] = s;
  }
  __syncthreads();
  if (tid < NV) coef[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
  __syncthreads();
}

}  // namespace bogp
