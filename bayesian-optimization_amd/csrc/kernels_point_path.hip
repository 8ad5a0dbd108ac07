// kernels_point_path.hip -- value and input gradient of a posterior sample path at B points: the evaluation behind the Thompson polish.
//
// A single-objective path of bogp_sweep_thompson (bogp_api_thompson.hip) is linear in r(x) plus a cosine sum,
//   path_j(x) = beta - b_j + sum_n c_j[n] r_n(x) + sum_l Wt[l][j] cos(omega_l . x + phase_l),   c_j = gamma - g_j,  Wt = sqrt(2 sigma2 / L) W
//   d path_j / d x_k = sum_n c_j[n] d r_n / d x_k - sum_l Wt[l][j] sin(omega_l . x + phase_l) omega_lk
// so it has no variance, no V = L^-1 and no N^2 term: value and gradient cost N d + L d operations a point, and ONE launch forms them
// where a criterion's point takes k_point_rhs + k_point_tri + k_point_finish (kernels_point.hip).  d r_n / d x_k is point_dx_entry
// (bogp_device.h), the expressions of k_point_rhs, D = 0 conventions included.
//
// k_point_path<KERNEL>: one workgroup of 256 threads per point; point b follows path member[b].
//   0  x and theta into LDS (as k_point_rhs).
//   1  conditioning term, per tile of PATH_TILE training rows: thread t takes rows t, t + 256, ... of the tile: weighted distance
//      (dist_term), profile (corr_profile), the radial scalars the derivative reads (r, D, exp(-sqrt(nu2) D)) and c_j[n] into LDS,
//      c_j[n] r_n into its value partial.
//   2  conditioning gradient: the threads rearranged as (slice, k), k fastest over KT lanes (the power of two >= min(d, 64)), 256 / KT
//      slices; slice s sums c_n d r_n / d x_k over the tile's rows s, s + 256 / KT, ... in ascending n, X[n][k] read coalesced along k.
//      d > 64: up to PATH_KP passes over k, one accumulator register each.
//   3  feature term, the same two steps per tile of PATH_TILE features: a thread per feature forms the phase, sin and cos, adds
//      Wt cos to its value partial and leaves u_l = -Wt sin in LDS; the (slice, k) arrangement then sums u_l omega_lk into the SAME
//      accumulators, omega read coalesced along k.
//   4  the value partials meet in LDS and are added in thread order (16 runs of 16, then the 16 sums); the gradient partials in slice
//      order, one k-pass at a time.
// No matrix instruction: a point is two matrix-vector products, each row of a 16-point tile would bring its own c_j and Wt column, and
// B / 16 <= 32 waves would be left for the chip.
// The order of every sum depends on N, d and L alone and a workgroup reads nothing another one wrote: a point's record is
// bit-identical whatever B is, wherever the point stands and whichever members stand beside it.
//
// The record is k_point_finish's for q = 1 with its gradient, so k_polish_step consumes it unchanged:
//   [path, 0, +-path, grad (d), 0 (d), +-grad (d)], the sign -1 when minimising (bogp_sweep_thompson's criterion).
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

namespace {

constexpr int PATH_TILE = 1024;                           // training rows / features per tile: N = 2048 is two tiles
constexpr int PATH_KP = (BOGP_POINT_MAX_D + 63) / 64;     // k-passes of the (slice, k) arrangement at most

template <int KERNEL, int KP>
__global__ __launch_bounds__(256) void k_point_path(PointPathArgs a) {
#pragma clang fp contract(off)
  constexpr bool HAS_D = KERNEL == BOGP_KERNEL_MATERN12 || KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  constexpr bool HAS_E = KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  __shared__ double xs[BOGP_POINT_MAX_D], ths[BOGP_POINT_MAX_D];
  __shared__ double s_c[PATH_TILE];  // c_j[n] of the tile's rows; u_l of the tile's features
  __shared__ double s_r[PATH_TILE];  // r_n
  __shared__ double s_D[HAS_D ? PATH_TILE : 1];
  __shared__ double s_e[HAS_E ? PATH_TILE : 1];
  __shared__ double red[256], red16[16];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int d = a.d, N = a.N, L = a.L;
  const int j = a.member[b];
  for (int k = tid; k < d; k += 256) {
    xs[k] = a.Xb[(size_t)b * d + k];
    ths[k] = a.theta[k];
  }
  // the (slice, k) arrangement of steps 2 and 3
  int KT = 1;
  while (KT < d && KT < 64) KT <<= 1;
  const int NS = 256 / KT, kk = tid & (KT - 1), sl = tid / KT;
  double vpart = 0.0, g[KP];
#pragma unroll
  for (int p = 0; p < KP; ++p) g[p] = 0.0;
  __syncthreads();

  if (a.coef) {
    const double* __restrict__ cj = a.coef + (size_t)j * N;
    for (int n0 = 0; n0 < N; n0 += PATH_TILE) {
      const int nt = min(PATH_TILE, N - n0);
      for (int i = tid; i < nt; i += 256) {
        const double* __restrict__ xr = a.X + (size_t)(n0 + i) * d;
        double s2 = 0.0;
#pragma unroll 8
        for (int k = 0; k < d; ++k) s2 += dist_term<KERNEL>(ths[k], fabs(xs[k] - xr[k]));
        const double rv = corr_profile<KERNEL>(s2);
        const double c = cj[n0 + i];
        s_c[i] = c;
        s_r[i] = rv;
        const double D = sqrt(s2);
        if (HAS_D) s_D[i] = D;
        if (KERNEL == BOGP_KERNEL_MATERN32) s_e[i] = exp(-1.7320508075688772 * D);
        if (KERNEL == BOGP_KERNEL_MATERN52) s_e[i] = exp(-2.23606797749979 * D);
        vpart = __builtin_fma(c, rv, vpart);
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < KP; ++p) {
        const int k = p * KT + kk;
        if (k < d) {
          const double xk = xs[k], tk = ths[k];
          const double* __restrict__ xc = a.X + (size_t)n0 * d + k;
          double acc = g[p];
          for (int i = sl; i < nt; i += NS) {
            const double dr = point_dx_entry<KERNEL>(s_r[i], HAS_D ? s_D[i] : 0.0, HAS_E ? s_e[i] : 0.0, tk, xk - xc[(size_t)i * d]);
            acc = __builtin_fma(s_c[i], dr, acc);
          }
          g[p] = acc;
        }
      }
      __syncthreads();
    }
  }

  const double* __restrict__ wj = a.W + (size_t)j * L;
  for (int l0 = 0; l0 < L; l0 += PATH_TILE) {
    const int lt = min(PATH_TILE, L - l0);
    for (int i = tid; i < lt; i += 256) {
      const double* __restrict__ om = a.omega + (size_t)(l0 + i) * d;
      double ph = 0.0;
#pragma unroll 8
      for (int k = 0; k < d; ++k) ph = __builtin_fma(om[k], xs[k], ph);
      ph += a.phase[l0 + i];
      const double w = wj[l0 + i];
      vpart = __builtin_fma(w, cos(ph), vpart);
      s_c[i] = -1 * (w * sin(ph));
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < KP; ++p) {
      const int k = p * KT + kk;
      if (k < d) {
        const double* __restrict__ oc = a.omega + (size_t)l0 * d + k;
        double acc = g[p];
        for (int i = sl; i < lt; i += NS) acc = __builtin_fma(s_c[i], oc[(size_t)i * d], acc);
        g[p] = acc;
      }
    }
    __syncthreads();
  }

  // ---- 4: the value in thread order, the gradient in slice order
  double* out = a.out + (size_t)b * a.rec_stride;
  const double sign = a.minimize ? -1.0 : 1.0;
  red[tid] = vpart;
  __syncthreads();
  if (tid < 16) {
    double s = red[16 * tid];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += red[16 * tid + u];
    red16[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    double s = red16[0];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += red16[u];
    const double v = (a.beta - (a.coef ? a.bt[j] : 0.0)) + s;
    out[0] = v;
    out[1] = 0.0;
    out[2] = sign * v;
  }
#pragma unroll
  for (int p = 0; p < KP; ++p) {
    if (p * KT >= d) break;
    __syncthreads();
    red[tid] = g[p];
    __syncthreads();
    const int k = p * KT + tid;
    if (tid < KT && k < d) {
      double s = red[tid];
      for (int u = 1; u < NS; ++u) s += red[u * KT + tid];
      out[3 + k] = s;
      out[3 + d + k] = 0.0;
      out[3 + 2 * d + k] = sign * s;
    }
  }
  // a one-point call's record went straight into pinned host memory: the sequence word behind it, as k_point_finish stores it
  if (a.done_flag) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

hipError_t launch_point_path(int kernel, const PointPathArgs& a, int B, hipStream_t st) {
  // d <= 64 is one k-pass: an instantiation of its own, with one accumulator and none of the other passes' address registers
#define CALL(K)                                                                             \
  if (a.d <= 64) hipLaunchKernelGGL((k_point_path<K, 1>), dim3(B), 256, 0, st, a);          \
  else hipLaunchKernelGGL((k_point_path<K, PATH_KP>), dim3(B), 256, 0, st, a)
  switch (kernel) {
    case BOGP_KERNEL_SE: CALL(BOGP_KERNEL_SE); break;
    case BOGP_KERNEL_MATERN12: CALL(BOGP_KERNEL_MATERN12); break;
    case BOGP_KERNEL_MATERN32: CALL(BOGP_KERNEL_MATERN32); break;
    case BOGP_KERNEL_MATERN52: CALL(BOGP_KERNEL_MATERN52); break;
    case BOGP_KERNEL_ABSEXP: CALL(BOGP_KERNEL_ABSEXP); break;
    default: return hipErrorInvalidValue;
  }
#undef CALL
  return hipGetLastError();
}

}  // namespace bogp
