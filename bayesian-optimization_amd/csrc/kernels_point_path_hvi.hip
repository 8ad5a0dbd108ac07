// kernels_point_path_hvi.hip -- hypervolume improvement of a JOINT sample path and its input gradient at B points: the evaluation behind
// the polish of multi-objective Thompson batches.
//
// A member j of bogp_sweep_thompson_ehvi (bogp_api_thompson.hip) draws the m objectives jointly over shared features,
//   path_{j,t}(x) = beta + sum_n c_{j,t}[n] r_n(x) + sum_l Wt[l][j,t] cos(omega_l . x + phase_l),   c_{j,t} = gamma_t - g_{j,t},
//   d path_{j,t} / d x_k = sum_n c_{j,t}[n] d r_n / d x_k - sum_l Wt[l][j,t] sin(omega_l . x + phase_l) omega_lk,   Wt = sqrt(2 sigma2_t / L) W
// and scores x by HVI(y) = sum_c prod_k max(0, min(y_k, u_ck) - l_ck), y = path_{j,.}(x): continuous and piecewise multilinear in y.
// The m targets share r(x), d r / d x and every sin and cos; only the coefficient column and the weight column differ.  So ONE launch
// forms y (m), J = dy/dx (m x d), HVI and its gradient for about the cost of one single-path evaluation (k_point_path,
// kernels_point_path.hip), where m launches of that kernel would redo the distances, the profiles and the phases m times.
//
// k_point_path_hvi<KERNEL, KP, MT>: one workgroup of 256 threads per point; point b follows member member[b], columns member[b] m + t.
// MT >= m is the compiled number of targets (2, 3, 4 or 8); the columns m .. MT - 1 are zeros and never leave the workgroup.
//   A  the Jacobian, k_point_path's tiling and (slice, k) arrangement with MT accumulators in place of one:
//      1  per tile of TILE training rows: thread t takes rows t, t + 256, ...: distance, profile, D, e ONCE, the row's MT coefficients
//         into LDS ([row][MT], so step 2 reads a row's coefficients as one broadcast), c r into its MT value partials.
//      2  (slice, k): slice s sums c_n d r_n / d x_k over rows s, s + 256 / KT, ... -- point_dx_entry ONCE per (row, k), MT fused
//         multiply-adds behind it; d > 64: KP passes over k, MT x KP accumulator registers.
//      3  the same two steps per tile of TILE features: phase, sin, cos ONCE per feature.
//      4  the MT value partials in thread order (16 runs of 16, then the 16 sums), the gradient partials in slice order: y and J in LDS.
//      TILE = 1024 rows for MT <= 4 and 512 for MT = 8: the tile's coefficients (8 MT TILE bytes) and radial scalars (24 TILE bytes) stay
//      at 56 KB or less, the whole workgroup below 64 KB, two workgroups a CU.  The buffers of 4 and of B lie over the tile buffers.
//   B  the scalarisation, same launch: the C cells dealt over the threads (thread t: cells t, t + 256, ... ascending); per cell
//         t_k = max(min(y_k, u_ck) - l_ck, 0);  pre_0 = 1, pre_{k+1} = pre_k t_k;  acc = acc + pre_m           (the sweep's product order)
//         suf_{m-1} = 1, suf_{k-1} = suf_k t_k;  P_k = pre_k suf_k;  w_k = w_k + P_k  where l_ck < y_k < u_ck  (both strict: on a face 0)
//      the m + 1 thread partials in the order of 4; grad_k' = w_0 J[0][k'], then + w_t J[t][k'] with t ascending.  No fused multiply-add
//      in B: from the device's own y and J a NumPy restatement in this order gives HVI, w and grad byte for byte
//      (bogp.thompson.hvi_grad_numpy(from_device=)).  A NaN among the m values: HVI = -inf and a zero gradient.
// No matrix instruction, for k_point_path's reason: a point is a (d x N) by (N x m) product with m <= 8 columns of its OWN member, the
// operand d r / d x is formed on the fly from transcendental radial scalars, and B <= 128 points leave a handful of waves per tile.
// The order of every sum depends on N, d, L and m alone and a workgroup reads nothing another one wrote: a point's outputs are
// bit-identical whatever B is, wherever the point stands and whichever members stand beside it.
//
// The record is k_point_finish's for q = 1 with its gradient, [HVI, 0, +HVI, grad (d), 0 (d), +grad (d)] (HVI is always maximised), so
// k_polish_step consumes it unchanged; y (m) and, on request, J (m x d) go to the point's second block.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

namespace {

constexpr int PATH_KP = (BOGP_POINT_MAX_D + 63) / 64;  // k-passes of the (slice, k) arrangement at most

template <int KERNEL, int KP, int MT>
__global__ __launch_bounds__(256) void k_point_path_hvi(PointPathHviArgs a) {
#pragma clang fp contract(off)
  constexpr bool HAS_D = KERNEL == BOGP_KERNEL_MATERN12 || KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  constexpr bool HAS_E = KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  constexpr int TILE = MT > 4 ? 512 : 1024;  // training rows / features per tile
  constexpr int NBUF = (MT + 3) * TILE;
  static_assert((MT + 1) * 256 + MT * BOGP_POINT_MAX_D <= NBUF, "the reduction buffer and J lie over the tile buffers");
  __shared__ double xs[BOGP_POINT_MAX_D], ths[BOGP_POINT_MAX_D];
  __shared__ double s_buf[NBUF];
  __shared__ double red16[16 * (MT + 1)], s_y[MT], s_w[MT + 1];
  double* const s_c = s_buf;              // [TILE][MT]: c_{j,t}[n] of the tile's rows; u_t[l] = -Wt sin of the tile's features
  double* const s_r = s_buf + MT * TILE;  // r_n
  double* const s_D = s_r + TILE;
  double* const s_e = s_D + TILE;
  double* const s_red = s_buf;                 // steps 4 and B: [MT + 1][256] thread partials
  double* const s_J = s_buf + (MT + 1) * 256;  // J [m][d]
  const int tid = threadIdx.x, b = blockIdx.x;
  const int d = a.d, N = a.N, L = a.L, m = a.m;
  const int j = a.member[b];
  for (int k = tid; k < d; k += 256) {
    xs[k] = a.Xb[(size_t)b * d + k];
    ths[k] = a.theta[k];
  }
  int KT = 1;
  while (KT < d && KT < 64) KT <<= 1;
  const int NS = 256 / KT, kk = tid & (KT - 1), sl = tid / KT;
  double vpart[MT], g[MT][KP];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    vpart[t] = 0.0;
#pragma unroll
    for (int p = 0; p < KP; ++p) g[t][p] = 0.0;
  }
  __syncthreads();

  // ---- A1, A2: the conditioning term
  const double* __restrict__ cj = a.coef + (size_t)j * m * N;
  for (int n0 = 0; n0 < N; n0 += TILE) {
    const int nt = min(TILE, N - n0);
    for (int i = tid; i < nt; i += 256) {
      const double* __restrict__ xr = a.X + (size_t)(n0 + i) * d;
      double s2 = 0.0;
#pragma unroll 8
      for (int k = 0; k < d; ++k) s2 += dist_term<KERNEL>(ths[k], fabs(xs[k] - xr[k]));
      const double rv = corr_profile<KERNEL>(s2);
      s_r[i] = rv;
      const double D = sqrt(s2);
      if (HAS_D) s_D[i] = D;
      if (KERNEL == BOGP_KERNEL_MATERN32) s_e[i] = exp(-1.7320508075688772 * D);
      if (KERNEL == BOGP_KERNEL_MATERN52) s_e[i] = exp(-2.23606797749979 * D);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const double c = t < m ? cj[(size_t)t * N + n0 + i] : 0.0;
        s_c[i * MT + t] = c;
        vpart[t] = __builtin_fma(c, rv, vpart[t]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < KP; ++p) {
      const int k = p * KT + kk;
      if (k < d) {
        const double xk = xs[k], tk = ths[k];
        const double* __restrict__ xc = a.X + (size_t)n0 * d + k;
        for (int i = sl; i < nt; i += NS) {
          const double dr = point_dx_entry<KERNEL>(s_r[i], HAS_D ? s_D[i] : 0.0, HAS_E ? s_e[i] : 0.0, tk, xk - xc[(size_t)i * d]);
#pragma unroll
          for (int t = 0; t < MT; ++t) g[t][p] = __builtin_fma(s_c[i * MT + t], dr, g[t][p]);
        }
      }
    }
    __syncthreads();
  }

  // ---- A3: the feature term
  const double* __restrict__ wj = a.W + (size_t)j * m * L;
  for (int l0 = 0; l0 < L; l0 += TILE) {
    const int lt = min(TILE, L - l0);
    for (int i = tid; i < lt; i += 256) {
      const double* __restrict__ om = a.omega + (size_t)(l0 + i) * d;
      double ph = 0.0;
#pragma unroll 8
      for (int k = 0; k < d; ++k) ph = __builtin_fma(om[k], xs[k], ph);
      ph += a.phase[l0 + i];
      const double cs = cos(ph), sn = sin(ph);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const double w = t < m ? wj[(size_t)t * L + l0 + i] : 0.0;
        vpart[t] = __builtin_fma(w, cs, vpart[t]);
        s_c[i * MT + t] = -1 * (w * sn);
      }
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < KP; ++p) {
      const int k = p * KT + kk;
      if (k < d) {
        const double* __restrict__ oc = a.omega + (size_t)l0 * d + k;
        for (int i = sl; i < lt; i += NS) {
          const double o = oc[(size_t)i * d];
#pragma unroll
          for (int t = 0; t < MT; ++t) g[t][p] = __builtin_fma(s_c[i * MT + t], o, g[t][p]);
        }
      }
    }
    __syncthreads();
  }

  // ---- A4: the values in thread order, the Jacobian in slice order (the tile buffers are free: the last tile ended in a barrier)
#pragma unroll
  for (int t = 0; t < MT; ++t) s_red[t * 256 + tid] = vpart[t];
  __syncthreads();
  if (tid < 16 * MT) {
    const double* r = s_red + (tid >> 4) * 256 + 16 * (tid & 15);
    double s = r[0];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += r[u];
    red16[tid] = s;
  }
  __syncthreads();
  if (tid < m) {
    double s = red16[16 * tid];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += red16[16 * tid + u];
    s_y[tid] = a.beta + s;
  }
#pragma unroll
  for (int p = 0; p < KP; ++p) {
    if (p * KT >= d) break;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MT; ++t) s_red[t * 256 + tid] = g[t][p];
    __syncthreads();
    for (int idx = tid; idx < m * KT; idx += 256) {
      const int t = idx / KT, kq = idx & (KT - 1), k = p * KT + kq;
      if (k < d) {
        const double* r = s_red + t * 256 + kq;
        double s = r[0];
        for (int u = 1; u < NS; ++u) s += r[u * KT];
        s_J[t * d + k] = s;
      }
    }
  }
  __syncthreads();
  if (a.mom) {
    double* mom = a.mom + (size_t)b * a.mom_stride;
    if (tid < m) mom[tid] = s_y[tid];
    if (a.want_jac)
      for (int idx = tid; idx < m * d; idx += 256) mom[m + idx] = s_J[idx];
  }

  // ---- B: the scalarisation over the cells
  double y[MT], w[MT], acc = 0.0;
  bool isnan_y = false;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    y[t] = t < m ? s_y[t] : 0.0;
    w[t] = 0.0;
    isnan_y = isnan_y || y[t] != y[t];
  }
  for (int c = tid; c < a.C; c += 256) {
    const double* __restrict__ lb = a.lower + (size_t)c * m;
    const double* __restrict__ ub = a.upper + (size_t)c * m;
    double tt[MT], pre[MT], p = 1.0;
    bool in[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k)
      if (k < m) {
        const double lo = lb[k], hi = ub[k];
        tt[k] = __builtin_fmax(__builtin_fmin(y[k], hi) - lo, 0.0);
        in[k] = lo < y[k] && y[k] < hi;
        pre[k] = p;
        p = p * tt[k];
      }
    acc = acc + p;
    double suf = 1.0;
#pragma unroll
    for (int k = MT - 1; k >= 0; --k)
      if (k < m) {
        const double P = pre[k] * suf;
        if (in[k]) w[k] = w[k] + P;
        suf = suf * tt[k];
      }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) s_red[t * 256 + tid] = w[t];
  s_red[MT * 256 + tid] = acc;
  __syncthreads();
  if (tid < 16 * (MT + 1)) {
    const double* r = s_red + (tid >> 4) * 256 + 16 * (tid & 15);
    double s = r[0];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += r[u];
    red16[tid] = s;
  }
  __syncthreads();
  if (tid <= MT) {
    double s = red16[16 * tid];
#pragma unroll
    for (int u = 1; u < 16; ++u) s += red16[16 * tid + u];
    s_w[tid] = s;
  }
  __syncthreads();
  double* out = a.out + (size_t)b * a.rec_stride;
  if (tid == 0) {
    const double v = isnan_y ? -INFINITY : s_w[MT];
    out[0] = v;
    out[1] = 0.0;
    out[2] = v;
  }
  for (int k = tid; k < d; k += 256) {
    double s = s_w[0] * s_J[k];
    for (int t = 1; t < m; ++t) s = s + s_w[t] * s_J[t * d + k];
    if (isnan_y) s = 0.0;
    out[3 + k] = s;
    out[3 + d + k] = 0.0;
    out[3 + 2 * d + k] = s;
  }
  // a one-point call's record went straight into pinned host memory: the sequence word behind it, as k_point_finish stores it
  if (a.done_flag) {
    __threadfence_system();
    __syncthreads();
    if (tid == 0) __hip_atomic_store(a.done_flag, a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <int KERNEL, int MT>
void launch_kp(const PointPathHviArgs& a, int B, hipStream_t st) {
  // d <= 64 is one k-pass: an instantiation of its own, with MT accumulators and none of the other passes' address registers
  if (a.d <= 64) hipLaunchKernelGGL((k_point_path_hvi<KERNEL, 1, MT>), dim3(B), 256, 0, st, a);
  else hipLaunchKernelGGL((k_point_path_hvi<KERNEL, PATH_KP, MT>), dim3(B), 256, 0, st, a);
}

template <int KERNEL>
void launch_mt(const PointPathHviArgs& a, int B, hipStream_t st) {
  if (a.m <= 2) launch_kp<KERNEL, 2>(a, B, st);
  else if (a.m == 3) launch_kp<KERNEL, 3>(a, B, st);
  else if (a.m == 4) launch_kp<KERNEL, 4>(a, B, st);
  else launch_kp<KERNEL, 8>(a, B, st);
}

}  // namespace

hipError_t launch_point_path_hvi(int kernel, const PointPathHviArgs& a, int B, hipStream_t st) {
  if (a.m < 1 || a.m > 8 || a.d < 1 || a.d > BOGP_POINT_MAX_D) return hipErrorInvalidValue;
  switch (kernel) {
    case BOGP_KERNEL_SE: launch_mt<BOGP_KERNEL_SE>(a, B, st); break;
    case BOGP_KERNEL_MATERN12: launch_mt<BOGP_KERNEL_MATERN12>(a, B, st); break;
    case BOGP_KERNEL_MATERN32: launch_mt<BOGP_KERNEL_MATERN32>(a, B, st); break;
    case BOGP_KERNEL_MATERN52: launch_mt<BOGP_KERNEL_MATERN52>(a, B, st); break;
    case BOGP_KERNEL_ABSEXP: launch_mt<BOGP_KERNEL_ABSEXP>(a, B, st); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace bogp
