// kernels_point_path_feasible.hip -- the merit "objective where the drawn constraints hold" of a JOINT sample path and its input gradient
// at B points: the evaluation behind the polish of Thompson batches under modelled constraints.
//
// A member j of bogp_sweep_thompson_constrained (m_obj = 1) or bogp_sweep_thompson_ehvi_constrained (m_obj >= 2) draws m = m_obj + n_con
// targets jointly over shared features (kernels_point_path_hvi.hip states the paths and their derivative).  With y_k = path_{j,k}(x),
// k < m_obj, and c_i = path_{j,m_obj+i}(x), i < n_con:
//   e_i = max(plo_i - c_i, c_i - phi_i, 0);  v_i = e_i inv_sd_{m_obj+i};  P = sum_i v_i v_i            against the POLISH bounds plo, phi
//   F   = s y_0 inv_sd_0 (m_obj = 1; s = -1 when minimising)   or   HVI(y_0 .. y_{m_obj-1}) f_scale (m_obj >= 2),  f_scale = prod_k inv_sd_k
//   merit = F - rho P:  C1 in the constraint values, maximised; the host forms plo, phi (the true bounds tightened), inv_sd and f_scale.
//
// k_point_path_feasible<KERNEL, KP, MT>: one workgroup of 256 threads per point; point b follows member member[b], columns member[b] m + t.
// MT >= m is the compiled number of columns (2, 3, 4 or 8); the columns m .. MT - 1 are zeros and never leave the workgroup.
//   A  y (m) and J = dy/dx (m x d): k_point_path_hvi's steps 1 - 4 in its operations and order, so y and J are that kernel's bits for the
//      same columns.  A copy of its own (path_front below): moving that kernel's front half into a shared header changed its register
//      allocation (VGPRs 199 -> 195, 215 -> 211 in four instantiations), so that kernel stays as it was compiled.
//      1  per tile of TILE training rows: thread t takes rows t, t + 256, ...: distance, profile, D, e ONCE, the row's MT coefficients
//         into LDS ([row][MT], one broadcast a row in step 2), c r into its MT value partials.
//      2  (slice, k): slice s sums c_n d r_n / d x_k over rows s, s + 256 / KT, ...; d > 64: KP passes over k, MT x KP accumulators.
//      3  the same two steps per tile of TILE features: phase, sin, cos ONCE per feature.
//      4  the MT value partials in thread order (16 runs of 16, then the 16 sums), the gradient partials in slice order: y and J in LDS.
//      TILE = 1024 rows for MT <= 4 and 512 for MT = 8: below 64 KB of LDS, two workgroups a CU.
//   B  the scalarisation, same launch, no fused multiply-add:
//      1  every thread, i ascending:  d1 = plo_i - c_i, d2 = c_i - phi_i;  e = d1 > 0 ? d1 : 0;  up = d2 > e;  e = up ? d2 : e;
//         v = e inv_sd;  P = P + v v;  g = (2 v) inv_sd;  u_i = up ? g : 0 - g                    (u_i = dP / dc_i; n_con <= 7 terms)
//      2  m_obj >= 2: the C cells over the first m_obj columns dealt over the threads, k_point_path_hvi's part B to the letter (prefix and
//         suffix products, strict faces, the m_obj + 1 thread partials in the order of A4): HVI and w_t.  m_obj = 1: no cells.
//      3  thread 0:  F = (s y_0) inv_sd_0, W_0 = s inv_sd_0   or   F = HVI f_scale, W_t = w_t f_scale;   merit = F - rho P;  Q_i = rho u_i
//      4  grad_k' = W_0 J[0][k'], + W_t J[t][k'] with t ascending, then - Q_i J[m_obj+i][k'] with i ascending.
//      From the device's own y and J a NumPy restatement in this order gives merit and gradient byte for byte
//      (bogp.thompson.feasible_merit_numpy(from_device=)).  A NaN among the m values: merit = -inf and a zero gradient.
// No matrix instruction, for k_point_path's reason: a point is a (d x N) by (N x m) product with m <= 8 columns of its OWN member, the
// operand d r / d x is formed on the fly from transcendental radial scalars, and B <= 128 points leave a handful of waves per tile.
// The order of every sum depends on N, d, L, m and m_obj alone and a workgroup reads nothing another one wrote: a point's outputs are
// bit-identical whatever B is, wherever the point stands and whichever members stand beside it.
//
// The record is k_point_finish's for q = 1 with its gradient, [merit, 0, +merit, grad (d), 0 (d), +grad (d)] (the merit is always
// maximised), so k_polish_step consumes it unchanged; y (m) and, on request, J (m x d) go to the point's second block.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

namespace {

constexpr int PATH_KP = (BOGP_POINT_MAX_D + 63) / 64;  // k-passes of the (slice, k) arrangement at most

template <int MT>
struct PathFront {
  static constexpr int TILE = MT > 4 ? 512 : 1024;  // training rows / features per tile
  static constexpr int NBUF = (MT + 3) * TILE;      // doubles of s_buf
  static_assert((MT + 1) * 256 + MT * BOGP_POINT_MAX_D <= NBUF, "the reduction buffer and J lie over the tile buffers");
};

// A: xs, ths: [BOGP_POINT_MAX_D]; s_buf: [PathFront<MT>::NBUF]; red16: [16 (MT + 1)]; s_y: [MT] -- all in LDS.  On return (behind a
// barrier): s_y[t] = y_t, t < m; J [m][d] at s_buf + (MT + 1) 256; the first (MT + 1) 256 doubles of s_buf are free for B's partials.
template <int KERNEL, int KP, int MT>
__device__ __forceinline__ void path_front(const PointPathFeasibleArgs& a, double* xs, double* ths, double* s_buf, double* red16, double* s_y) {
#pragma clang fp contract(off)
  constexpr bool HAS_D = KERNEL == BOGP_KERNEL_MATERN12 || KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  constexpr bool HAS_E = KERNEL == BOGP_KERNEL_MATERN32 || KERNEL == BOGP_KERNEL_MATERN52;
  constexpr int TILE = PathFront<MT>::TILE;
  double* const s_c = s_buf;              // [TILE][MT]: c_{j,t}[n] of the tile's rows; u_t[l] = -Wt sin of the tile's features
  double* const s_r = s_buf + MT * TILE;  // r_n
  double* const s_D = s_r + TILE;
  double* const s_e = s_D + TILE;
  double* const s_red = s_buf;                 // step 4: [MT][256] thread partials
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

  // ---- 1, 2: the conditioning term
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

  // ---- 3: the feature term
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

  // ---- 4: the values in thread order, the Jacobian in slice order (the tile buffers are free: the last tile ended in a barrier)
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
}


template <int KERNEL, int KP, int MT>
__global__ __launch_bounds__(256) void k_point_path_feasible(PointPathFeasibleArgs a) {
#pragma clang fp contract(off)
  __shared__ double xs[BOGP_POINT_MAX_D], ths[BOGP_POINT_MAX_D];
  __shared__ double s_buf[PathFront<MT>::NBUF];
  __shared__ double red16[16 * (MT + 1)], s_y[MT], s_w[MT + 1], s_g[MT], s_merit;
  double* const s_red = s_buf;                 // B2: [MT + 1][256] thread partials
  double* const s_J = s_buf + (MT + 1) * 256;  // J [m][d]
  const int tid = threadIdx.x, b = blockIdx.x;
  const int d = a.d, m = a.m, mo = a.m_obj;
  path_front<KERNEL, KP, MT>(a, xs, ths, s_buf, red16, s_y);

  // ---- B1: the penalty and its weights (every thread the same few operations: no exchange)
  double y[MT], u[MT], P = 0.0;
  bool isnan_y = false;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    y[t] = t < m ? s_y[t] : 0.0;
    u[t] = 0.0;
    isnan_y = isnan_y || y[t] != y[t];
  }
#pragma unroll
  for (int t = 1; t < MT; ++t)
    if (t >= mo && t < m) {  // (plo, phi and inv_sd are indexed by column)
      const double d1 = a.plo[t] - y[t], d2 = y[t] - a.phi[t];
      double e = d1 > 0.0 ? d1 : 0.0;
      const bool up = d2 > e;
      e = up ? d2 : e;
      const double v = e * a.inv_sd[t];
      P = P + v * v;
      const double g = (2.0 * v) * a.inv_sd[t];
      u[t] = up ? g : 0.0 - g;
    }

  // ---- B2: the cells over the objective columns (none for one objective)
  if (mo >= 2) {
    double w[MT], acc = 0.0;
#pragma unroll
    for (int t = 0; t < MT; ++t) w[t] = 0.0;
    for (int c = tid; c < a.C; c += 256) {
      const double* __restrict__ lb = a.lower + (size_t)c * mo;
      const double* __restrict__ ub = a.upper + (size_t)c * mo;
      double tt[MT], pre[MT], p = 1.0;
      bool in[MT];
#pragma unroll
      for (int k = 0; k < MT; ++k)
        if (k < mo) {
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
        if (k < mo) {
          const double Pk = pre[k] * suf;
          if (in[k]) w[k] = w[k] + Pk;
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
      for (int v = 1; v < 16; ++v) s += r[v];
      red16[tid] = s;
    }
    __syncthreads();
    if (tid <= MT) {
      double s = red16[16 * tid];
#pragma unroll
      for (int v = 1; v < 16; ++v) s += red16[16 * tid + v];
      s_w[tid] = s;
    }
    __syncthreads();
  }

  // ---- B3: the merit and the m weights of the rows of J
  if (tid == 0) {
    const double F = mo >= 2 ? s_w[MT] * a.f_scale : (a.sgn * y[0]) * a.inv_sd[0];
    s_merit = isnan_y ? -INFINITY : F - a.rho * P;
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (t < m) s_g[t] = t >= mo ? a.rho * u[t] : mo >= 2 ? s_w[t] * a.f_scale : a.sgn * a.inv_sd[0];
  }
  __syncthreads();

  // ---- B4: the gradient and the record
  double* out = a.out + (size_t)b * a.rec_stride;
  if (tid == 0) {
    const double v = s_merit;
    out[0] = v;
    out[1] = 0.0;
    out[2] = v;
  }
  for (int k = tid; k < d; k += 256) {
    double s = s_g[0] * s_J[k];
    for (int t = 1; t < mo; ++t) s = s + s_g[t] * s_J[t * d + k];
    for (int t = mo; t < m; ++t) s = s - s_g[t] * s_J[t * d + k];
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
void launch_kp(const PointPathFeasibleArgs& a, int B, hipStream_t st) {
  // d <= 64 is one k-pass: an instantiation of its own, with MT accumulators and none of the other passes' address registers
  if (a.d <= 64) hipLaunchKernelGGL((k_point_path_feasible<KERNEL, 1, MT>), dim3(B), 256, 0, st, a);
  else hipLaunchKernelGGL((k_point_path_feasible<KERNEL, PATH_KP, MT>), dim3(B), 256, 0, st, a);
}

template <int KERNEL>
void launch_mt(const PointPathFeasibleArgs& a, int B, hipStream_t st) {
  if (a.m <= 2) launch_kp<KERNEL, 2>(a, B, st);
  else if (a.m == 3) launch_kp<KERNEL, 3>(a, B, st);
  else if (a.m == 4) launch_kp<KERNEL, 4>(a, B, st);
  else launch_kp<KERNEL, 8>(a, B, st);
}

}  // namespace

hipError_t launch_point_path_feasible(int kernel, const PointPathFeasibleArgs& a, int B, hipStream_t st) {
  if (a.m < 2 || a.m > 8 || a.m_obj < 1 || a.m_obj >= a.m || a.d < 1 || a.d > BOGP_POINT_MAX_D) return hipErrorInvalidValue;
  if (a.m_obj >= 2 ? a.C < 1 : a.C != 0) return hipErrorInvalidValue;
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
