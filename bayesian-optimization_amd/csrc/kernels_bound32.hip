// kernels_bound32.hip -- the FP32 bounding stage of the one-pass pruned sweep (gfx950).
//
// The one-pass flow (kernels_prune.hip) needs the sums r . gamma and w . r of EVERY row behind the pilot only to decide which rows can
// be ruled out; every row that is not ruled out is evaluated again by the exact producer.  That decision does not need FP64: a row
// dropped by a looser bound is still dropped correctly.  Here the sums come from FP32 correlations -- the cross term on
// v_mfma_f32_16x16x4_f32, the hardware square root and exponential -- and every row carries a rigorous margin (bound32_margin,
// bogp_device.h) within which the exact sums lie.  The bound then takes the most optimistic values of the margins' intervals
// (acq_upper_bound_interval), so the rows it flags are a superset of the rows the exact bound flags.
//   k_bound32_prepare  at commit: FP32 copies of the scaled training points, their norms, gamma and w
//   k_bound32_stats    at commit: |gamma|_1, |w|_1, max |b_n|^2 (one workgroup, fixed order)
//   k_bound32_sums     per 64 rows: the two sums and |a|^2 of every row, d <= 32: candidate fragments in registers, a straight-line block,
//                      the profile's constants folded into the operands, the squared distance straight from the matrix chain
//   k_bound32_sums_any the same for any d up to BOUND32_MAX_D: fragments re-read from LDS, the k loop at run time, unscaled operands
//   k_bound32_flags    k_prune_bound with margins: flags and block counts for k_prune_scan / k_prune_index
// Served: SE, Matern-3/2 and Matern-5/2 (profiles with a bounded slope in the squared distance) up to d = BOUND32_MAX_D.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

// kappa: the factor folded into both operands of the register-fragment kernel (d <= 32), so that its squared distance comes out in the
// units its profile wants -- kappa^2 s is exp2's argument for SE and the square of exp2's argument for the Matern kernels -- and no lane
// multiplies by a constant: kappa^2 = log2(e) (SE), 3 log2(e)^2 (Matern-3/2), 5 log2(e)^2 (Matern-5/2).
__host__ __device__ constexpr double bound32_kappa(int kernel) {
  return kernel == BOGP_KERNEL_SE ? 1.2011224087864498 : kernel == BOGP_KERNEL_MATERN32 ? 2.4988211106473432 : 3.225964182229561;
}
constexpr int BOUND32_REG_KS = BOUND32_REG_D / 4;  // k-steps (four dimensions each) up to which the candidate fragments stay in registers

// bscale, nscale: -2 kappa and kappa^2 where the register-fragment kernel serves d (its chain adds a_k (-2 kappa b_k) to kappa^2 (na + nb)),
// 1 and 1 for the general kernel; applied in FP64, one rounding to FP32
__global__ __launch_bounds__(256) void k_bound32_prepare(const double* __restrict__ XthT, const double* __restrict__ xnorm,
                                                         const double* __restrict__ gamma, const double* __restrict__ wvec, int d, int Np,
                                                         int rows, double bscale, double nscale, float* __restrict__ XthT32,
                                                         float* __restrict__ vec32) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (int64_t)rows * Np) XthT32[i] = i < (int64_t)d * Np ? (float)(bscale * XthT[i]) : 0.0f;
  if (i < Np) {
    vec32[i] = (float)(nscale * xnorm[i]);
    vec32[Np + i] = (float)gamma[i];
    vec32[2 * (size_t)Np + i] = (float)wvec[i];
  }
}

__global__ __launch_bounds__(256) void k_bound32_stats(const double* __restrict__ xnorm, const double* __restrict__ gamma,
                                                       const double* __restrict__ wvec, int Np, double* __restrict__ stats) {
  __shared__ double s[3][256];
  double g1 = 0.0, w1 = 0.0, nb = 0.0;
  for (int i = threadIdx.x; i < Np; i += 256) {
    g1 += fabs(gamma[i]);
    w1 += fabs(wvec[i]);
    const double v = xnorm[i];
    nb = (v > nb || v != v) ? v : nb;  // (a NaN norm stays: the margin is then infinite)
  }
  s[0][threadIdx.x] = g1; s[1][threadIdx.x] = w1; s[2][threadIdx.x] = nb;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 256; ++k) {
      g1 += s[0][k];
      w1 += s[1][k];
      const double v = s[2][k];
      nb = (v > nb || v != v) ? v : nb;
    }
    // (the FP64 sums of N non-negative terms are short by N 2^-53 relative at most)
    stats[0] = g1 * (1.0 + 1e-9); stats[1] = w1 * (1.0 + 1e-9); stats[2] = nb;
  }
}

// the profile in FP32 on a clamped squared distance: one hardware square root and one hardware exponential at most
template <int KERNEL>
__device__ __forceinline__ float profile32(float s) {
  if (KERNEL == BOGP_KERNEL_SE) return __builtin_amdgcn_exp2f(s * -1.44269504f);
  const float dist = __builtin_amdgcn_sqrtf(s);
  if (KERNEL == BOGP_KERNEL_MATERN32) {
    const float K = dist * 1.73205081f;
    return (1.0f + K) * __builtin_amdgcn_exp2f(K * -1.44269504f);
  }
  const float K = dist * 2.23606798f;
  const float p = __builtin_fmaf(K, __builtin_fmaf(K, 0.333333333f, 1.0f), 1.0f);
  return p * __builtin_amdgcn_exp2f(K * -1.44269504f);
}

// Workgroup = 64 rows x all training points; wave g takes the 16-point blocks g, g + 4, ...; lane (li, lk) of a block holds the four
// candidates 16 t + li against the four training points 4 lk + c (the C / D layout of the FP32 16x16x4 instruction: row 4 lk + c,
// column li -- NOT the FP64 instruction's lk + 4 c).
constexpr int XS_LD = 80;  // row stride of the candidate tile: the four k rows a wave reads together fall into four different bank groups
template <int KERNEL>
__global__ __launch_bounds__(256) void k_bound32_sums_any(Bound32Args a) {
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  __shared__ float na_s[64];
  __shared__ double red[2][4][64];
  const int d = a.d, Np = a.Np;
  const int KS = (d + 3) >> 2;
  float* xs = smem32;  // [4 KS][XS_LD] theta-scaled candidate tile, k-major, rounded to FP32
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = (int64_t)blockIdx.x * 64;  // first row of the tile within the region
  const int64_t mg0 = a.m0 + r0;
  const int64_t mend = a.m0 + a.rcount < a.M ? a.m0 + a.rcount : a.M;
  for (int idx = tid; idx < 64 * d; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int64_t gm = mg0 + row;
    const double v = gm < mend ? a.Xs[gm * d + k] : 0.0;
    xs[k * XS_LD + row] = (float)(v * a.sqrt_theta[k]);
  }
  for (int idx = tid + XS_LD * d; idx < XS_LD * 4 * KS; idx += 256) xs[idx] = 0.0f;
  double na64 = 0.0;
  if (tid < 64) {  // |a|^2 of the row's FP64 scaled point, summed in dimension order as the exact producer sums it
    const int64_t gm = mg0 + tid;
    if (gm < mend)
      for (int k = 0; k < d; ++k) {
        const double v = a.Xs[gm * d + k] * a.sqrt_theta[k];
        na64 = __builtin_fma(v, v, na64);
      }
    na_s[tid] = (float)na64;
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
  float na[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) na[t] = na_s[16 * t + li];
  typedef float f4t __attribute__((ext_vector_type(4)));
  float mu32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wd32[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double mu[4] = {0.0, 0.0, 0.0, 0.0}, wd[4] = {0.0, 0.0, 0.0, 0.0};
  const float* __restrict__ xth = a.md.XthT;
  const float* bp = xs + lk * XS_LD + li;
  int step = 0;
  for (int n0 = 16 * g; n0 < Np; n0 += 64) {  // (Np is a multiple of 32: a block that begins below Np ends at or below it)
    // this lane's four training points n0 + 4 lk + c: norm, gamma, w (16-byte loads: Np and n0 are multiples of 16)
    const f4t nbv = *reinterpret_cast<const f4t*>(a.md.xnorm + n0 + 4 * lk);
    const f4t gv = *reinterpret_cast<const f4t*>(a.md.gamma + n0 + 4 * lk);
    const f4t wv = *reinterpret_cast<const f4t*>(a.md.wvec + n0 + 4 * lk);
    f4t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f4t){0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int KB = 8;  // A fragments requested together
    for (int ks0 = 0; ks0 < KS; ks0 += KB) {
      float av[KB];
#pragma unroll
      for (int u = 0; u < KB; ++u)
        if (ks0 + u < KS) av[u] = xth[(size_t)(4 * (ks0 + u) + lk) * Np + n0 + li];  // (wave-uniform: a branch, no select in front of the MFMA)
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        if (ks0 + u < KS) {
          const int ks = ks0 + u;
          const float b0 = bp[ks * 4 * XS_LD], b1 = bp[ks * 4 * XS_LD + 16], b2 = bp[ks * 4 * XS_LD + 32], b3 = bp[ks * 4 * XS_LD + 48];
          // (inline asm like every matrix instruction of the library: the accumulators stay in VGPRs; the drain below is by hand -- the rules are in
          // bogp_mfma.h, whose FP64 wrappers do not fit this FP32 chain and its shorter drain)
          asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[0]) : "v"(av[u]), "v"(b0));
          asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[1]) : "v"(av[u]), "v"(b1));
          asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[2]) : "v"(av[u]), "v"(b2));
          asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[3]) : "v"(av[u]), "v"(b3));
        }
      }
    }
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");  // the matrix pipe drains before anything but the chain touches an accumulator
#pragma unroll
    for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(acc[t]));
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float nab = na[t] + nbv[c];
        const float s = __builtin_fmaxf(__builtin_fmaf(-2.0f, acc[t][c], nab), 0.0f);
        const float r = profile32<KERNEL>(s);
        mu32[t] = __builtin_fmaf(r, gv[c], mu32[t]);
        wd32[t] = __builtin_fmaf(r, wv[c], wd32[t]);
      }
    if (++step == BOUND32_FLUSH) {  // (wave-uniform)
      step = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mu[t] += (double)mu32[t]; wd[t] += (double)wd32[t];
        mu32[t] = 0.0f; wd32[t] = 0.0f;
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    mu[t] += (double)mu32[t]; wd[t] += (double)wd32[t];
    // the four point groups of the wave, in a fixed order
    mu[t] += shfl_xor_f64(mu[t], 16); wd[t] += shfl_xor_f64(wd[t], 16);
    mu[t] += shfl_xor_f64(mu[t], 32); wd[t] += shfl_xor_f64(wd[t], 32);
    if (lk == 0) {
      red[0][g][16 * t + li] = mu[t];
      red[1][g][16 * t + li] = wd[t];
    }
  }
  __syncthreads();
  if (tid < 64 && r0 + tid < a.rcount) {
    a.mu[r0 + tid] = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
    a.wd[r0 + tid] = ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid];
    a.na[r0 + tid] = na64;
  }
}

// the profile on sh = kappa^2 s as the chain leaves it (operands scaled by bound32_kappa): no multiplication by a constant in front of
// the square root or the exponential, |.| as a source modifier where a clamp stood (for S >= 0, ||sh| - S| <= |sh - S|)
template <int KERNEL>
__device__ __forceinline__ float profile32_scaled(float sh) {
  if (KERNEL == BOGP_KERNEL_SE) return __builtin_amdgcn_exp2f(-__builtin_fabsf(sh));
  const float K = __builtin_amdgcn_sqrtf(__builtin_fabsf(sh));  // = log2(e) sqrt(3 s) or log2(e) sqrt(5 s)
  const float e = __builtin_amdgcn_exp2f(-K);
  if (KERNEL == BOGP_KERNEL_MATERN32) return __builtin_fmaf(K, 0.693147181f, 1.0f) * e;
  return __builtin_fmaf(K, __builtin_fmaf(K, 0.160151005f, 0.693147181f), 1.0f) * e;  // 1 + ln2 K + (ln2^2 / 3) K^2
}

// The same workgroup, wave and lane layout for d <= 32 (KS = ceil(d / 4) <= BOUND32_REG_KS at compile time).  The candidate tile belongs
// to the workgroup and the loop runs over training blocks, so each lane reads its 4 KS fragment values from LDS ONCE and keeps them; a
// block is straight-line: loads, 4 KS matrix instructions, the drain, the profile.  The operands carry the profile's constants
// (bound32_kappa): the tile holds fl(kappa a), the commit-time copy fl(-2 kappa b) and fl(kappa^2 nb), and the accumulators start at
// fl(kappa^2 na) + fl(kappa^2 nb), so the drained accumulator IS kappa^2 s -- the matrix instruction assembles na + nb - 2 a.b itself.
// WD = false under simple kriging: w is all zeros there and k_bound32_flags reads w . r only with a trend, so that sum is written as 0.
template <int KERNEL, int KS, bool WD>
__global__ __launch_bounds__(256, 4) void k_bound32_sums(Bound32Args a) {  // (four waves a SIMD at least: 128 registers, as the general kernel has)
  extern __shared__ __attribute__((aligned(16))) float smem32[];
  __shared__ float na_s[64];
  __shared__ double red[2][4][64];
  constexpr double KAPPA = bound32_kappa(KERNEL);
  const int d = a.d, Np = a.Np;
  float* xs = smem32;  // [4 KS][XS_LD] theta- and kappa-scaled candidate tile, k-major, rounded to FP32
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t r0 = (int64_t)blockIdx.x * 64;  // first row of the tile within the region
  const int64_t mg0 = a.m0 + r0;
  const int64_t mend = a.m0 + a.rcount < a.M ? a.m0 + a.rcount : a.M;
  for (int idx = tid; idx < 64 * d; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int64_t gm = mg0 + row;
    const double v = gm < mend ? a.Xs[gm * d + k] : 0.0;
    xs[k * XS_LD + row] = (float)(v * a.sqrt_theta[k] * KAPPA);
  }
  for (int idx = tid + XS_LD * d; idx < XS_LD * 4 * KS; idx += 256) xs[idx] = 0.0f;
  double na64 = 0.0;
  if (tid < 64) {  // |a|^2 of the row's FP64 scaled point, summed in dimension order as the exact producer sums it (exported unscaled)
    const int64_t gm = mg0 + tid;
    if (gm < mend)
      for (int k = 0; k < d; ++k) {
        const double v = a.Xs[gm * d + k] * a.sqrt_theta[k];
        na64 = __builtin_fma(v, v, na64);
      }
    na_s[tid] = (float)(na64 * (KAPPA * KAPPA));
  }
  __syncthreads();
  const int li = lane & 15, lk = lane >> 4;
  typedef float f4t __attribute__((ext_vector_type(4)));
  float na[4], bf[KS][4];  // kappa^2 |a|^2 and the B fragments of the lane's four candidates 16 t + li: loop-invariant
#pragma unroll
  for (int t = 0; t < 4; ++t) na[t] = na_s[16 * t + li];
#pragma unroll
  for (int u = 0; u < KS; ++u)
#pragma unroll
    for (int t = 0; t < 4; ++t) bf[u][t] = xs[(4 * u + lk) * XS_LD + 16 * t + li];
  float mu32[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wd32[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double mu[4] = {0.0, 0.0, 0.0, 0.0}, wd[4] = {0.0, 0.0, 0.0, 0.0};
  // NO VECTOR ADDRESS ARITHMETIC IN THE LOOP (the form k_contract16d's loads have, DESIGN.md 5.2''): every address is a scalar base --
  // the operand's row at column n0, stepped by scalar arithmetic -- plus one of the lane's two loop-invariant 32-bit byte offsets, the
  // `v_offset, s[base]` form of global_load.  hipcc selects that form only where it sees the zero-extension of the offset next to the load,
  // so the offsets pass through an empty asm inside the loop; hoisted, each load gets a 64-bit vector add on the pipe the chain needs.
  // (offA <= 4 (3 Np + 15) bytes: launch_bound32_sums refuses an Np at which that would not fit 32 bits, for this kernel alone.)
  unsigned offA = 4u * ((unsigned)lk * (unsigned)Np + (unsigned)li);  // fragment row 4 u + lk, column n0 + li
  unsigned offV = 16u * (unsigned)lk;                                 // the lane's four training points n0 + 4 lk + c
  const size_t rowstep = (size_t)16 * Np;                             // four rows of the commit-time copy, in bytes
  typedef const __attribute__((address_space(1))) char* gbytes;  // (a global pointer: through the asm below a generic one would load flat)
  typedef const __attribute__((address_space(1))) float* gfloat;
  typedef const __attribute__((address_space(1))) f4t* gf4;
  const gbytes xthb = (gbytes) reinterpret_cast<const char*>(a.md.XthT);
  const gbytes nbb = (gbytes) reinterpret_cast<const char*>(a.md.xnorm);
  const gbytes gb = (gbytes) reinterpret_cast<const char*>(a.md.gamma);
  const gbytes wb = (gbytes) reinterpret_cast<const char*>(a.md.wvec);
  struct Operands {  // of one 16-point block: this lane's A fragments, and norm, gamma, w of its four training points n0 + 4 lk + c
    float av[KS];
    f4t nbv, gv, wv;
  };
  auto load = [&](int n0, Operands& o) {  // (16-byte loads: Np and n0 are multiples of 16)
    asm volatile("" : "+v"(offA), "+v"(offV));
    const size_t col = (size_t)4 * n0;  // (wave-uniform: n0 comes from g)
    // (each base passes through an empty asm as a scalar, or the compiler adds the column to the lane's offset first -- a vector add again)
    gbytes pn = nbb + col, pg = gb + col, pw = wb + col;
    asm volatile("" : "+s"(pn), "+s"(pg));
    o.nbv = *(gf4)(pn + offV);
    o.gv = *(gf4)(pg + offV);
    if (WD) {
      asm volatile("" : "+s"(pw));
      o.wv = *(gf4)(pw + offV);
    }
#pragma unroll
    for (int u = 0; u < KS; ++u) {
      gbytes pa = xthb + u * rowstep + col;
      asm volatile("" : "+s"(pa));
      o.av[u] = *(gfloat)(pa + offA);
    }
    __builtin_amdgcn_sched_barrier(0);  // every request of the block goes out before the first of them is waited for
  };
  int step = 0;
  // (the operands are asked for at the top of their own block: asking one block ahead cost 5 registers, the fifth wave a SIMD and 0.14 ms
  // at C3 -- profiles/bound32_trim.txt)
  for (int n0 = 16 * g; n0 < Np; n0 += 64) {  // (Np is a multiple of 32: a block that begins below Np ends at or below it)
    Operands o;
    load(n0, o);
    f4t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[t][c] = na[t] + o.nbv[c];
    // (inline asm like every matrix instruction of the library: the accumulators stay in VGPRs; the drain below is by hand -- the rules are in
    // bogp_mfma.h, whose FP64 wrappers do not fit this FP32 chain and its shorter drain.  s_nop 1: the accumulators were written by vector
    // instructions just above, and nothing pads an asm statement's operands)
    asm volatile(
        "s_nop 1\n\t"
        "v_mfma_f32_16x16x4_f32 %0, %4, %5, %0\n\t"
        "v_mfma_f32_16x16x4_f32 %1, %4, %6, %1\n\t"
        "v_mfma_f32_16x16x4_f32 %2, %4, %7, %2\n\t"
        "v_mfma_f32_16x16x4_f32 %3, %4, %8, %3"
        : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])
        : "v"(o.av[0]), "v"(bf[0][0]), "v"(bf[0][1]), "v"(bf[0][2]), "v"(bf[0][3]));
#pragma unroll
    for (int u = 1; u < KS; ++u)
#pragma unroll
      for (int t = 0; t < 4; ++t) asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(o.av[u]), "v"(bf[u][t]));
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");  // the matrix pipe drains before anything but the chain touches an accumulator
#pragma unroll
    for (int t = 0; t < 4; ++t) asm volatile("" : "+v"(acc[t]));
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float r = profile32_scaled<KERNEL>(acc[t][c]);
        mu32[t] = __builtin_fmaf(r, o.gv[c], mu32[t]);
        if (WD) wd32[t] = __builtin_fmaf(r, o.wv[c], wd32[t]);
      }
    if (++step == BOUND32_FLUSH) {  // (wave-uniform)
      step = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mu[t] += (double)mu32[t];
        mu32[t] = 0.0f;
        if (WD) { wd[t] += (double)wd32[t]; wd32[t] = 0.0f; }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    // the four point groups of the wave, in a fixed order
    mu[t] += (double)mu32[t];
    mu[t] += shfl_xor_f64(mu[t], 16);
    mu[t] += shfl_xor_f64(mu[t], 32);
    if (lk == 0) red[0][g][16 * t + li] = mu[t];
    if (WD) {
      wd[t] += (double)wd32[t];
      wd[t] += shfl_xor_f64(wd[t], 16);
      wd[t] += shfl_xor_f64(wd[t], 32);
      if (lk == 0) red[1][g][16 * t + li] = wd[t];
    }
  }
  __syncthreads();
  if (tid < 64 && r0 + tid < a.rcount) {
    a.mu[r0 + tid] = ((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid];
    a.wd[r0 + tid] = WD ? ((red[1][0][tid] + red[1][1][tid]) + red[1][2][tid]) + red[1][3][tid] : 0.0;
    a.na[r0 + tid] = na64;
  }
}

// k_prune_bound's statements on the FP32 sums and their margins: y_hat within e_mu of the row's exact value, sd_ub from the largest
// |w . r - 1| the margin allows.  A row is dropped only when every criterion's interval bound is below its threshold.
__global__ __launch_bounds__(256) void k_bound32_flags(PruneBoundArgs a, int kernel, int d, const double* __restrict__ wdv,
                                                       const double* __restrict__ nav, Bound32Model md) {
  __shared__ int s_cnt[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.rcount;
  bool keep = false;
  if (valid) {
    double e_mu, e_w;
    bound32_margin(kernel, d, nav[i], md.nb_max, md.gamma_l1, md.w_l1, &e_mu, &e_w);
    const double mu = a.beta + a.mu_part[i];
    double u2 = 0.0;
    if (a.estimate_trend) {
      const double u = (fabs(wdv[i] - 1.0) + e_w) / fabs(a.G);
      u2 = u * u;
    }
    // (1e-12: the roundings of the exact bound's own u, u2, mse and square root, each of which this one must not fall below)
    const double sd_ub = sqrt((1.0 + u2) * a.sigma2) * (1.0 + 1e-12);
    const double y_hat = a.minimize ? mu : -1 * mu;
    const double e_y = e_mu + 1e-15 * fabs(mu);  // (the rounding of beta + the sum, on both sides)
    keep = true;
    bool below = true;
    for (int c = 0; c < a.q; ++c) {
      const double b = acq_upper_bound_interval(a.acq_id[c], a.acq_par[c], y_hat, e_y, sd_ub, a.plugin, a.sigma2);
      below = below && prune_below(b, a.best_val[c]);  // (false for a NaN or an infinity)
    }
    keep = !below;
    a.flags[i] = keep ? 1 : 0;
  }
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) a.blk_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

hipError_t launch_bound32_prepare(int kernel, const double* XthT, const double* xnorm, const double* gamma, const double* wvec, int d, int Np,
                                  float* XthT32, float* vec32, double* stats, hipStream_t st) {
  const int rows = 4 * ((d + 3) / 4);
  const bool reg = rows <= 4 * BOUND32_REG_KS;  // the kernel launch_bound32_sums will pick for this d
  const double kappa = bound32_kappa(kernel), bscale = -2.0 * kappa;
  hipLaunchKernelGGL(k_bound32_prepare, dim3((unsigned)(((size_t)rows * Np + 255) / 256)), 256, 0, st, XthT, xnorm, gamma, wvec, d, Np, rows,
                     reg ? bscale : 1.0, reg ? kappa * kappa : 1.0, XthT32, vec32);
  hipLaunchKernelGGL(k_bound32_stats, dim3(1), 256, 0, st, xnorm, gamma, wvec, Np, stats);
  return hipGetLastError();
}

template <int KERNEL, int KS>
static void launch_bound32_sums_reg(const Bound32Args& a, dim3 grid, size_t shm, hipStream_t st) {
  if (a.estimate_trend) hipLaunchKernelGGL((k_bound32_sums<KERNEL, KS, true>), grid, 256, shm, st, a);
  else hipLaunchKernelGGL((k_bound32_sums<KERNEL, KS, false>), grid, 256, shm, st, a);
}
template <int KERNEL>
static void launch_bound32_sums_of(const Bound32Args& a, dim3 grid, size_t shm, hipStream_t st) {
  switch ((a.d + 3) / 4) {
    case 1: launch_bound32_sums_reg<KERNEL, 1>(a, grid, shm, st); break;
    case 2: launch_bound32_sums_reg<KERNEL, 2>(a, grid, shm, st); break;
    case 3: launch_bound32_sums_reg<KERNEL, 3>(a, grid, shm, st); break;
    case 4: launch_bound32_sums_reg<KERNEL, 4>(a, grid, shm, st); break;
    case 5: launch_bound32_sums_reg<KERNEL, 5>(a, grid, shm, st); break;
    case 6: launch_bound32_sums_reg<KERNEL, 6>(a, grid, shm, st); break;
    case 7: launch_bound32_sums_reg<KERNEL, 7>(a, grid, shm, st); break;
    case 8: launch_bound32_sums_reg<KERNEL, 8>(a, grid, shm, st); break;
    default: hipLaunchKernelGGL((k_bound32_sums_any<KERNEL>), grid, 256, shm, st, a); break;  // (what launch_bound32_prepare left unscaled)
  }
}

hipError_t launch_bound32_sums(int kernel, const Bound32Args& a, hipStream_t st) {
  if (!bound32_supported(kernel, a.d)) return hipErrorInvalidValue;
  // k_bound32_sums (d <= 32) addresses a fragment by a 32-bit byte offset of at most 4 (3 Np + 15) from its row's base
  if ((a.d + 3) / 4 <= BOUND32_REG_KS && 4 * (3 * (int64_t)a.Np + 15) > (int64_t)UINT32_MAX) return hipErrorInvalidValue;
  static_assert(BOUND32_REG_KS == 8, "launch_bound32_sums_of lists the register-fragment kernels case by case");
  const dim3 grid((unsigned)((a.rcount + 63) / 64));
  const size_t shm = (size_t)4 * ((a.d + 3) / 4) * XS_LD * sizeof(float);  // <= 40 KB (BOUND32_MAX_D)
  switch (kernel) {
    case BOGP_KERNEL_SE: launch_bound32_sums_of<BOGP_KERNEL_SE>(a, grid, shm, st); break;
    case BOGP_KERNEL_MATERN32: launch_bound32_sums_of<BOGP_KERNEL_MATERN32>(a, grid, shm, st); break;
    default: launch_bound32_sums_of<BOGP_KERNEL_MATERN52>(a, grid, shm, st); break;
  }
  return hipGetLastError();
}

hipError_t launch_bound32_flags(const PruneBoundArgs& pb, int kernel, int d, const double* wd, const double* na, const Bound32Model& md,
                                hipStream_t st) {
  hipLaunchKernelGGL(k_bound32_flags, dim3((unsigned)((pb.rcount + 255) / 256)), 256, 0, st, pb, kernel, d, wd, na, md);
  return hipGetLastError();
}

}  // namespace bogp
