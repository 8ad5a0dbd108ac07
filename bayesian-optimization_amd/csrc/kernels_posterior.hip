// kernels_posterior.hip -- the candidates/sec hot path of libbogp on gfx950 (MI355X).
//
// Replaces GaussianProcess.predict (surrogate/gaussian_process/gpr.py:486-510):
//     dx = |X*_i - X_j|                  (M*N, d) temporary          -> never materialised
//     r  = corr(theta, dx)               (M, N)                      -> k_corr_chunk   (FP64 VALU)
//     mu = mean + r @ gamma                                          -> k_corr_chunk   (fused)
//     rt = solve_triangular(L, r.T)      N^2 flops per candidate     -> k_contract     (FP64 MFMA)
//     1 - sum(rt^2) [+ sum(u^2)]                                     -> k_contract epilogue (+ acquisition kernel)
//
// Design constants come from measurements on the target (tools/probes/ubench_f64*.hip, tools/probes/ubench_mfma16.hip; profiles/r01_ubench_f64.txt,
// r01_ubench_mfma16.txt, r01_ubench_mfma_stream.txt):
//   * v_mfma_f64_4x4x4_4b_f64 issues every 16 cycles (512 flop) = 32 flop/clk/SIMD = the 78.6 TF/s FP64 peak (kernel B below);
//     v_mfma_f64_16x16x4_f64 issues every 64 cycles (2048 flop) = the same rate -- but only with its accumulator in
//     architectural VGPRs (with AGPR accumulators, where the builtin puts them: ~130 cycles).  Kernel B' below, the DEFAULT,
//     is built on it: one A and one B register per 2048 flop instead of four rotated A registers.
//   * FP64 VALU work does not hide beside FP64 MFMA (same DP pipe: times add), so the kernel-matrix
//     producer must run ONCE per (candidate, training point) -- it is split into its own kernel and r is
//     staged through HBM/L2 in candidate chunks instead of being recomputed per column tile.
//   * lane layout of v_mfma_f64_4x4x4_4b_f64 (tools/probes/probe_mfma_layout.hip): A lane = 16k+4b+i,
//     B lane = 16k+4b+j, D lane = 16i+4b+j  (b = block 0..3).
//
// Triangular contraction.  With V = L^-1 (lower triangular, packed once per fit into B-fragment order),
// rt = V r and sum(rt^2) = sum_j (sum_{n<=j} V[j][n] r[n])^2.  A workgroup owns 64 candidates x 256 columns j
// (4 waves x 4 sixteen-wide column tiles, dealt so that every wave carries the same share of the diagonal) and walks n in
// blocks of 32; 16x16 blocks above the diagonal are skipped (executed flops ~= N^2 (1 + 16/N) per candidate).
// A 16x16 output tile is 4 instructions: instruction t pairs A row-block (b+t)%4 with B column-block b, so ONE
// B register and four rotated A reads (LDS) feed 2048 flop.
#include <algorithm>
#include <cstdlib>

#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_mfma.h"

namespace bogp {

// ---------------------------------------------------------------------------------------------------
// Kernel A: correlation chunk  rT[n][m] = corr(theta, |x*_m - x_n|), + partial mean / trend dot products
//   grid (Mc/64, S): 64 candidates x one slice of the training set per workgroup; 256 threads.
//   thread (m = tid&63, g = tid>>6) produces r for 8 consecutive n per 32-block; the training rows are
//   wave-uniform => scalar loads from the theta-scaled transposed copy XthT[d][Np].
// ---------------------------------------------------------------------------------------------------
struct CorrDims {
  int64_t M, m0, Mc;
  int d, Np, nblk_per_split;
  int wld;  // PV > 0: row pitch of Wrow
};
// pointers are separate __restrict__ kernel arguments (not struct members) so that the wave-uniform reads of
// XthT / gamma / wvec are provably read-only and become scalar (SMEM) loads
// PV > 0 (polynomial trend with p <= PV columns under universal kriging, r04): the producer also forms the slice sums of
// T = W^T r, W = L^-T Ft (gpr.py:496-498: Ft^T L^-1 r).  Every 32-row block of r is parked in LDS on its way out and contracted there
// against the rows Wrow[n][0 .. PV) on the matrix cores -- wave g: candidates 16 g .. 16 g + 15 x PV / 16 column tiles,
// v_mfma_f64_16x16x4_f64 (the columns p .. PV of Wrow are zero padding) -- 16 MFMAs a block and wave beside ~450 FP64 VALU
// instructions.  The separate tile product it replaces re-read the whole 1-GiB correlation chunk for 21 live columns of a 128-column
// tile (+13 % per sweep for a linear trend at C3).  A first version with PV scalar-loaded FMAs a pair doubled the producer's time
// (SGPR-starved: 8 x 24 wave-uniform doubles a block): profiles/r04_trend_timing.txt.
template <int KERNEL, int PV>
__global__ __launch_bounds__(256) void k_corr_chunk(const double* __restrict__ Xs, const double* __restrict__ sqrt_theta,
                                                    const double* __restrict__ XthT, const double* __restrict__ gamma,
                                                    const double* __restrict__ wvec, double* __restrict__ rT,
                                                    double* __restrict__ mu_part, double* __restrict__ w_part,
                                                    const double* __restrict__ Wrow, double* __restrict__ t_part, CorrDims a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* xs = smem;  // [d][64] theta-scaled candidate tile, k-major
  const int tid = threadIdx.x;
  const int m = tid & 63;
  const int g = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t mc0 = (int64_t)blockIdx.x * 64;  // offset inside the chunk
  const int64_t mg0 = a.m0 + mc0;                // global candidate index of row 0
  const int d = a.d;

  for (int idx = tid; idx < 64 * d; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int64_t gm = mg0 + row;
    const double v = gm < a.M ? Xs[gm * d + k] : 0.0;
    xs[k * 64 + row] = v * sqrt_theta[k];
  }
  __syncthreads();

  const double pexp = kernel_exponent<KERNEL>(sqrt_theta, d);
  const int nb0 = blockIdx.y * a.nblk_per_split * 32;
  const int nb1 = min(a.Np, nb0 + a.nblk_per_split * 32);
  double mu = 0.0, wd = 0.0;
  constexpr int NTT = PV > 0 ? PV / 16 : 1;
  d4 tacc[NTT];
#pragma unroll
  for (int c = 0; c < NTT; ++c) tacc[c] = (d4){0.0, 0.0, 0.0, 0.0};
  double* rtile = smem + max(64 * d, 512);  // PV > 0: [32][64] the block of r being contracted (behind the candidate tile / the reduction arrays)
  const int lk = m >> 4, li = m & 15;
  for (int nb = nb0; nb < nb1; nb += 32) {
    const int n0 = nb + g * 8;
    double acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = dist_init<KERNEL>();
#pragma unroll 2
    for (int k = 0; k < d; ++k) {
      const double xk = xs[k * 64 + m];
      const double* __restrict__ xr = XthT + (size_t)k * a.Np + n0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        acc[i] = dist_accumulate<KERNEL>(xk - xr[i], acc[i], pexp);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double r = corr_profile<KERNEL>(acc[i], pexp);
      rT[(size_t)(n0 + i) * a.Mc + mc0 + m] = r;
      mu = __builtin_fma(r, gamma[n0 + i], mu);
      wd = __builtin_fma(r, wvec[n0 + i], wd);
      if (PV > 0) rtile[(g * 8 + i) * 64 + m] = r;
    }
    if (PV > 0) {
      __syncthreads();
      // A: lane (k, i) = r[candidate 16 g + i][n = nb + 4 ks + k];  B: lane (k, j) = W[n][16 t + j]
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const double av = rtile[(4 * ks + lk) * 64 + 16 * g + li];
        const double* __restrict__ wr = Wrow + (size_t)(nb + 4 * ks + lk) * a.wld + li;
#pragma unroll
        for (int t = 0; t < NTT; ++t) {
          const double bv = wr[16 * t];
          mfma16(av, bv, tacc[t]);
        }
      }
      __syncthreads();  // the block is overwritten by the next trip
    }
  }
  // reduce the 4 n-groups (fixed order) -> partial sums of this training-set slice
  __syncthreads();
  double* red = smem;  // reuse: [2][4][64]
  red[g * 64 + m] = mu;
  red[256 + g * 64 + m] = wd;
  __syncthreads();
  if (tid < 64) {
    const double s0 = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
    const double s1 = ((red[256 + tid] + red[320 + tid]) + red[384 + tid]) + red[448 + tid];
    mu_part[(size_t)blockIdx.y * a.Mc + mc0 + tid] = s0;
    w_part[(size_t)blockIdx.y * a.Mc + mc0 + tid] = s1;
  }
  if (PV > 0) {
    // the trend tiles: D[i][j] sits in lane 16 (i % 4) + j, component i / 4 (i = candidate in the fragment, j = column in the tile)
    mfma16_drain();
#pragma unroll
    for (int t = 0; t < NTT; ++t) mfma16_fence(tacc[t]);
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        t_part[((size_t)blockIdx.y * PV + 16 * t + li) * a.Mc + mc0 + 16 * g + 4 * c + lk] = tacc[t][c];
  }
}

// ---------------------------------------------------------------------------------------------------
// Kernel A' (r05, the DEFAULT for the squared-distance kernels without a fused polynomial trend): the same chunk with the
// weighted squared distance formed on the matrix cores.
//   s2(m, n) = |a_m|^2 + |b_n|^2 - 2 a_m . b_n          a = sqrt(theta) x*_m,  b = sqrt(theta) x_n
// The (sub, fma) pair per dimension of kernel A is 2 d FP64 VALU instructions per pair -- half of the producer at C3 -- and an FP64 MFMA
// moves exactly as many flops per clock as the FP64 VALU, so the cross term a . b as a 16 x 16 x 4 matrix product costs d
// FMA-equivalents per pair instead of 2 d, plus three for the assembly of s2.  The price is cancellation: the cross-term form carries an
// ABSOLUTE error of ~sqrt(d) eps (|a|^2 + |b|^2) / 2 where the difference form carries a RELATIVE error of ~d eps.  Hence the guard:
//   a pair with s2 * 64 < |a|^2 + |b|^2 (a candidate within an eighth of the typical distance of a training point; never, for
//   space-filling candidates in d >= 3; routinely, once a BO run concentrates around the incumbent) is recomputed in the difference form,
//   with kernel A's very operations in kernel A's order -- so a candidate ON a training point still gives s2 = 0, r = 1 and a clipped
//   MSE of exactly 0 (the guards of EI / MGFI, acquisition_fun.py:162-164, 274-275, see tests G7), and every pair has s2 to <= ~64 sqrt(d) eps
//   relative.  The branch is wave-uniform (ballot); a wave pays the slow path only for its flagged lanes' values.
// Layout: workgroup = 64 candidates x one slice of the training set (as kernel A); wave g owns training rows 16 g .. 16 g + 15 of every
// 64-row block and all 64 candidates: four 16 x 16 output tiles D[i = row][j = candidate] sharing one A fragment (training rows, a
// 128-byte run of XthT per dimension: L1 / L2 resident) against four B fragments (candidate tile, LDS, k-major: conflict-free).
// v_mfma_f64_16x16x4_f64: A lane 16 k + i, B lane 16 k + j, D[i][j] in lane 16 (i % 4) + j, component i / 4 (probe_mfma_layout).
// ---------------------------------------------------------------------------------------------------
template <int KERNEL>
// (four waves per SIMD: 128 VGPRs, a dozen spilled in the prologue -- 5.40 against 5.62 ms at three waves and 155 VGPRs, C3; profiles/r05_corr_mfma_ab.txt)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_corr_mfma(const double* __restrict__ Xs, const double* __restrict__ sqrt_theta,
                                                   const double* __restrict__ XthT, const double* __restrict__ xnorm,
                                                   const double* __restrict__ gamma, const double* __restrict__ wvec,
                                                   double* __restrict__ rT, double* __restrict__ mu_part, double* __restrict__ w_part,
                                                   CorrDims a) {
#define BOGP_CORR_STORE 1
#include "corr_mfma_body.inc"
#undef BOGP_CORR_STORE
}
// the same producer without the store of r (the one-pass pruned sweep, kernels_prune.hip: the bounding pass needs mu_part / w_part only)
template <int KERNEL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_corr_mfma_sums(const double* __restrict__ Xs, const double* __restrict__ sqrt_theta,
                                                   const double* __restrict__ XthT, const double* __restrict__ xnorm,
                                                   const double* __restrict__ gamma, const double* __restrict__ wvec,
                                                   double* __restrict__ mu_part, double* __restrict__ w_part, CorrDims a) {
#define BOGP_CORR_STORE 0
#include "corr_mfma_body.inc"
#undef BOGP_CORR_STORE
}

#undef BOGP_OPQ
// ---------------------------------------------------------------------------------------------------
// Kernel B: triangular contraction  ss_part[jg][m] = sum_{j in group jg} (sum_{n<=j} V[j][n] r[m][n])^2
// ---------------------------------------------------------------------------------------------------
constexpr int MR = 4;                // 16-row fragments per wave  (64 candidates)
constexpr int NWJ = 4;               // waves per workgroup (along j)
// NR = 16-column fragments per wave (template parameter, 4 in every instantiation): 256 columns per workgroup, 128 accumulator VGPRs.
// (NR = 2 -- 128-column groups, three workgroups per CU -- lost in r01, was never the default and went with its switch in r06.)
constexpr int KB = 32;               // training points per staged block
constexpr int PITCH = 64 + 16;       // LDS row pitch in doubles: 640 B == 128 (mod 256) -> conflict-free A reads

// (r04: the first contraction kernel, k_contract on v_mfma_f64_4x4x4_4b_f64 with AGPR accumulators -- opt-in since r01 through
// BOGP_CONTRACT_MFMA=4x4, 20 % slower than k_contract16 -- was removed: tests/test_isa_lint.py found AGPR spills inside its main loop and an
// accumulator read ahead of its drain in the ROCm 7.2 build.  Its description stays in DESIGN.md section 5.2; the code is in git 26333e7.)

// ---------------------------------------------------------------------------------------------------
// Kernel B': the same contraction on v_mfma_f64_16x16x4_f64.
//
// The first probe of this instruction (builtin, AGPR accumulators) measured half the FP64 rate, which is why kernel B was built on
// the 4x4x4 form; as inline asm with the accumulator in architectural VGPRs it runs at the peak, at 1-4 waves per SIMD (bogp_mfma.h, 1.)
// -- and it needs ONE A register and ONE B register per 2048 flop where the 4x4x4 form needs four rotated A registers: a quarter of
// the LDS reads, no rotation, a quarter of the MFMA issue slots.  Lane layout: bogp_mfma.h (the B order is the one k_pack_V already
// produces).
// Tiling, staging, guards and the epilogue's summation order are those of kernel B.  (The wrapper, the drain and their rules: bogp_mfma.h.)
// (The stamped build of this kernel that produced the MFMA-idle attribution of profiles/r06_contract_att.txt, and the removal experiments of the
// same file, went when kernel B'' below became the default; they are in git 6cdd2df.)
// ---------------------------------------------------------------------------------------------------

// The epilogue idiom of both contraction kernels: the operand-less drain, then a fence on every accumulator (bogp_mfma.h, 3.).
// (BOGP_LINT_NO_DRAIN / BOGP_LINT_NO_FENCE: negative controls of tests/test_isa_lint.py -- builds WITHOUT the drain / the fences must be
// flagged by the ISA lint; never defined in the product build)
template <int MRT, int NR>
__device__ __forceinline__ void contract_drain(d4 (&acc)[MRT][NR]) {
#ifndef BOGP_LINT_NO_DRAIN
  mfma16_drain();
#endif
#ifndef BOGP_LINT_NO_FENCE
#pragma unroll
  for (int mi = 0; mi < MRT; ++mi)
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) mfma16_fence(acc[mi][ni]);
#endif
}

template <int NR, bool GUARDED>
__device__ __forceinline__ void contract_block16(const double* __restrict__ tile, const double2* __restrict__ vp,
                                                 const size_t (&boff)[NR], const int (&jt)[NR], int aoff, int kb, int kp_last,
                                                 double2 (&bq)[4][NR], d4 (&acc)[MR][NR]) {
  // A fragments are read one k-step AHEAD of the MFMAs that use them (two register sets): with only four LDS reads per
  // sixteen MFMAs their latency would otherwise sit in front of every k-step
  double af[2][MR];
#pragma unroll
  for (int mi = 0; mi < MR; ++mi) af[0][mi] = tile[aoff + 16 * mi];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kp = kb * 4 + s;
    const int kb16 = kp >> 1;
    {  // B fragments are requested TWO k-pairs ahead (four slots = the four k-pairs of a block; clamped at the end)
      const int kpn = min(kp + 2, kp_last);
#pragma unroll
      for (int ni = 0; ni < NR; ++ni) bq[(s + 2) & 3][ni] = vp[boff[ni] + (size_t)kpn * 64];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int sub = 2 * s + h;
      if (sub < 7) {
        const double* trow = tile + (4 * (sub + 1)) * PITCH;
#pragma unroll
        for (int mi = 0; mi < MR; ++mi) af[(sub + 1) & 1][mi] = trow[aoff + 16 * mi];
      }
#pragma unroll
      for (int ni = 0; ni < NR; ++ni) {
        if (!GUARDED || kb16 <= jt[ni]) {
          const double bv = h == 0 ? bq[s][ni].x : bq[s][ni].y;
#pragma unroll
          for (int mi = 0; mi < MR; ++mi) mfma16(af[sub & 1][mi], bv, acc[mi][ni]);
        }
      }
    }
  }
}

// NCP != 0 (16 / 32 / 64): the batched one-point path (kernels_point.hip, k_point_rhs_T).  The 64 "candidates" of a workgroup are
// then the right-hand-side columns [r | dr/dx_1 .. dr/dx_d | 0 ..] of 64 / NCP points, NCP columns each, and what a point needs
// from C = V rhs is not |C_c|^2 but the cross products  sum_j C_0[j] C_c[j]  with its FIRST column ((V^T V r) . dr/dx_k =
// (V r) . (V dr/dx_k): one pass over V serves the posterior AND its d input-derivatives, gpr.py:537-576).  Only the epilogue
// differs: the first row of every NCP-row group (fragment head, register 0, lane quarter 0) is broadcast to the other quarters
// and multiplies instead of the square; the sums land as the row-block records k_point_finish reads.
template <int NR, int NCP = 0>
__global__ __launch_bounds__(256, 2) void k_contract16(ContractArgs a) {
  constexpr int JT16 = NWJ * NR;
  __shared__ __attribute__((aligned(16))) double lds[2 * KB * PITCH];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nMt = a.nMt;
  // Column-group-major order, heaviest group first: concurrent workgroups then walk the SAME 256-column panel of V, which
  // stays hot in every XCD's L2 (the B fragments feed the MFMAs straight from global loads).  Measured alternative (r02,
  // tools/ab/ab_contract_order.sh): the nJ groups of one candidate tile back to back on one XCD -- r tiles shared in L2, but the
  // B reads then span all of V (16 MB against 4 MB of L2): 61.5 -> 85.4 ms per step.  r is re-read (nJ + 1) / 2 times instead.
  const int jg = a.nJ - 1 - (int)(blockIdx.x / nMt);
  const int mt = blockIdx.x % nMt;
  const int64_t mc0 = (int64_t)mt * 64;
  if (a.live && mc0 >= *a.live) return;  // pruned sweep: the live row count is on the device, tiles past it have nothing to do
  const int NJ16 = a.NJ16, NKP = a.NKP;
  const int kmax16 = min((jg + 1) * JT16, NJ16);
  const int nkb = kmax16 >> 1;
  const int nkb_full = jg * (JT16 / 2);
  const int kp_last = 2 * kmax16 - 1;

  int jt[NR];
  size_t boff[NR];
  bool valid[NR];
#pragma unroll
  for (int ni = 0; ni < NR; ++ni) {
    // serpentine tile assignment {w, 7-w, 8+w, 15-w}: in the diagonal zone tile t carries t+1 sixteen-row groups, so every
    // wave gets the same 34 of them (the plain interleave w + 4 ni gives wave 3 640 MFMAs against wave 0's 448)
    const int j = jg * JT16 + ((ni & 1) ? NWJ * (ni + 1) - 1 - w : NWJ * ni + w);
    valid[ni] = j < NJ16;
    jt[ni] = valid[ni] ? j : -1;
    boff[ni] = (size_t)min(j, NJ16 - 1) * NKP * 64;
  }

  d4 acc[MR][NR];
#pragma unroll
  for (int mi = 0; mi < MR; ++mi)
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};

  const int srow = tid >> 5;
  const int scol = (tid & 31) * 2;
  const double* __restrict__ rbase = a.rT + mc0 + scol;
  const size_t Mc = (size_t)a.Mc;
  // Two register sets for the staged r tiles: tile kb + 2 is requested while tile kb is contracted and tile kb + 1 (requested one
  // block earlier) is written to LDS at the END of the block -- every load has TWO blocks of MFMA work to arrive.  With one
  // set (one block of cover) the half-empty blocks of the diagonal zone no longer hid the ~2 us round trip to HBM.
  double2 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
#define BOGP_STAGE_LOAD(S, kb_)                                                                      \
  do {                                                                                               \
    const double* p_ = rbase + (size_t)((kb_)*KB + srow) * Mc;                                       \
    S##0 = *reinterpret_cast<const double2*>(p_);                                                    \
    S##1 = *reinterpret_cast<const double2*>(p_ + 8 * Mc);                                           \
    S##2 = *reinterpret_cast<const double2*>(p_ + 16 * Mc);                                          \
    S##3 = *reinterpret_cast<const double2*>(p_ + 24 * Mc);                                          \
  } while (0)
#define BOGP_STAGE_STORE(S, buf_)                                                                    \
  do {                                                                                               \
    double* q_ = &lds[(buf_)*KB * PITCH + srow * PITCH + scol];                                      \
    *reinterpret_cast<double2*>(q_) = S##0;                                                          \
    *reinterpret_cast<double2*>(q_ + 8 * PITCH) = S##1;                                              \
    *reinterpret_cast<double2*>(q_ + 16 * PITCH) = S##2;                                             \
    *reinterpret_cast<double2*>(q_ + 24 * PITCH) = S##3;                                             \
  } while (0)

  const double2* __restrict__ vp = a.Vp + lane;
  double2 bq[4][NR];
#pragma unroll
  for (int ni = 0; ni < NR; ++ni) {
    bq[0][ni] = vp[boff[ni]];
    bq[1][ni] = vp[boff[ni] + (size_t)min(1, kp_last) * 64];
  }

  // A lane = 16 k + i reads row k of the k-step, candidate 16 mi + i: pitch 640 B puts the four rows of a read in four
  // different 128-byte bank groups
  const int aoff = (lane >> 4) * PITCH + (lane & 15);

  BOGP_STAGE_LOAD(sa, 0);
  BOGP_STAGE_STORE(sa, 0);
  BOGP_STAGE_LOAD(sa, min(1, nkb - 1));  // tile 1 -> set A (stored at the end of block 0)

  // Two loops, one body each (r06): the full blocks run WITHOUT the per-tile guards -- as one code path with a run-time guard the compiler put a
  // compare / select / branch chain in front of every four MFMAs of the full blocks too and moved three of the four tile groups out of line
  // (six taken branches a k-step); an if / else of the two bodies inside ONE loop made the register allocator shuffle the 128 accumulators
  // (734 spills).  nkb_full = 8 jg is even, so the zone starts on buffer 0.
#define BOGP_BLOCK_PAIR(G)                                                                           \
  do {                                                                                               \
    __syncthreads(); /* tile kb is in lds[0]; every wave is done with lds[1] */                      \
    BOGP_STAGE_LOAD(sb, min(kb + 2, nkb - 1));                                                       \
    contract_block16<NR, G>(&lds[0], vp, boff, jt, aoff, kb, kp_last, bq, acc);                      \
    BOGP_STAGE_STORE(sa, 1); /* tile kb + 1 */                                                       \
    if (kb + 1 >= nkb) break;                                                                        \
    __syncthreads(); /* tile kb + 1 is in lds[1]; every wave is done with lds[0] */                  \
    BOGP_STAGE_LOAD(sa, min(kb + 3, nkb - 1));                                                       \
    contract_block16<NR, G>(&lds[KB * PITCH], vp, boff, jt, aoff, kb + 1, kp_last, bq, acc);         \
    BOGP_STAGE_STORE(sb, 0); /* tile kb + 2 */                                                       \
  } while (0)
  int kb = 0;
  for (; kb < nkb_full; kb += 2) BOGP_BLOCK_PAIR(false);
  for (; kb < nkb; kb += 2) BOGP_BLOCK_PAIR(true);
#undef BOGP_BLOCK_PAIR
#undef BOGP_STAGE_LOAD
#undef BOGP_STAGE_STORE

  // ---- epilogue: D[i][j] sits in lane 16 (i % 4) + j, register i / 4 ---------------------------------
  contract_drain(acc);
  __syncthreads();
  // red[slot][wave][row] with a row pitch of 65 doubles: the writes (lanes = 4 rows x 16 slots) fall on (4 slot + row)
  // mod 32 = every bank pair twice, the reads (lanes = 64 consecutive rows) are conflict free.  (The first layout,
  // [wave][row][slot], made every read a 64-way bank conflict: 13.7k cycles of epilogue per workgroup.)
  constexpr int RP = 65;
  double* red = lds;                    // [16 slots][NWJ][RP]
  double* red2 = lds + 16 * NWJ * RP;   // [NWJ][64]: per-wave partial sums
  const int q = lane >> 4, jc = lane & 15;
  if constexpr (NCP == 0) {
#pragma unroll
    for (int mi = 0; mi < MR; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double s = 0.0;
#pragma unroll
        for (int ni = 0; ni < NR; ++ni)
          if (valid[ni]) s = __builtin_fma(acc[mi][ni][r], acc[mi][ni][r], s);
        red[(jc * NWJ + w) * RP + 16 * mi + 4 * r + q] = s;  // slot = column inside the 16-tile
      }
  } else {
    constexpr int FPG = NCP / 16;  // fragments per point
    double head[MR / FPG][NR];     // row 0 of each point, for this lane's column jc: D[16 mi0][jc] = lane jc, register 0
#pragma unroll
    for (int g = 0; g < MR / FPG; ++g)
#pragma unroll
      for (int ni = 0; ni < NR; ++ni) head[g][ni] = __shfl(acc[g * FPG][ni][0], jc);
#pragma unroll
    for (int mi = 0; mi < MR; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        double s = 0.0;
#pragma unroll
        for (int ni = 0; ni < NR; ++ni)
          if (valid[ni]) s = __builtin_fma(acc[mi][ni][r], head[mi / FPG][ni], s);
        red[(jc * NWJ + w) * RP + 16 * mi + 4 * r + q] = s;
      }
  }
  __syncthreads();
  {  // every thread adds the 16 slots of one (wave, row) in a fixed order, then 64 threads add the four waves
    double s = 0.0;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) s += red[(sl * NWJ + w) * RP + lane];
    red2[w * 64 + lane] = s;
  }
  __syncthreads();
  if (tid < 64) {
    const double tot = ((red2[tid] + red2[64 + tid]) + red2[128 + tid]) + red2[192 + tid];
    if constexpr (NCP == 0) {
      a.ss_part[(size_t)jg * a.Mc + mc0 + tid] = tot;
    } else {  // record 1 + jg of point b: [0][c] = sum over this column group of C_0 C_c  (k_point_finish adds the groups)
      const int64_t m = mc0 + tid;
      const int64_t b = m / NCP;
      const int c = (int)(m - b * NCP);
      if (b < a.cross_B) a.ss_part[((size_t)b * (a.nJ + 1) + 1 + jg) * (2 * NCP) + c] = tot;
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Kernel B'' (r06): the same contraction with NO LDS and NO barrier in the main loop.
//
// profiles/r06_contract_att.txt: in k_contract16 ONE wave does not keep its SIMD's MFMA pipe full -- the A reads (LDS) end up just in
// front of the MFMAs that use them, the B fragments (L2) retire behind the stage loads (HBM) on the in-order vmcnt, and whenever one of
// the two resident waves waits at the per-block barrier or stores its stage registers the pipe runs at what the other wave manages
// alone.  Here every wave fetches its own operands: the A fragment of a k-step is 4 rows x 16 candidates = four 128-byte runs of rT,
// read as ONE global_load_dwordx4 per PAIR of fragments (lane (k, i) takes candidates 2 i and 2 i + 1 of a 32-candidate half: fragment
// mi = 2 half + e holds candidates 32 half + 2 i + e -- any bijection of fragment rows onto candidates will do, the epilogue knows it),
// the B fragments as before.  A and B of k-pair t + DD are requested before k-pair t is multiplied (DD + 1 register slots of
// 32 VGPRs beside the 128 accumulators), the four waves of a workgroup run free of each other (the sibling waves' A requests hit
// L1 / L2 behind the first one) and meet only in the epilogue, which is k_contract16's and adds in the same order: the sums are
// bit-identical to k_contract16's.
// Measured and settled (profiles/r06_contract_direct_ab.txt, contract ms per sweep at C3 against 58.4 - 58.6 for the first version of this kernel; the build switches
// of these experiments are in git 6cdd2df): ONE k-pair in flight 58.7; non-temporal A loads 61.4, non-temporal B loads 59.2; no reduction
// epilogue 58.3.  Removal experiments (wrong sums, priced only): no diagonal zone 50.1, every A pair / every B fragment from the tile's first
// k-pair (cache-hot) 57.1 / 56.4, both 55.3.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 ld2_plain(const char* p) { return *reinterpret_cast<const double2*>(p); }
constexpr int DD = 2;       // k-pairs in flight
constexpr int DR = DD + 1;  // register slots

#ifdef CONTRACT_D_TRACE
// (profiling builds only, -DCONTRACT_D_TRACE: shader-clock stamps of every wave -- entry, loop start, the start of EVERY k-pair, loop end, drain, reduction, exit --
// parked in LDS and written out at the end; tools/contract_d_trace.py -> profiles/r06_contract_d_trace.txt.  A k-pair's stamp is requested in front of its first load
// and waited for / stored behind its first four MFMAs, so that the scalar-memory round trip of s_memtime hides under matrix work.)
constexpr int DT_NST = 8 + 264;  // words per wave: 8 header + one per k-pair (N <= 2112)
#define BOGP_DT_NOW(idx_)                                                            \
  do {                                                                               \
    unsigned long long t_;                                                           \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_));                 \
    dtr[(idx_)] = t_;                                                                \
  } while (0)
#define BOGP_DT_ISSUE() asm volatile("s_memtime %0" : "=s"(dt_pending))
#define BOGP_DT_STORE(idx_)                                                          \
  do {                                                                               \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(dt_pending));                         \
    if ((idx_) < DT_NST) dtr[(idx_)] = dt_pending;                                   \
  } while (0)
__global__ __launch_bounds__(256, 2) void k_contract16d(ContractArgs a, unsigned long long* trace_out) {
#else
#define BOGP_DT_NOW(idx_) ((void)0)
#define BOGP_DT_ISSUE() ((void)0)
#define BOGP_DT_STORE(idx_) ((void)0)
__global__ __launch_bounds__(256, 2) void k_contract16d(ContractArgs a) {
#endif
  constexpr int NR = 4;
  constexpr int JT16 = NWJ * NR;
  constexpr int RP = 65;
  __shared__ __attribute__((aligned(16))) double lds[16 * NWJ * RP + NWJ * 64];  // the epilogue's reduction arrays only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
#ifdef CONTRACT_D_TRACE
  __shared__ unsigned long long dtr_all[NWJ][DT_NST];
  unsigned long long* dtr = dtr_all[w];
  unsigned long long dt_pending = 0;
  {
    unsigned hwid, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    dtr[0] = (unsigned long long)hwid | ((unsigned long long)xcc << 32);
  }
  BOGP_DT_NOW(1);
#endif
  const int nMt = a.nMt;
  const int jg = a.nJ - 1 - (int)(blockIdx.x / nMt);  // heaviest column group first (k_contract16)
  const int mt = blockIdx.x % nMt;
  const int64_t mc0 = (int64_t)mt * 64;
  if (a.live && mc0 >= *a.live) return;  // pruned sweep (k_contract16): wave-uniform, before any load
  const int NJ16 = a.NJ16, NKP = a.NKP;
  const int kmax16 = min((jg + 1) * JT16, NJ16);
  const int nkp_full = 2 * jg * JT16;    // k-pairs without a guard
  // k-pairs of this WAVE: its last tile (15 - w of the group, serpentine below) ends 2 w k-pairs before the group does -- the waves do not
  // wait for each other before the epilogue, so a wave that has nothing left to multiply stops requesting operands too
  const int nkp = min(2 * kmax16, max(2 * ((jg + 1) * JT16 - w), 2));
  const int kp_last = nkp - 1;

  int jt[NR];
  bool valid[NR];
  const char* vb[NR];
#pragma unroll
  for (int ni = 0; ni < NR; ++ni) {
    const int j = jg * JT16 + ((ni & 1) ? NWJ * (ni + 1) - 1 - w : NWJ * ni + w);  // serpentine (k_contract16)
    valid[ni] = j < NJ16;
    jt[ni] = valid[ni] ? j : -1;
    vb[ni] = reinterpret_cast<const char*>(a.Vp + (size_t)min(j, NJ16 - 1) * NKP * 64);
  }
  const size_t Mc = (size_t)a.Mc;
  const char* ab = reinterpret_cast<const char*>(a.rT + mc0);
  const size_t kp_stride = 8 * Mc * sizeof(double);                                                    // 8 rows a k-pair
  unsigned voffA0 = (unsigned)(((size_t)(lane >> 4) * Mc + 2 * (lane & 15)) * sizeof(double));   // k-step 0 of the pair
  unsigned voffA1 = voffA0 + (unsigned)(4 * Mc * sizeof(double));                                // k-step 1
  unsigned voffB = (unsigned)lane * 16u;

  d4 acc[MR][NR];
#pragma unroll
  for (int mi = 0; mi < MR; ++mi)
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};

  double2 av[DR][2][2], bv[DR][NR];
  // load g of a k-pair, in the order the groups below need them (a group waits for the loads up to its own, vmcnt retires in order):
  // 0, 1 = the A pairs of k-step 0 (candidate halves 0 / 1), 2 .. 5 = the B fragments of tiles 0 .. 3, 6, 7 = the A pairs of k-step 1
#define BOGP_D_LOAD1(slot, g, ap_, kpc_, vb_)                                                                         \
  do {                                                                                                                \
    if ((g) < 2) av[slot][0][(g) & 1] = ld2_plain((ap_) + voffA0 + (((g) & 1) ? 256 : 0));                            \
    else if ((g) >= 6) av[slot][1][(g) & 1] = ld2_plain((ap_) + voffA1 + (((g) & 1) ? 256 : 0));                      \
    else bv[slot][(g) - 2] = ld2_plain((vb_)[(g) - 2] + (size_t)(kpc_) * 1024 + voffB);                               \
  } while (0)
  // The eight loads of k-pair kp_ + DD go out as ONE block in front of the 32 MFMAs of k-pair kp_ (the first version of this kernel sent load g in front of
  // group g).  The phase trace (profiles/r06_contract_d_trace.txt) showed a FULL k-pair taking 4284 cycles where the two waves of a SIMD need 4096: every
  // hand-over of the issue port between them costs a few cycles, and a load between two groups of MFMAs is a hand-over.  58.4 -> 58.0 ms.
  // NO VALU IN THE LOOP: the address of every load is a scalar base (advanced by scalar arithmetic) + the lane's constant 32-bit offset, the `v_offset, s[base]`
  // form of global_load.  hipcc only selects that form when it sees the zero-extension of the offset next to the load; hoisted out of the loop (it is loop
  // invariant) the offset is a 64-bit register pair and every load gets a v_lshl_add_u64 -- a 64-bit VALU operation, i.e. one that runs on the SAME FP64 pipe as
  // the MFMAs: eight of them per k-pair and wave.  Passing the three offsets through an empty asm inside the loop keeps the zero-extension where the load is.
  // 58.0 -> 55.9 ms a step at C3 (0.917 -> 0.956 of peak), 454.9 -> 439.1 ms at C5 (profiles/r06_contract_d_trace.txt).
  // one k-pair: 8 groups of 4 MFMAs (k-step h = g / 4, tile ni = g % 4), the eight loads in front of group 0; the sched_barriers pin that order.
  // (The loads stay INSIDE the group loop: hoisted in front of it the compiler orders the scalar code of the k-pair differently.)
#define BOGP_D_KPAIR(G, u, kp_)                                                                                       \
  do {                                                                                                                \
    const int kpc_ = min((kp_) + DD, kp_last);                                                                        \
    const char* ap_ = ab + (size_t)kpc_ * kp_stride;                                                                  \
    const int k16_ = (kp_) >> 1;                                                                                      \
    asm volatile("" : "+v"(voffA0), "+v"(voffA1), "+v"(voffB));                                                       \
    /* diagonal zone: a tile that is past its diagonal at k-pair kpc_ needs no fragment -- its request goes to the address */ \
    /* of the wave's last tile instead (an L1 hit on a line that is on its way anyway, no second L2 request)            */ \
    const char* vbe_[NR];                                                                                             \
    _Pragma("unroll") for (int ni = 0; ni < NR; ++ni) vbe_[ni] = (!(G) || ((kpc_ >> 1) <= jt[ni])) ? vb[ni] : vb[NR - 1]; \
    BOGP_DT_ISSUE();                                                                                                  \
    _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                                   \
      if (g == 1) BOGP_DT_STORE(8 + (kp_));                                                                           \
      if (g == 0) {                                                                                                   \
        _Pragma("unroll") for (int l_ = 0; l_ < 8; ++l_) BOGP_D_LOAD1(((u) + DD) % DR, l_, ap_, kpc_, vbe_);          \
      }                                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
      if (!(G) || k16_ <= jt[g & 3]) {                                                                                \
        const double b_ = (g >> 2) == 0 ? bv[u][g & 3].x : bv[u][g & 3].y;                                            \
        _Pragma("unroll") for (int mi = 0; mi < MR; ++mi)                                                             \
          mfma16((mi & 1) ? av[u][g >> 2][mi >> 1].y : av[u][g >> 2][mi >> 1].x, b_, acc[mi][g & 3]);             \
      }                                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
    }                                                                                                                 \
  } while (0)

#pragma unroll
  for (int t = 0; t < DD; ++t) {
    const int kpc = min(t, kp_last);
    const char* ap = ab + (size_t)kpc * kp_stride;
#pragma unroll
    for (int g = 0; g < 8; ++g) BOGP_D_LOAD1(t, g, ap, kpc, vb);
  }

  BOGP_DT_NOW(2);
  int kp = 0;
  // full k-pairs, DR at a time (static register slots); what is left of them goes through the guarded loop (its guards hold there)
  for (; kp + DR <= nkp_full; kp += DR) {
#pragma unroll
    for (int u = 0; u < DR; ++u) BOGP_D_KPAIR(false, u, kp + u);
  }
  for (; kp < nkp; kp += DR) {
#pragma unroll
    for (int u = 0; u < DR; ++u)
      if (kp + u < nkp) BOGP_D_KPAIR(true, u, kp + u);
  }
#undef BOGP_D_KPAIR
#undef BOGP_D_LOAD1
  BOGP_DT_NOW(3);

  // ---- epilogue (k_contract16's): D[i][j] sits in lane 16 (i % 4) + j, register i / 4; row i of fragment mi = candidate
  // 32 (mi / 2) + 2 i + (mi % 2)
  contract_drain(acc);
  BOGP_DT_NOW(4);
  double* red = lds;                    // [16 slots][NWJ][RP]
  double* red2 = lds + 16 * NWJ * RP;   // [NWJ][64]: per-wave partial sums
  const int q = lane >> 4, jc = lane & 15;
#pragma unroll
  for (int mi = 0; mi < MR; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s = 0.0;
#pragma unroll
      for (int ni = 0; ni < NR; ++ni)
        if (valid[ni]) s = __builtin_fma(acc[mi][ni][r], acc[mi][ni][r], s);
      red[(jc * NWJ + w) * RP + 32 * (mi >> 1) + 2 * (4 * r + q) + (mi & 1)] = s;  // slot = column inside the 16-tile
    }
  // the wave's own slots: no workgroup barrier needed between its writes and its reads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  {
    double s = 0.0;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) s += red[(sl * NWJ + w) * RP + lane];
    red2[w * 64 + lane] = s;
  }
  BOGP_DT_NOW(5);
  __syncthreads();
  if (tid < 64) {
    const double tot = ((red2[tid] + red2[64 + tid]) + red2[128 + tid]) + red2[192 + tid];
    a.ss_part[(size_t)jg * a.Mc + mc0 + tid] = tot;
  }
#ifdef CONTRACT_D_TRACE
  BOGP_DT_NOW(6);
  dtr[7] = (unsigned long long)nkp | ((unsigned long long)nkp_full << 32);
  __syncthreads();
  if (trace_out) {
    unsigned long long* dst = trace_out + (size_t)blockIdx.x * (NWJ * DT_NST);
    const unsigned long long* src = &dtr_all[0][0];
    for (int i = tid; i < NWJ * DT_NST; i += 256) dst[i] = src[i];
  }
#endif
}
#undef BOGP_DT_NOW
#undef BOGP_DT_ISSUE
#undef BOGP_DT_STORE

// ---------------------------------------------------------------------------------------------------
// Kernel B'' with a narrower candidate tile: 16 MRN = 32 or 16 candidates a workgroup instead of 64 (DESIGN.md 5.2''').
//
// A launch of kernel B'' with few candidate tiles is bound by ONE workgroup's walk over the heaviest 256-column group: at N = 2048 that is 256 k-pairs x
// 32 MFMAs x 64 cycles = 0.22 ms however few rows there are, with most of the chip idle (the survivors' round of a pruned sweep: 13 x 8 workgroups on 256
// CUs).  With MRN fragments a wave the chain is MRN / 4 as long and the grid 4 / MRN as large; every workgroup still reads all of its column group's V, so
// the V bytes per row grow by the same factor (from L2 and the Infinity Cache) -- which is why launch_contract only takes this kernel while the 64-row
// grid leaves the chip idle (contract_tile_rows, bogp_internal.h).
// The column side is kernel B'' unchanged: four waves x NR = 4 tiles in serpentine order, the guarded diagonal zone, the per-wave early stop, the
// `v_offset, s[base]` loads with the empty asm that keeps them, the sched_barriers, ss_part[jg][m].  The A fragment of a k-step is ONE load a lane: a
// double2 (lane (k, i): candidates 2 i and 2 i + 1 -- fragment e holds candidate 2 i + e) for 32 rows, a double (candidate i) for 16: 256- / 128-byte
// runs of rT.  A k-pair is six loads in front of 8 MRN MFMAs; the 64 / 32 accumulator registers leave room for DDN k-pairs in flight.
// WHY NO BIT CAN CHANGE: rows of the contraction are independent.  Element D[i][j] of a fragment is the same k-ordered chain of matrix instructions from
// zero whatever other fragments the wave holds, and the order in which a row's columns are added -- ni within a lane, then the 16 slots, then the four
// waves, then jg in k_acquisition -- belongs to the column side.  ss_part, hence MSE, every criterion value and every winner, is bit-identical at 16, 32
// and 64 rows a tile; a difference is a bug, not rounding (tests/test_gpu_contract_tile.py).
// ---------------------------------------------------------------------------------------------------
template <int MRN> struct ContractAFrag;
template <> struct ContractAFrag<1> { typedef double type; };
template <> struct ContractAFrag<2> { typedef double2 type; };
__device__ __forceinline__ double afrag_row(double a, int) { return a; }
__device__ __forceinline__ double afrag_row(const double2& a, int mi) { return mi ? a.y : a.x; }

template <int MRN, int DDN, int WPE>
__global__ __launch_bounds__(256, WPE) void k_contract16n(ContractArgs a) {
  constexpr int NR = 4;
  constexpr int JT16 = NWJ * NR;
  constexpr int ROWS = 16 * MRN;  // candidates a workgroup
  constexpr int RP = ROWS + 1;
  constexpr int DRN = DDN + 1;    // register slots
  typedef typename ContractAFrag<MRN>::type afrag;
  __shared__ __attribute__((aligned(16))) double lds[16 * NWJ * RP + NWJ * ROWS];  // the epilogue's reduction arrays only

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nMt = a.nMt * (64 / ROWS);                // a.nMt counts 64-row tiles
  const int jg = a.nJ - 1 - (int)(blockIdx.x / nMt);  // heaviest column group first (k_contract16)
  const int mt = blockIdx.x % nMt;
  const int64_t mc0 = (int64_t)mt * ROWS;
  if (a.live && mc0 >= *a.live) return;  // (launch_contract keeps the gated launches on 64 rows; kept for the same meaning of the argument)
  const int NJ16 = a.NJ16, NKP = a.NKP;
  const int kmax16 = min((jg + 1) * JT16, NJ16);
  const int nkp_full = 2 * jg * JT16;    // k-pairs without a guard
  const int nkp = min(2 * kmax16, max(2 * ((jg + 1) * JT16 - w), 2));  // k-pairs of this WAVE (k_contract16d)
  const int kp_last = nkp - 1;

  int jt[NR];
  bool valid[NR];
  const char* vb[NR];
#pragma unroll
  for (int ni = 0; ni < NR; ++ni) {
    const int j = jg * JT16 + ((ni & 1) ? NWJ * (ni + 1) - 1 - w : NWJ * ni + w);  // serpentine (k_contract16)
    valid[ni] = j < NJ16;
    jt[ni] = valid[ni] ? j : -1;
    vb[ni] = reinterpret_cast<const char*>(a.Vp + (size_t)min(j, NJ16 - 1) * NKP * 64);
  }
  const size_t Mc = (size_t)a.Mc;
  const char* ab = reinterpret_cast<const char*>(a.rT + mc0);
  const size_t kp_stride = 8 * Mc * sizeof(double);                                                      // 8 rows a k-pair
  unsigned voffA0 = (unsigned)(((size_t)(lane >> 4) * Mc + MRN * (lane & 15)) * sizeof(double));   // k-step 0 of the pair (below k_contract16d's offsets)
  unsigned voffA1 = voffA0 + (unsigned)(4 * Mc * sizeof(double));                                  // k-step 1
  unsigned voffB = (unsigned)lane * 16u;

  d4 acc[MRN][NR];
#pragma unroll
  for (int mi = 0; mi < MRN; ++mi)
#pragma unroll
    for (int ni = 0; ni < NR; ++ni) acc[mi][ni] = (d4){0.0, 0.0, 0.0, 0.0};

  afrag av[DRN][2];
  double2 bv[DRN][NR];
  // load g of a k-pair, in the order the groups need them: 0 = the A fragments of k-step 0, 1 .. 4 = the B fragments of tiles 0 .. 3, 5 = the A fragments of k-step 1
#define BOGP_N_LOAD1(slot, g, ap_, kpc_, vb_)                                                                         \
  do {                                                                                                                \
    if ((g) == 0) av[slot][0] = *reinterpret_cast<const afrag*>((ap_) + voffA0);                                      \
    else if ((g) == 5) av[slot][1] = *reinterpret_cast<const afrag*>((ap_) + voffA1);                                 \
    else bv[slot][(g) - 1] = ld2_plain((vb_)[(g) - 1] + (size_t)(kpc_) * 1024 + voffB);                               \
  } while (0)
  // one k-pair: 8 groups of MRN MFMAs (k-step h = g / 4, tile ni = g % 4), the six loads of k-pair kp_ + DDN as one block in front of group 0, the offsets
  // through the empty asm, the zone's dead requests sent to the wave's last tile: all as in k_contract16d, whose comments give the measurements
#define BOGP_N_KPAIR(G, u, kp_)                                                                                       \
  do {                                                                                                                \
    const int kpc_ = min((kp_) + DDN, kp_last);                                                                       \
    const char* ap_ = ab + (size_t)kpc_ * kp_stride;                                                                  \
    const int k16_ = (kp_) >> 1;                                                                                      \
    asm volatile("" : "+v"(voffA0), "+v"(voffA1), "+v"(voffB));                                                       \
    const char* vbe_[NR];                                                                                             \
    _Pragma("unroll") for (int ni = 0; ni < NR; ++ni) vbe_[ni] = (!(G) || ((kpc_ >> 1) <= jt[ni])) ? vb[ni] : vb[NR - 1]; \
    _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                                   \
      if (g == 0) {                                                                                                   \
        _Pragma("unroll") for (int l_ = 0; l_ < 6; ++l_) BOGP_N_LOAD1(((u) + DDN) % DRN, l_, ap_, kpc_, vbe_);        \
      }                                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
      if (!(G) || k16_ <= jt[g & 3]) {                                                                                \
        const double b_ = (g >> 2) == 0 ? bv[u][g & 3].x : bv[u][g & 3].y;                                            \
        _Pragma("unroll") for (int mi = 0; mi < MRN; ++mi) mfma16(afrag_row(av[u][g >> 2], mi), b_, acc[mi][g & 3]);  \
      }                                                                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                              \
    }                                                                                                                 \
  } while (0)

#pragma unroll
  for (int t = 0; t < DDN; ++t) {
    const int kpc = min(t, kp_last);
    const char* ap = ab + (size_t)kpc * kp_stride;
#pragma unroll
    for (int g = 0; g < 6; ++g) BOGP_N_LOAD1(t, g, ap, kpc, vb);
  }

  int kp = 0;
  // full k-pairs, DRN at a time (static register slots); what is left of them goes through the guarded loop (its guards hold there)
  for (; kp + DRN <= nkp_full; kp += DRN) {
#pragma unroll
    for (int u = 0; u < DRN; ++u) BOGP_N_KPAIR(false, u, kp + u);
  }
  for (; kp < nkp; kp += DRN) {
#pragma unroll
    for (int u = 0; u < DRN; ++u)
      if (kp + u < nkp) BOGP_N_KPAIR(true, u, kp + u);
  }
#undef BOGP_N_KPAIR
#undef BOGP_N_LOAD1

  // ---- epilogue (k_contract16's): D[i][j] sits in lane 16 (i % 4) + j, register i / 4; row i of fragment mi = candidate MRN i + mi
  contract_drain(acc);
  double* red = lds;                    // [16 slots][NWJ][RP]
  double* red2 = lds + 16 * NWJ * RP;   // [NWJ][ROWS]: per-wave partial sums
  const int q = lane >> 4, jc = lane & 15;
#pragma unroll
  for (int mi = 0; mi < MRN; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double s = 0.0;
#pragma unroll
      for (int ni = 0; ni < NR; ++ni)
        if (valid[ni]) s = __builtin_fma(acc[mi][ni][r], acc[mi][ni][r], s);
      red[(jc * NWJ + w) * RP + MRN * (4 * r + q) + mi] = s;  // slot = column inside the 16-tile
    }
  // the wave's own slots: no workgroup barrier needed between its writes and its reads
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane < ROWS) {
    double s = 0.0;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) s += red[(sl * NWJ + w) * RP + lane];
    red2[w * ROWS + lane] = s;
  }
  __syncthreads();
  if (tid < ROWS) {
    const double tot = ((red2[tid] + red2[ROWS + tid]) + red2[2 * ROWS + tid]) + red2[3 * ROWS + tid];
    a.ss_part[(size_t)jg * a.Mc + mc0 + tid] = tot;
  }
}

// ---------------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------------
// the kernels launch_corr_chunk serves with kernel A' (the squared-distance kernels without a fused trend; against kernel A everywhere:
// profiles/r05_corr_mfma_ab.txt) -- the producer that also exists without the store of r (CorrArgs::store = false)
static bool corr_sqdist_kernel(int kernel) {
  return kernel == BOGP_KERNEL_SE || kernel == BOGP_KERNEL_MATERN12 || kernel == BOGP_KERNEL_MATERN32 || kernel == BOGP_KERNEL_MATERN52;
}
bool corr_chunk_without_store(int kernel, int pv, bool have_xnorm) { return corr_sqdist_kernel(kernel) && pv == 0 && have_xnorm; }

hipError_t launch_corr_chunk(int kernel, const CorrArgs& a, int nMt, int S, hipStream_t st) {
  dim3 grid((unsigned)nMt, (unsigned)S);
  // (the general-nu Matern kernel is a squared-distance kernel too, but its profile -- K_nu: hundreds of operations a pair -- dwarfs the distance and
  // needs 270 VGPRs: it stays on kernel A, which holds it without spills)
  if (corr_chunk_without_store(kernel, a.pv, a.xnorm != nullptr)) {
    const int KS = (a.d + 3) / 4;
    const size_t shm = (size_t)max(4 * KS * 64, 2048) * sizeof(double);  // <= 160 KB up to d = 320, like kernel A
    CorrDims dm{a.M, a.m0, a.Mc, a.d, a.Np, a.nblk_per_split, a.wld};
#define BOGP_LAUNCH_CORR_MFMA(K)                                                                                                      \
  do {                                                                                                                                \
    if (shm > 64 * 1024) {                                                                                                            \
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_corr_mfma<K>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                          (int)shm);                                                                                  \
      if (e_ != hipSuccess) return e_;                                                                                                \
    }                                                                                                                                 \
    hipLaunchKernelGGL((k_corr_mfma<K>), grid, 256, shm, st, a.Xs, a.sqrt_theta, a.XthT, a.xnorm, a.gamma, a.wvec, a.rT, a.mu_part,   \
                       a.w_part, dm);                                                                                                 \
  } while (0)
#define BOGP_LAUNCH_CORR_SUMS(K)                                                                                                      \
  do {                                                                                                                                \
    if (shm > 64 * 1024) {                                                                                                            \
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_corr_mfma_sums<K>),                                        \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                                      \
      if (e_ != hipSuccess) return e_;                                                                                                \
    }                                                                                                                                 \
    hipLaunchKernelGGL((k_corr_mfma_sums<K>), grid, 256, shm, st, a.Xs, a.sqrt_theta, a.XthT, a.xnorm, a.gamma, a.wvec, a.mu_part,    \
                       a.w_part, dm);                                                                                                 \
  } while (0)
    if (!a.store) {
      switch (kernel) {
        case BOGP_KERNEL_SE: BOGP_LAUNCH_CORR_SUMS(BOGP_KERNEL_SE); break;
        case BOGP_KERNEL_MATERN12: BOGP_LAUNCH_CORR_SUMS(BOGP_KERNEL_MATERN12); break;
        case BOGP_KERNEL_MATERN32: BOGP_LAUNCH_CORR_SUMS(BOGP_KERNEL_MATERN32); break;
        default: BOGP_LAUNCH_CORR_SUMS(BOGP_KERNEL_MATERN52); break;
      }
      return hipGetLastError();
    }
    switch (kernel) {
      case BOGP_KERNEL_SE: BOGP_LAUNCH_CORR_MFMA(BOGP_KERNEL_SE); break;
      case BOGP_KERNEL_MATERN12: BOGP_LAUNCH_CORR_MFMA(BOGP_KERNEL_MATERN12); break;
      case BOGP_KERNEL_MATERN32: BOGP_LAUNCH_CORR_MFMA(BOGP_KERNEL_MATERN32); break;
      default: BOGP_LAUNCH_CORR_MFMA(BOGP_KERNEL_MATERN52); break;
    }
#undef BOGP_LAUNCH_CORR_MFMA
#undef BOGP_LAUNCH_CORR_SUMS
    return hipGetLastError();
  }
  if (!a.store) return hipErrorInvalidValue;  // (kernel A always stores: corr_chunk_without_store() is false for it)
  size_t shm = (size_t)(max(64 * a.d, 512) + (a.pv > 0 ? 32 * 64 : 0)) * sizeof(double);
  CorrDims dm{a.M, a.m0, a.Mc, a.d, a.Np, a.nblk_per_split, a.wld};
  // the candidate tile is 64 x d doubles of dynamic LDS: above the 64 KB default (d > 128) the kernel has to be allowed
  // more, up to the CU's 160 KB (d <= 320; occupancy then drops to one workgroup per CU, which only matters for the
  // ~10 % of the sweep this producer accounts for)
#define BOGP_LAUNCH_CORR_PV(K, PV)                                                                                       \
  do {                                                                                                                   \
    if (shm > 64 * 1024) {                                                                                               \
      hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_corr_chunk<K, PV>),                           \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);                         \
      if (e_ != hipSuccess) return e_;                                                                                   \
    }                                                                                                                    \
    hipLaunchKernelGGL((k_corr_chunk<K, PV>), grid, 256, shm, st, a.Xs, a.sqrt_theta, a.XthT, a.gamma, a.wvec, a.rT, a.mu_part, \
                       a.w_part, a.Wrow, a.t_part, dm);                                                                  \
  } while (0)
#define BOGP_LAUNCH_CORR(K)                                    \
  do {                                                         \
    if (a.pv == 0) BOGP_LAUNCH_CORR_PV(K, 0);                  \
    else if (a.pv == 16) BOGP_LAUNCH_CORR_PV(K, 16);           \
    else if (a.pv == 32) BOGP_LAUNCH_CORR_PV(K, 32);           \
    else return hipErrorInvalidValue;                          \
  } while (0)
  switch (kernel) {
    case BOGP_KERNEL_SE: BOGP_LAUNCH_CORR(BOGP_KERNEL_SE); break;
    case BOGP_KERNEL_MATERN12: BOGP_LAUNCH_CORR(BOGP_KERNEL_MATERN12); break;
    case BOGP_KERNEL_MATERN32: BOGP_LAUNCH_CORR(BOGP_KERNEL_MATERN32); break;
    case BOGP_KERNEL_ABSEXP: BOGP_LAUNCH_CORR(BOGP_KERNEL_ABSEXP); break;
    case BOGP_KERNEL_CUBIC: BOGP_LAUNCH_CORR(BOGP_KERNEL_CUBIC); break;
    case BOGP_KERNEL_GENEXP: BOGP_LAUNCH_CORR(BOGP_KERNEL_GENEXP); break;
    case BOGP_KERNEL_MATERN_NU: BOGP_LAUNCH_CORR(BOGP_KERNEL_MATERN_NU); break;
    default: BOGP_LAUNCH_CORR(BOGP_KERNEL_MATERN52); break;
  }
#undef BOGP_LAUNCH_CORR_PV
#undef BOGP_LAUNCH_CORR
  return hipGetLastError();
}

// (wider bases stay on the tile products: with 16 column tiles a wave -- PV = 256, quadratic trend at d = 20 -- the producer went from
// 6.8 to 88 ms per 1e6 candidates: 128 accumulator registers beside the distance loop and 16 un-staged B loads a k-step;
// profiles/r04_trend_timing.txt)
int corr_trend_columns(int p) { return p <= 1 ? 0 : (p <= 16 ? 16 : (p <= 32 ? 32 : 0)); }

#ifdef CONTRACT_D_TRACE
static unsigned long long* g_trace = nullptr;
static size_t g_trace_words = 0, g_trace_used = 0;
static int g_trace_dims[4] = {0, 0, 0, 0};
// the stamps of the largest launch so far: dims = {nMt, nJ, NJ16, words per wave}; out may be NULL (size query)
hipError_t debug_contract_trace(unsigned long long* out, size_t cap_words, size_t* used_words, int* dims) {
  if (used_words) *used_words = g_trace_used;
  if (dims) for (int i = 0; i < 4; ++i) dims[i] = g_trace_dims[i];
  if (!out) return hipSuccess;
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return e;
  return hipMemcpy(out, g_trace, std::min(cap_words, g_trace_used) * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}
#else
// BOGP_CONTRACT_DIRECT=0: the LDS-staged kernel (k_contract16<4>); the A/B switch of profiles/r06_contract_direct_ab.txt
static bool contract_direct() {
  static const bool on = [] {
    const char* e = getenv("BOGP_CONTRACT_DIRECT");
    return !(e && atoi(e) == 0);
  }();
  return on;
}
#endif

// k-pairs in flight and waves a SIMD of the narrow forms (profiles/contract_rows.txt, section C)
constexpr int CONTRACT_DD32 = 4, CONTRACT_WPE32 = 2;
constexpr int CONTRACT_DD16 = 4, CONTRACT_WPE16 = 3;

// ct.forced = 0: the candidate tile by contract_tile_rows (bogp_internal.h); ct.last = the rows a tile of this launch had
hipError_t launch_contract(const ContractArgs& a, hipStream_t st, ContractTile& ct) {
  const dim3 grid((unsigned)(a.nMt * a.nJ));
  ct.last = 64;
#ifdef CONTRACT_D_TRACE  // always k_contract16d, with the stamp buffer as its second argument
  const size_t need = (size_t)a.nMt * a.nJ * NWJ * DT_NST;
  if (need > g_trace_words) {
    if (g_trace) (void)hipFree(g_trace);
    hipError_t e = hipMalloc((void**)&g_trace, need * sizeof(unsigned long long));
    if (e != hipSuccess) return e;
    g_trace_words = need;
  }
  // the stamps of the LARGEST launch seen are kept (a sweep's last chunk is a short one); smaller launches run the same code without the dump
  const bool keep = need >= g_trace_used;
  if (keep) {
    g_trace_used = need;
    g_trace_dims[0] = a.nMt; g_trace_dims[1] = a.nJ; g_trace_dims[2] = a.NJ16; g_trace_dims[3] = DT_NST;
  }
  hipLaunchKernelGGL(k_contract16d, grid, 256, 0, st, a, keep ? g_trace : (unsigned long long*)nullptr);
#else
  if (!contract_direct()) {
    hipLaunchKernelGGL(k_contract16<4>, grid, 256, 0, st, a);
    return hipGetLastError();
  }
  // the gated launches of the per-chunk pruned path (a.live) keep 64 rows whatever is forced: most of their workgroups return at once
  const int rows = a.live ? 64 : ct.forced ? ct.forced : contract_tile_rows(a.nMt, a.nJ, ct.n_cu, false);
  const dim3 gridn((unsigned)(a.nMt * (64 / rows) * a.nJ));  // a.nMt counts 64-row tiles: the narrow tiles stay inside the same rows
  if (rows == 16) hipLaunchKernelGGL((k_contract16n<1, CONTRACT_DD16, CONTRACT_WPE16>), gridn, 256, 0, st, a);
  else if (rows == 32) hipLaunchKernelGGL((k_contract16n<2, CONTRACT_DD32, CONTRACT_WPE32>), gridn, 256, 0, st, a);
  else hipLaunchKernelGGL(k_contract16d, grid, 256, 0, st, a);
  ct.last = rows;
#endif
  return hipGetLastError();
}

// four 16-column fragments per wave (both kernels) = 256-column groups
int contract_cols_per_group() { return NWJ * 4 * 16; }

// the cross-product flavour for the batched one-point path: ncp = 16 / 32 / 64 right-hand-side columns per point; always the
// 256-column workgroups (a.nJ must be ceil(Np / 256)); a.ss_part = the points' record array, a.cross_B = points
hipError_t launch_contract_cross(const ContractArgs& a, int ncp, hipStream_t st) {
  const dim3 grid((unsigned)(a.nMt * a.nJ));
  if (ncp == 16) hipLaunchKernelGGL((k_contract16<4, 16>), grid, 256, 0, st, a);
  else if (ncp == 32) hipLaunchKernelGGL((k_contract16<4, 32>), grid, 256, 0, st, a);
  else if (ncp == 64) hipLaunchKernelGGL((k_contract16<4, 64>), grid, 256, 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace bogp
