// kernels_thompson.hip -- q sample paths of the fitted surrogate over a chunk of candidates (gfx950, FP64 MFMA): Thompson sampling.
//
// The reference declares GaussianProcess.sampling_prior / sampling_posterior and leaves both as `pass` (gpr.py:312-316).  By pathwise
// conditioning (Matheron's rule on a random-Fourier-feature prior draw; Wilson et al. 2020) a path at a candidate x is
//   path_j(x) = mu(x) + z_j(x) - r(x) . g_j - b_j,     z_j(x) = sum_l W[l][j] cos(omega_l . x + phase_l)
// with W pre-scaled by sqrt(2 sigma2 / L) and (g_j, b_j) the kriging of the draw's own "data" (bogp_api_thompson.hip).  It needs the
// correlation column r(x) once -- the producer's n-major chunk -- and never the N^2 variance contraction.
//
// The feature term and the conditioning term below live in bogp_thompson_phases.h, which k_thompson_constrained shares.
// k_thompson: one workgroup of 256 serves 64 candidates, one wave 16 candidates x 16 paths (q padded by zero columns of W and g) in
// ONE v_mfma_f64_16x16x4_f64 accumulator acc[cand][path]: D row = candidate = (lane >> 4) + 4 reg, D column = path = lane & 15.
//   feature term, per tile of 16 features f0 ..: the phase tile TRANSPOSED, P[feature][cand] = Omega_tile X^T, ceil(d / 4) k-steps with
//     A = Omega[f0 + (l & 15)][4 s + (l >> 4)], B = X[c0 + (l & 15)][4 s + (l >> 4)] (zero past d).  Register reg of lane l then holds
//     feature f0 + 4 reg + (l >> 4) of candidate l & 15: after + phase and cos it IS the A operand A[cand = l & 15][k = l >> 4] of the
//     k-step over the features f0 + 4 reg .. + 3, whose B is W[f0 + 4 reg + (l >> 4)][path l & 15] -- four steps into acc, no lane
//     movement, no LDS;
//   conditioning term: acc -= rT_tile g, A = rT[(n0 + (l >> 4)) ld + c0 + (l & 15)], B = -g[n0 + (l >> 4)][l & 15], n ascending in steps
//     of 4 (the four waves read one 512-byte run per n row); rows n >= N are masked to zero, -g arrives zero padded to a multiple of 4;
//   epilogue: (mu + acc) - b_path with mu = beta + the producer's slice sums (as k_acquisition forms it), negated when minimising, the
//     optional store of the q x M values and one np.argmax record (first maximum, NaN maximal) per path and 64 candidates.
// The order of every sum depends on N, d and L alone: the outputs are bit-identical for any chunking of the candidates.
// mode 0 writes z alone (the draw at the training rows), mode 1 beta + z (prior paths); neither reads the chunk.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_mfma.h"
#include "bogp_thompson_phases.h"

namespace bogp {

__global__ __launch_bounds__(256) void k_thompson(ThompsonArgs a) {
  __shared__ double sv[4][16];
  __shared__ int64_t si[4][16];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + 16 * w;  // first row of this wave inside the launch
  const int d = a.d;

  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  // ---- feature term
  const bool xrow = c0 + li < a.mcount;
  const double* xp = a.X + (size_t)(a.row0 + c0 + li) * d;  // dereferenced under xrow only
  thompson_feature_term(a.omega, a.phase, a.W, a.L, d, xp, xrow, li, lk, acc);
  // ---- conditioning term: acc -= r . g (the host uploads -g)
  if (a.mode == 2) thompson_conditioning_term(a.rT + c0 + li, a.ld, a.ngt, a.N, li, lk, acc);
  mfma16_drain(acc);

  // ---- epilogue: lane l holds path li of the candidates c0 + 4 reg + lk
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  const double bt = a.mode == 2 ? a.bt[li] : 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = c0 + 4 * r + lk;
    if (i >= a.mcount || li >= a.q) continue;
    double val = acc[r];
    if (a.mode == 2) {
      double mu = 0.0;
      for (int s = 0; s < a.S; ++s) mu += a.mu_part[(size_t)s * a.ld + i];
      mu = a.beta + mu;
      val = (mu + val) - bt;
    } else if (a.mode == 1) {
      val = a.beta + val;
    }
    if (a.minimize) val = -1 * val;
    const int64_t row = a.row0 + i;
    if (a.vals) a.vals[(size_t)li * a.M + row] = val;
    if (better(val, row, v, idx)) {
      v = val;
      idx = row;
    }
  }
  if (!a.blk_val) return;
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const double ov = shfl_xor_f64(v, off);
    const int64_t oi = shfl_xor_i64(idx, off);
    if (better(ov, oi, v, idx)) {
      v = ov;
      idx = oi;
    }
  }
  if (lk == 0) {
    sv[w][li] = v;
    si[w][li] = idx;
  }
  __syncthreads();
  if (threadIdx.x < a.q) {
    const int p = threadIdx.x;
    v = sv[0][p];
    idx = si[0][p];
    for (int k = 1; k < 4; ++k)
      if (better(sv[k][p], si[k][p], v, idx)) {
        v = sv[k][p];
        idx = si[k][p];
      }
    a.blk_val[(size_t)p * a.nblk_total + a.blk_offset + blockIdx.x] = v;
    a.blk_idx[(size_t)p * a.nblk_total + a.blk_offset + blockIdx.x] = idx;
  }
}

hipError_t launch_thompson(const ThompsonArgs& a, hipStream_t st) {
  if (a.mcount <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_thompson, dim3((unsigned)((a.mcount + 63) / 64)), 256, 0, st, a);
  return hipGetLastError();
}

}  // namespace bogp
