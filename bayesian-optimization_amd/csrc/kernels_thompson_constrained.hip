// kernels_thompson_constrained.hip -- joint sample paths of the objective and the modelled constraints of a multi-target surrogate
// over a chunk of candidates (gfx950, FP64 MFMA): Thompson batches under modelled constraints (Eriksson & Poloczek 2021).
//
// The targets of a multi-target model share R, theta and so the correlation column r(x); sigma2_t and gamma_t differ, and the
// trend is a fixed constant (no b to subtract).  A call carries q batch members; column (j, t) is member j's path of target t:
//   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x),     z_{j,t}(x) = sum_l W[l][(j,t)] cos(omega_l . x + phase_l)
// with W pre-scaled by sqrt(2 sigma2_t / L) and the mean r . gamma_t folded into the coefficient column (bogp_api_thompson.hip), so
// the producer's slice sums are not read.
//
// k_thompson_constrained keeps k_thompson's geometry and its two matrix phases (bogp_thompson_phases.h): a workgroup of 256 serves 64
// candidates, one wave 16 candidates x 16 columns in ONE accumulator, lane l holding column l & 15 of the candidates 4 reg + (l >> 4).
// The columns are laid out t q + j: the m values of member j at a candidate sit in the lanes j, q + j, 2 q + j, ... of the SAME
// 16-lane group, and lane j gathers them with m - 1 lane reads (ds_bpermute; no LDS).  Epilogue, per candidate and member, with
// c_t = path_{j,t}(x):
//   e_t  = max(lo_t - c_t, c_t - hi_t, 0)           viol = max_{t >= 1} (e_t inv_sd_t)        feas = every lo_t <= c_t <= hi_t
//   A    = feas ? (minimize ? -c_0 : c_0) : -inf    B = 0.0 - viol                            a NaN among the m values: A = B = -inf
// Maxima of single products and comparisons only: no sum that a fused multiply-add could contract, so NumPy reproduces A and B from
// the stored path values bit for bit.  Stored on request: the [2 q][M] scores (row 2 j is A_j, 2 j + 1 is B_j) and the [q m][M] path
// values (row j m + t, the ABI's order); always one np.argmax record (first maximum) per score and 64 candidates.
// The order of every sum depends on N, d and L alone: the outputs are bit-identical for any chunking of the candidates, and a
// member's values do not depend on the members beside it.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_mfma.h"
#include "bogp_thompson_phases.h"

namespace bogp {

namespace {
__device__ __forceinline__ double shfl_f64(double v, int src) {
  int lo = __shfl(__double2loint(v), src, 64);
  int hi = __shfl(__double2hiint(v), src, 64);
  return __hiloint2double(hi, lo);
}
}  // namespace

__global__ __launch_bounds__(256) void k_thompson_constrained(ThompsonConstrainedArgs a) {
  __shared__ double sv[4][16];
  __shared__ int64_t si[4][16];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + 16 * w;  // first row of this wave inside the launch
  const int d = a.d, q = a.q, m = a.m;

  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  const bool xrow = c0 + li < a.mcount;
  const double* xp = a.X + (size_t)(a.row0 + c0 + li) * d;  // dereferenced under xrow only
  thompson_feature_term(a.omega, a.phase, a.W, a.L, d, xp, xrow, li, lk, acc);
  thompson_conditioning_term(a.rT + c0 + li, a.ld, a.coef, a.N, li, lk, acc);
  mfma16_drain(acc);

  // ---- epilogue: lane l holds column li = t q + j of the candidates c0 + 4 reg + lk; the lanes li < q form member li's scores
  const int pt = li / q, pj = li - pt * q;
  const bool column = li < q * m;
  double va = -INFINITY, vb = -INFINITY;
  int64_t ia = INT64_MAX, ib = INT64_MAX;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = c0 + 4 * r + lk;
    const bool live = i < a.mcount;
    const int64_t row = a.row0 + i;
    const double val = a.beta + acc[r];
    if (a.paths && live && column) a.paths[(size_t)(pj * m + pt) * a.M + row] = val;
    bool feas = true, bad = isnan(val);
    double viol = 0.0;
    for (int t = 1; t < m; ++t) {  // (every lane takes part in the lane reads; those of the lanes li >= q are not used)
      const double c = shfl_f64(val, 16 * lk + ((t * q + li) & 15));
      const double lo = a.lo[t], hi = a.hi[t];
      const double d1 = lo - c, d2 = c - hi;
      double e = 0.0;
      if (d1 > e) e = d1;
      if (d2 > e) e = d2;
      const double p = e * a.inv_sd[t];
      if (p > viol) viol = p;
      feas = feas && (lo <= c) && (c <= hi);
      bad = bad || isnan(c);
    }
    double A = feas ? (a.minimize ? -1 * val : val) : -INFINITY;
    double B = 0.0 - viol;
    if (bad) A = B = -INFINITY;
    if (!live || li >= q) continue;
    if (a.scores) {
      a.scores[(size_t)(2 * li) * a.M + row] = A;
      a.scores[(size_t)(2 * li + 1) * a.M + row] = B;
    }
    if (better(A, row, va, ia)) {
      va = A;
      ia = row;
    }
    if (better(B, row, vb, ib)) {
      vb = B;
      ib = row;
    }
  }
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const double oa = shfl_xor_f64(va, off), ob = shfl_xor_f64(vb, off);
    const int64_t ja = shfl_xor_i64(ia, off), jb = shfl_xor_i64(ib, off);
    if (better(oa, ja, va, ia)) {
      va = oa;
      ia = ja;
    }
    if (better(ob, jb, vb, ib)) {
      vb = ob;
      ib = jb;
    }
  }
  if (lk == 0 && li < q) {  // 2 q <= 16 slots
    sv[w][2 * li] = va;
    si[w][2 * li] = ia;
    sv[w][2 * li + 1] = vb;
    si[w][2 * li + 1] = ib;
  }
  __syncthreads();
  if (threadIdx.x < 2 * q) {
    const int p = threadIdx.x;
    double v = sv[0][p];
    int64_t idx = si[0][p];
    for (int k = 1; k < 4; ++k)
      if (better(sv[k][p], si[k][p], v, idx)) {
        v = sv[k][p];
        idx = si[k][p];
      }
    a.blk_val[(size_t)p * a.nblk_total + a.blk_offset + blockIdx.x] = v;
    a.blk_idx[(size_t)p * a.nblk_total + a.blk_offset + blockIdx.x] = idx;
  }
}

hipError_t launch_thompson_constrained(const ThompsonConstrainedArgs& a, hipStream_t st) {
  if (a.mcount <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_thompson_constrained, dim3((unsigned)((a.mcount + 63) / 64)), 256, 0, st, a);
  return hipGetLastError();
}

}  // namespace bogp
