// kernels_thompson_ehvi.hip -- joint sample paths of the m objectives of a multi-target surrogate over a chunk of candidates, selected by
// the hypervolume improvement of the drawn vector (gfx950, FP64 MFMA): Thompson batches for multi-objective runs.
//
// A call carries q batch members; column j m + t (the ABI's own order) is member j's path of target t,
//   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x),     z_{j,t}(x) = sum_l W[l][j m + t] cos(omega_l . x + phase_l)
// exactly as k_thompson_constrained forms it: the same geometry and the same two matrix phases (bogp_thompson_phases.h), a workgroup of
// 256 for 64 candidates, one wave 16 candidates x 16 columns in ONE accumulator, lane l holding column l & 15 of the candidates
// 4 reg + (l >> 4).  A column's bits do not depend on where it stands among the 16.
//
// Epilogue.  The constrained kernel gathers a member's m values into one lane of each 16-lane group, which leaves 16 - q lanes of every
// group idle: harmless for its m - 1 comparisons, not for a loop over C cells.  Here the wave's 16 x 16 tile (beta added) goes to LDS,
// 2 KB, and the 16 q (candidate, member) pairs are dealt over ALL 64 lanes: lane p takes the pairs p and p + 64 (pair = candidate * q +
// member, so a lane's m values are m consecutive words and a round of lanes reads a dense run).  (m, q) = (2, 8): two pairs a lane;
// (3, 5): 80 pairs, a second round of 16 lanes; q <= 4: one round of 16 q lanes.  NR, the rounds, is a template parameter beside MT = m:
// the NR MT values stay in registers, and both pairs of a lane go through ONE pass over the cells, so every bound is fetched once -- at a
// wave-uniform address, into scalar registers, as ehvi_cells reads them -- and the two chains interleave.  With y_k the m values of a pair:
//   per cell c, k = 0 .. m - 1:   t_k = max(min(y_k, u_ck) - l_ck, 0)       p = t_0; p = p t_1; ...;  acc = acc + p       (acc from 0.0)
//                                 e_k = max(l_ck - y_k, y_k - u_ck, 0) inv_sd_k;  cm = max_k e_k (from 0.0);  dist = min(dist, cm) (from +inf)
//   A = acc > 0 ? acc : -inf      B = 0.0 - dist      a NaN among the m values: A = B = -inf
// Contraction is off: every product and every sum is rounded on its own, in this order, for every chunking and whatever members stand
// beside the pair -- NumPy reproduces A and B from the stored path values byte for byte (thompson.hvi_select_numpy).  The minima and
// maxima are v_min_f64 / v_max_f64; the sign of a zero they return cannot reach A or B (0.0 + -0.0 and 0.0 - -0.0 are +0.0).
// A pair's cells are never split over lanes: that would change the order of the sum.
//
// Records: the scores go back to the wave's tile as [2 q][16] (row 2 j is A_j, 2 j + 1 is B_j; 2 q <= 16), lane s < 2 q scans its 16
// candidates in order with `better` (np.argmax: first maximum), and the four waves are combined as in k_thompson_constrained.  Stored on
// request: the [2 q][M] scores and the [q m][M] path values; always one record per score and 64 candidates.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_mfma.h"
#include "bogp_thompson_phases.h"

namespace bogp {

template <int MT, int NR>
__global__ __launch_bounds__(256) void k_thompson_ehvi(ThompsonEhviArgs a) {
#pragma clang fp contract(off)
  __shared__ double tile[4][256];
  __shared__ double sv[4][16];
  __shared__ int64_t si[4][16];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + 16 * w;  // first row of this wave inside the launch
  const int d = a.d, q = a.q;

  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  const bool xrow = c0 + li < a.mcount;
  const double* xp = a.X + (size_t)(a.row0 + c0 + li) * d;  // dereferenced under xrow only
  thompson_feature_term(a.omega, a.phase, a.W, a.L, d, xp, xrow, li, lk, acc);
  thompson_conditioning_term(a.rT + c0 + li, a.ld, a.coef, a.N, li, lk, acc);
  mfma16_drain(acc);

  // ---- the tile: lane l holds column li of the candidates c0 + 4 reg + lk
  double* tw = tile[w];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = c0 + 4 * r + lk;
    const double val = a.beta + acc[r];
    if (a.paths && i < a.mcount && li < q * MT) a.paths[(size_t)li * a.M + a.row0 + i] = val;
    tw[(4 * r + lk) * 16 + li] = val;
  }
  __syncthreads();

  // ---- the pairs of this lane: pair p = candidate * q + member
  const int npair = 16 * q;
  double y[NR][MT], hv[NR], dist[NR];
  int pr[NR], pj[NR];
  bool on[NR], bad[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int p = lane + 64 * u;
    on[u] = p < npair;
    pr[u] = on[u] ? p / q : 0;
    pj[u] = on[u] ? p - pr[u] * q : 0;
    bad[u] = false;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      y[u][k] = tw[pr[u] * 16 + pj[u] * MT + k];
      bad[u] = bad[u] || isnan(y[u][k]);
    }
    hv[u] = 0.0;
    dist[u] = INFINITY;
  }
  // ---- ONE pass over the cells for HVI and dist; the bounds are the same for every lane
  for (int c = 0; c < a.C; ++c) {
    double lb[MT], ub[MT];
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      lb[k] = a.lower[(size_t)c * MT + k];
      ub[k] = a.upper[(size_t)c * MT + k];
    }
#pragma unroll
    for (int u = 0; u < NR; ++u) {
      double p = 0.0, cm = 0.0;
#pragma unroll
      for (int k = 0; k < MT; ++k) {
        const double yk = y[u][k];
        const double t = __builtin_fmax(__builtin_fmin(yk, ub[k]) - lb[k], 0.0);
        p = k == 0 ? t : p * t;
        const double e = __builtin_fmax(__builtin_fmax(lb[k] - yk, yk - ub[k]), 0.0);
        cm = __builtin_fmax(cm, e * a.inv_sd[k]);
      }
      hv[u] = hv[u] + p;
      dist[u] = __builtin_fmin(dist[u], cm);
    }
  }
  __syncthreads();  // every lane has its values: the tile now takes the scores, [2 q][16]

#pragma unroll
  for (int u = 0; u < NR; ++u) {
    double A = hv[u] > 0.0 ? hv[u] : -INFINITY;
    double B = 0.0 - dist[u];
    if (bad[u]) A = B = -INFINITY;
    if (!on[u]) continue;
    tw[(2 * pj[u]) * 16 + pr[u]] = A;
    tw[(2 * pj[u] + 1) * 16 + pr[u]] = B;
    const int64_t i = c0 + pr[u];
    if (a.scores && i < a.mcount) {
      a.scores[(size_t)(2 * pj[u]) * a.M + a.row0 + i] = A;
      a.scores[(size_t)(2 * pj[u] + 1) * a.M + a.row0 + i] = B;
    }
  }
  __syncthreads();

  // ---- records: lane s < 2 q takes the first maximum of its score over the wave's 16 candidates, thread s < 2 q that of the four waves
  if (lane < 2 * q) {
    double v = -INFINITY;
    int64_t idx = INT64_MAX;
    for (int r = 0; r < 16; ++r) {
      const int64_t i = c0 + r;
      const double s = tw[lane * 16 + r];
      if (i < a.mcount && better(s, a.row0 + i, v, idx)) {
        v = s;
        idx = a.row0 + i;
      }
    }
    sv[w][lane] = v;
    si[w][lane] = idx;
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

namespace {
template <int MT>
hipError_t launch_m(const ThompsonEhviArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.mcount + 63) / 64));
  if (16 * a.q > 64) {  // q >= 5: m <= 3
    if constexpr (MT <= 3) hipLaunchKernelGGL((k_thompson_ehvi<MT, 2>), grid, 256, 0, st, a);
    else return hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((k_thompson_ehvi<MT, 1>), grid, 256, 0, st, a);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_thompson_ehvi(const ThompsonEhviArgs& a, hipStream_t st) {
  if (a.mcount <= 0) return hipSuccess;
  if (a.q < 1 || a.q * a.m > 16 || a.C < 1) return hipErrorInvalidValue;
  switch (a.m) {
    case 2: return launch_m<2>(a, st);
    case 3: return launch_m<3>(a, st);
    case 4: return launch_m<4>(a, st);
    case 5: return launch_m<5>(a, st);
    case 6: return launch_m<6>(a, st);
    case 7: return launch_m<7>(a, st);
    case 8: return launch_m<8>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bogp
