// kernels_thompson_ehvi_constrained.hip -- joint sample paths of the m_obj objectives and the n_con modelled constraints of a
// multi-target surrogate over a chunk of candidates, selected by the hypervolume improvement of the drawn vector where the drawn
// constraints hold (gfx950, FP64 MFMA): Thompson batches for constrained multi-objective runs.
//
// A call carries q batch members; column j m + t (m = m_obj + n_con; the ABI's own order) is member j's path of target t,
//   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x),     z_{j,t}(x) = sum_l W[l][j m + t] cos(omega_l . x + phase_l)
// exactly as k_thompson_constrained and k_thompson_ehvi form it: the same geometry and the same two matrix phases
// (bogp_thompson_phases.h), a workgroup of 256 for 64 candidates, one wave 16 candidates x 16 columns in ONE accumulator, lane l holding
// column l & 15 of the candidates 4 reg + (l >> 4).  A column's bits do not depend on where it stands among the 16.  beta is added and
// the wave's tile goes to LDS (2 KB a wave), as in k_thompson_ehvi.
//
// Epilogue.  Under constraints most (candidate, member) pairs are infeasible by the draw: their A and B are -inf whatever the cells say,
// so running k_thompson_ehvi's loop over the C cells for them is work thrown away.  Here the loop runs over the feasible pairs only:
//   1  feasibility: the 16 q pairs of a wave are dealt over its 64 lanes (pair = candidate * q + member, NR = 1 or 2 rounds); a lane reads
//      its pair's m values from the tile and forms, with c_i = path_{j, m_obj + i}(x),
//        e_i = max(lo_i - c_i, c_i - hi_i, 0)    viol = max_i (e_i inv_sd_{m_obj + i})    feas = every lo_i <= c_i <= hi_i
//        V = 0.0 - viol                          a NaN among the m values: bad, V = -inf
//      in k_thompson_constrained's arithmetic (comparisons and single products).
//   2  compaction: the feasible, non-NaN pairs of live rows of all four waves go, order preserved (wave, round, lane), into ONE list in
//      LDS -- a ballot and a popcount prefix inside the wave, the waves' offsets through four words of LDS.  F <= 64 q <= 320 entries.
//   3  the cell loop on the list: thread t takes entry t (and entry t + 256 where NR = 2: only q = 5 can fill more than 256), so
//      ceil(F / 64) waves run the loop and the others skip it; F = 0 skips it for the whole workgroup.  A lane's entries go through
//      ONE pass over the cells, the bounds read at wave-uniform addresses as in k_thompson_ehvi, and per pair the operations and their order are
//      k_thompson_ehvi's:
//        per cell c, k = 0 .. m_obj - 1:   t_k = max(min(y_k, u_ck) - l_ck, 0)       p = t_0; p = p t_1; ...;  acc = acc + p   (acc from 0.0)
//                                          e_k = max(l_ck - y_k, y_k - u_ck, 0) inv_sd_k;  cm = max_k e_k (from 0.0);  dist = min(dist, cm)
//        A = acc > 0 ? acc : -inf          B = 0.0 - dist
//      Contraction is off; a pair's cells are never split over lanes.  What a pair's lane computes depends on the pair's own values
//      and the cells alone, so where the pair stands in the list changes no bit.
//   4  scores and records: the scores go back to the OWNING wave's tile as [3 q][16] (row 3 j is A_j, 3 j + 1 is B_j, 3 j + 2 is V_j;
//      3 q <= 15): a listed pair's A and B by the lane that ran its cells, every pair's V -- and A = B = -inf of an unlisted pair -- by
//      the lane of step 1.  Lane s < 3 q scans its 16 candidates in order with `better`, and the four waves are combined as in the
//      sibling kernels: one record per score and 64 candidates.
// Every sum's order depends on N, d, L, C and m_obj alone: the outputs are bit-identical for any chunking, with and without the stored
// paths, and for a member alone or beside others.
#include "bogp_device.h"
#include "bogp_internal.h"
#include "bogp_mfma.h"
#include "bogp_thompson_phases.h"

namespace bogp {

template <int MO, int NR>
__global__ __launch_bounds__(256) void k_thompson_ehvi_constrained(ThompsonEhviConstrainedArgs a) {
#pragma clang fp contract(off)
  __shared__ double tile[4][256];
  __shared__ double sv[4][16];
  __shared__ int64_t si[4][16];
  __shared__ unsigned short list[64 * 5];  // (wave << 7) | pair, pair < 80
  __shared__ int wcount[4];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * 64 + 16 * w;  // first row of this wave inside the launch
  const int d = a.d, q = a.q, nc = a.n_con, m = MO + nc;

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
    if (a.paths && i < a.mcount && li < q * m) a.paths[(size_t)li * a.M + a.row0 + i] = val;
    tw[(4 * r + lk) * 16 + li] = val;
  }
  __syncthreads();

  // ---- 1: feasibility of this lane's pairs, pair p = candidate * q + member
  const int npair = 16 * q;
  int pr[NR], pj[NR];
  bool on[NR], ok[NR];
  double V[NR];
  unsigned long long mask[NR];
  int mine = 0;
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int p = lane + 64 * u;
    on[u] = p < npair;
    pr[u] = on[u] ? p / q : 0;
    pj[u] = on[u] ? p - pr[u] * q : 0;
    const double* yp = tw + pr[u] * 16 + pj[u] * m;
    bool bad = false, feas = true;
#pragma unroll
    for (int k = 0; k < MO; ++k) bad = bad || isnan(yp[k]);
    double viol = 0.0;
    for (int t = 0; t < nc; ++t) {
      const double c = yp[MO + t];
      const double lo = a.lo[t], hi = a.hi[t];
      const double d1 = lo - c, d2 = c - hi;
      double e = 0.0;
      if (d1 > e) e = d1;
      if (d2 > e) e = d2;
      const double p2 = e * a.inv_sd[MO + t];
      if (p2 > viol) viol = p2;
      feas = feas && (lo <= c) && (c <= hi);
      bad = bad || isnan(c);
    }
    V[u] = bad ? -INFINITY : 0.0 - viol;
    ok[u] = on[u] && feas && !bad && c0 + pr[u] < a.mcount;
    mask[u] = __ballot(ok[u]);
    mine += __popcll(mask[u]);
  }
  // ---- 2: the list of the workgroup's feasible pairs, in the order (wave, round, lane)
  if (lane == 0) wcount[w] = mine;
  __syncthreads();
  int base = 0, F = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ck = wcount[k];
    if (k < w) base += ck;
    F += ck;
  }
  F = __builtin_amdgcn_readfirstlane(F);
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    if (ok[u]) list[base + __popcll(mask[u] & ((1ull << lane) - 1ull))] = (unsigned short)((w << 7) | (lane + 64 * u));
    base += __popcll(mask[u]);
  }
  __syncthreads();

  // ---- 3: ONE pass over the cells for the entries threadIdx.x (+ 256) of the list; the waves past the list's end skip it
  double y[NR][MO], hv[NR], dist[NR];
  int ew[NR], er[NR], ej[NR];
  bool have[NR];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int e = (int)threadIdx.x + 256 * u;
    have[u] = e < F;
    const int code = have[u] ? (int)list[e] : 0;
    const int p = code & 127;
    ew[u] = code >> 7;
    er[u] = p / q;
    ej[u] = p - er[u] * q;
#pragma unroll
    for (int k = 0; k < MO; ++k) y[u][k] = have[u] ? tile[ew[u]][er[u] * 16 + ej[u] * m + k] : 0.0;
    hv[u] = 0.0;
    dist[u] = INFINITY;
  }
  if (64 * w < F) {
    for (int c = 0; c < a.C; ++c) {
      double lb[MO], ub[MO];
#pragma unroll
      for (int k = 0; k < MO; ++k) {
        lb[k] = a.lower[(size_t)c * MO + k];
        ub[k] = a.upper[(size_t)c * MO + k];
      }
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        double p = 0.0, cm = 0.0;
#pragma unroll
        for (int k = 0; k < MO; ++k) {
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
  }
  __syncthreads();  // every entry's values are in registers: the tiles now take the scores, [3 q][16]

  // ---- 4: the scores.  A listed pair's A and B come from the lane that ran its cells, the rest from the lane of step 1
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    if (!have[u]) continue;
    const double A = hv[u] > 0.0 ? hv[u] : -INFINITY;
    const double B = 0.0 - dist[u];
    tile[ew[u]][(3 * ej[u]) * 16 + er[u]] = A;
    tile[ew[u]][(3 * ej[u] + 1) * 16 + er[u]] = B;
    if (a.scores) {  // (a listed pair's row is below mcount)
      const int64_t row = a.row0 + (int64_t)blockIdx.x * 64 + 16 * ew[u] + er[u];
      a.scores[(size_t)(3 * ej[u]) * a.M + row] = A;
      a.scores[(size_t)(3 * ej[u] + 1) * a.M + row] = B;
    }
  }
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    if (!on[u]) continue;
    const int64_t i = c0 + pr[u];
    const bool store = a.scores && i < a.mcount;
    tw[(3 * pj[u] + 2) * 16 + pr[u]] = V[u];
    if (store) a.scores[(size_t)(3 * pj[u] + 2) * a.M + a.row0 + i] = V[u];
    if (ok[u]) continue;
    tw[(3 * pj[u]) * 16 + pr[u]] = -INFINITY;
    tw[(3 * pj[u] + 1) * 16 + pr[u]] = -INFINITY;
    if (store) {
      a.scores[(size_t)(3 * pj[u]) * a.M + a.row0 + i] = -INFINITY;
      a.scores[(size_t)(3 * pj[u] + 1) * a.M + a.row0 + i] = -INFINITY;
    }
  }
  __syncthreads();

  // ---- records: lane s < 3 q takes the first maximum of its score over the wave's 16 candidates, thread s < 3 q that of the four waves
  if (lane < 3 * q) {
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
  if (threadIdx.x < 3 * q) {
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
template <int MO>
hipError_t launch_mo(const ThompsonEhviConstrainedArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)((a.mcount + 63) / 64));
  if (16 * a.q > 64) {  // q = 5: m = 3, two objectives and one constraint
    if constexpr (MO == 2) hipLaunchKernelGGL((k_thompson_ehvi_constrained<2, 2>), grid, 256, 0, st, a);
    else return hipErrorInvalidValue;
  } else {
    hipLaunchKernelGGL((k_thompson_ehvi_constrained<MO, 1>), grid, 256, 0, st, a);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t launch_thompson_ehvi_constrained(const ThompsonEhviConstrainedArgs& a, hipStream_t st) {
  if (a.mcount <= 0) return hipSuccess;
  const int m = a.m_obj + a.n_con;
  if (a.q < 1 || a.n_con < 1 || m > 8 || a.q * m > 16 || a.C < 1) return hipErrorInvalidValue;
  switch (a.m_obj) {
    case 2: return launch_mo<2>(a, st);
    case 3: return launch_mo<3>(a, st);
    case 4: return launch_mo<4>(a, st);
    case 5: return launch_mo<5>(a, st);
    case 6: return launch_mo<6>(a, st);
    case 7: return launch_mo<7>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bogp
