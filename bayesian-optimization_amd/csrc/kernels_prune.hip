// kernels_prune.hip -- the pruned sweep: skip the N^2 variance contraction for candidates that cannot win (gfx950).
//
// A sweep that returns only its q winners does not need the variance of a row whose criteria cannot reach the best values found
// so far even with the most optimistic variance: |L^-1 r|^2 >= 0, so MSE <= (1 + u^2) sigma2 =: sd_ub^2, and the producer has
// already delivered mu and w . r (hence u).  Per chunk region, behind the producer:
//   k_prune_bound    per row: mu, u and sd_ub exactly as k_acquisition forms them with ss = 0, acq_upper_bound of every criterion
//                    against the running best (device resident); a row survives unless EVERY criterion is out of reach
//                    (prune_below); per workgroup: the number of survivors
//   k_prune_scan     exclusive scan of the workgroup counts (one workgroup, kernels_lift.hip's pattern) and the region's decision:
//                    more than a quarter survives -> the region is contracted in place as ever; else its survivors are appended
//                    to the survivor buffer
//   k_prune_compact  survivors, in their original order -> their region rows, their global indices and their mu / w partials
//   k_prune_gather   the survivors' columns of rT -> the survivor buffer (a bit copy)
//   k_prune_update   the block records of an acquisition launch (in place, or of the flushed buffer) merged into the running best
// The host never learns a count: every count lives in the control words below, k_contract16d / k_acquisition / the kernels here
// read the one they need and workgroups beyond it return at once.  (The one-pass flow below is the exception: it reads two counts.)
// No atomic append: two runs give the same buffers.  A pruned
// row is strictly worse than a value an evaluated row attained, so the winners (lowest index on ties, a NaN first) are those of
// the full sweep, and their values are the full sweep's bits: rows of the contraction are independent of each other.
//
// One pass (run_sweep): where every candidate is resident and the producer exists without its store, the rows behind
// the pilot are bounded in ONE launch per segment -- the producer leaves only its partial sums -- and only the survivors' correlation
// columns are ever produced:
//   k_prune_scan     with cap < 0: the exclusive scan and the survivor count (PC_TOTAL), which the host reads
//   k_prune_index    survivors, in their original order -> their global indices
//   k_prune_rows     a round of at most one survivor buffer: the survivors' candidate rows -> a compact candidate array, which the
//                    storing producer, k_contract16d, k_acquisition (through the index map) and k_prune_update then take with exact grids
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

// control words (long long): [0] survivors in the buffer, [1] rows of the current region to contract in place (0: gathered),
// [2] survivors of the current region to gather (0: in place), [3] their first slot in the buffer, [4] rows that went through the
// contraction in this sweep
// [5] one pass: survivors of the region bounded last
enum { PC_BUF = 0, PC_INPLACE = 1, PC_GATHER = 2, PC_BASE = 3, PC_CONTRACTED = 4, PC_TOTAL = 5 };
static_assert(PC_TOTAL == PRUNE_CTL_TOTAL && PC_CONTRACTED == PRUNE_CTL_CONTRACTED && PC_TOTAL < PRUNE_CTL_WORDS, "control words");

__global__ void k_prune_init(long long* ctl, double* best_val, int64_t* best_idx, int q, long long pilot_rows) {
  const int t = threadIdx.x;
  if (t < PRUNE_CTL_WORDS) ctl[t] = t == PC_CONTRACTED ? pilot_rows : 0;
  if (t < q) {
    best_val[t] = -INFINITY;
    best_idx[t] = INT64_MAX;
  }
}

__global__ __launch_bounds__(256) void k_prune_bound(PruneBoundArgs a) {
  __shared__ int s_cnt[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < a.rcount;
  bool keep = false;
  if (valid) {
    // k_acquisition's own statements with ss = 0: ss >= 0 can only lower 1.0 - ss, and +, * sigma2 > 0 and sqrt are monotone in
    // floating point, so sd <= sd_ub holds for the row's exact sd
    double mu = 0.0, wd = 0.0, ss = 0.0;
    for (int s = 0; s < a.S; ++s) {
      mu += a.mu_part[(size_t)s * a.Mc + i];
      wd += a.w_part[(size_t)s * a.Mc + i];
    }
    mu = a.beta + mu;
    double u2 = 0.0;
    if (a.estimate_trend) {
      const double u = (wd - 1.0) / a.G;
      u2 = u * u;
    }
    double mse = (1.0 - ss + u2) * a.sigma2;
    if (mse < 0.0) mse = 0.0;
    const double y_hat = a.minimize ? mu : -1 * mu;
    const double sd_ub = sqrt(mse);
    for (int c = 0; c < a.q; ++c) {
      const double b = acq_upper_bound(a.acq_id[c], a.acq_par[c], y_hat, sd_ub, a.plugin, a.sigma2);
      keep = keep || !prune_below(b, a.best_val[c]);
    }
    a.flags[i] = keep ? 1 : 0;
  }
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) a.blk_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// offsets[b] = survivors in workgroups 0 .. b - 1; then the region's decision.  `cap` = rows of the survivor buffer (the host
// flushes it before a region whose quarter might not fit; a region that would not fit is contracted in place all the same).
// cap < 0 (one pass): no decision here -- the count goes to PC_TOTAL for the host, nothing else changes.
__global__ __launch_bounds__(1024) void k_prune_scan(const int* __restrict__ blk_count, int64_t nblk, int64_t* __restrict__ offsets,
                                                     int64_t rcount, int64_t cap, long long* __restrict__ ctl) {
  __shared__ int64_t s[1024];
  const int t = threadIdx.x;
  const int64_t per = (nblk + 1023) / 1024;
  const int64_t b0 = std::min<int64_t>(nblk, t * per), b1 = std::min<int64_t>(nblk, b0 + per);
  int64_t sum = 0;
  for (int64_t b = b0; b < b1; ++b) sum += blk_count[b];
  s[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t v = t >= off ? s[t - off] : 0;
    __syncthreads();
    s[t] += v;
    __syncthreads();
  }
  int64_t run = s[t] - sum;
  for (int64_t b = b0; b < b1; ++b) {
    offsets[b] = run;
    run += blk_count[b];
  }
  if (t == 1023) {
    const int64_t total = s[1023];
    if (cap < 0) {
      ctl[PC_TOTAL] = total;
      return;
    }
    const int64_t have = ctl[PC_BUF];
    const bool inplace = 4 * total > rcount || have + total > cap;
    ctl[PC_INPLACE] = inplace ? rcount : 0;
    ctl[PC_GATHER] = inplace ? 0 : total;
    ctl[PC_BASE] = have;
    if (inplace) ctl[PC_CONTRACTED] += rcount;
    else ctl[PC_BUF] = have + total;
  }
}

// same 256-row workgroups as k_prune_bound: survivor i of workgroup b is the (offsets[b] + survivors before it in b)-th of the region
__global__ __launch_bounds__(256) void k_prune_compact(PruneGatherArgs a) {
  __shared__ int s_cnt[4];
  if (a.ctl[PC_GATHER] == 0) return;  // contracted in place (or nothing survived)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < a.rcount && a.flags[i] != 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_cnt[w] = __popcll(bal);
  __syncthreads();
  if (!keep) return;
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) before += s_cnt[k];
  const int64_t k = a.offsets[blockIdx.x] + before;  // < ctl[PC_GATHER] <= rcount / 4
  const int64_t dst = a.ctl[PC_BASE] + k;            // < Ms (k_prune_scan)
  a.sel[k] = (int)i;
  a.map[dst] = a.m0 + i;
  for (int s = 0; s < a.S; ++s) {
    a.mu_s[(size_t)s * a.Ms + dst] = a.mu_part[(size_t)s * a.Mc + i];
    a.w_s[(size_t)s * a.Ms + dst] = a.w_part[(size_t)s * a.Mc + i];
  }
}

// (`through`, FP32 stage: the region is a list of rows -- S1 -- and a survivor's entry of that list is kept instead of m0 + i)
// one pass: k_prune_compact's enumeration, the global indices alone; `cap` entries (a region with more survivors falls back: its list is not read)
__global__ __launch_bounds__(256) void k_prune_index(const unsigned char* __restrict__ flags, const int64_t* __restrict__ offsets, int64_t rcount,
                                                     int64_t m0, int64_t cap, int64_t* __restrict__ sidx, const int64_t* __restrict__ through) {
  __shared__ int s_cnt[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool keep = i < rcount && flags[i] != 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) s_cnt[w] = __popcll(bal);
  __syncthreads();
  if (!keep) return;
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) before += s_cnt[k];
  const int64_t k = offsets[blockIdx.x] + before;
  if (k < cap) sidx[k] = through ? through[i] : m0 + i;
}

// one pass: rows sidx[0 .. count) of the candidates -> Xc (count x d, row-major)
__global__ __launch_bounds__(256) void k_prune_rows(const double* __restrict__ Xs, const int64_t* __restrict__ sidx, int64_t count, int d,
                                                    double* __restrict__ Xc) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count * d) return;
  const int64_t row = e / d;
  Xc[e] = Xs[sidx[row] * d + (e - row * d)];
}

// workgroup (x, y): survivors [64 x, 64 x + 64) of the region, rows [32 y, 32 y + 32) of rT; 64 consecutive doubles per store
__global__ __launch_bounds__(256) void k_prune_gather(PruneGatherArgs a) {
  const int64_t n_g = a.ctl[PC_GATHER];
  const int64_t k = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  if ((int64_t)blockIdx.x * 64 >= n_g) return;
  if (k >= n_g) return;
  const int64_t src = a.sel[k];
  const int64_t dst = a.ctl[PC_BASE] + k;
  const int n0 = blockIdx.y * 32 + (threadIdx.x >> 6);
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int n = n0 + 4 * r;
    if (n < a.Np) a.rTs[(size_t)n * a.Ms + dst] = a.rT[(size_t)n * a.Mc + src];
  }
}

// one workgroup per criterion: the records of the launch's live blocks and the running best -> the running best
__global__ __launch_bounds__(256) void k_prune_update(const double* blk_val, const int64_t* blk_idx, int64_t stride, const long long* live,
                                                      int64_t count, double* best_val, int64_t* best_idx) {
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  const int c = blockIdx.x;
  const int64_t rows = live ? (int64_t)*live : count;
  const int64_t nblk = (rows + 255) / 256;
  if (nblk == 0) return;
  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  for (int64_t k = threadIdx.x; k < nblk; k += 256) {
    const double ov = blk_val[(size_t)c * stride + k];
    const int64_t oi = blk_idx[(size_t)c * stride + k];
    if (better(ov, oi, v, idx)) {
      v = ov;
      idx = oi;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = shfl_xor_f64(v, off);
    const int64_t oi = shfl_xor_i64(idx, off);
    if (better(ov, oi, v, idx)) {
      v = ov;
      idx = oi;
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sv[w] = v;
    si[w] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k)
      if (better(sv[k], si[k], v, idx)) {
        v = sv[k];
        idx = si[k];
      }
    if (better(v, idx, best_val[c], best_idx[c])) {
      best_val[c] = v;
      best_idx[c] = idx;
    }
  }
}

__global__ void k_prune_flushed(long long* ctl) {
  ctl[PC_CONTRACTED] += ctl[PC_BUF];
  ctl[PC_BUF] = 0;
}

hipError_t launch_prune_init(long long* ctl, double* best_val, int64_t* best_idx, int q, int64_t pilot_rows, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_init, dim3(1), 64, 0, st, ctl, best_val, best_idx, q, (long long)pilot_rows);
  return hipGetLastError();
}

hipError_t launch_prune_bound(const PruneBoundArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_bound, dim3((unsigned)((a.rcount + 255) / 256)), 256, 0, st, a);
  return hipGetLastError();
}

hipError_t launch_prune_scan(const int* blk_count, int64_t nblk, int64_t* offsets, int64_t rcount, int64_t cap, long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_scan, dim3(1), 1024, 0, st, blk_count, nblk, offsets, rcount, cap, ctl);
  return hipGetLastError();
}

hipError_t launch_prune_gather(const PruneGatherArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_compact, dim3((unsigned)((a.rcount + 255) / 256)), 256, 0, st, a);
  const int64_t max_g = a.rcount / 4;  // a region with more survivors is contracted in place
  if (max_g > 0)
    hipLaunchKernelGGL(k_prune_gather, dim3((unsigned)((max_g + 63) / 64), (unsigned)((a.Np + 31) / 32)), 256, 0, st, a);
  return hipGetLastError();
}

hipError_t launch_prune_index(const unsigned char* flags, const int64_t* offsets, int64_t rcount, int64_t m0, int64_t cap, int64_t* sidx,
                              hipStream_t st, const int64_t* through) {
  hipLaunchKernelGGL(k_prune_index, dim3((unsigned)((rcount + 255) / 256)), 256, 0, st, flags, offsets, rcount, m0, cap, sidx, through);
  return hipGetLastError();
}

hipError_t launch_prune_rows(const double* Xs, const int64_t* sidx, int64_t count, int d, double* Xc, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_rows, dim3((unsigned)((count * d + 255) / 256)), 256, 0, st, Xs, sidx, count, d, Xc);
  return hipGetLastError();
}

hipError_t launch_prune_update(const double* blk_val, const int64_t* blk_idx, int64_t stride, const long long* live, int64_t count, int q,
                               double* best_val, int64_t* best_idx, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_update, dim3(q), 256, 0, st, blk_val, blk_idx, stride, live, count, best_val, best_idx);
  return hipGetLastError();
}

hipError_t launch_prune_flushed(long long* ctl, hipStream_t st) {
  hipLaunchKernelGGL(k_prune_flushed, dim3(1), 1, 0, st, ctl);
  return hipGetLastError();
}

}  // namespace bogp
