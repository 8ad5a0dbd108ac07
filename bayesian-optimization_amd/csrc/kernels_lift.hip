// kernels_lift.hip -- the box penalty of a lifted sweep (PCA-BO, extension.py:56-86) and the order-preserving compaction
// of its feasible rows (gfx950).
//
// PCA-BO maximises its criterion over a box of the REDUCED space (r dimensions, extension.py:113-119) and maps every
// candidate z back, x_ = (z A + mean) + center (:56-59); a row whose x_ leaves the original box [lo, hi] gets
// -sum(violations) INSTEAD of the criterion (:62-86).  Of a uniform design of the reduced box 95 .. 100 % of the rows are
// such rows, so feasibility is decided for all M rows first -- M r D multiply-adds, bound by reading the
// M r doubles of z -- and the posterior sweep runs on the survivors only:
//   k_lift_penalty   per row: x_, the penalty (-0.0 <=> feasible); per workgroup: the number of feasible rows
//   k_lift_scan      exclusive scan of the workgroup counts (one workgroup)
//   k_lift_compact   feasible rows, in their original order, -> compact candidates (M_f x r) + index map (M_f)
//   k_lift_fill / k_lift_merge   value[c][m] = penalty[m], then the survivors' criterion values through the index map
// No atomic append anywhere: two runs give the same buffers, and the tie rule of the argmax (lower index) carries over to
// the original numbering.  Every store is a plain vector store.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

// A (r x D, row-major), mean, center, lo, hi (D each) are staged in LDS and read lane-uniformly (broadcast); z lives in
// registers (RB = r rounded up to the instantiation).  The sum over j runs in index order with contraction off, so that the
// NumPy restatement of the tests (bogp.Lift.to_original) follows it operation by operation.
template <int RB>
__global__ __launch_bounds__(256) void k_lift_penalty(LiftArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double s_lift[];
  __shared__ int s_cnt[4];
  const int r = a.r, D = a.D;
  const int nl = r * D + 4 * D;
  for (int t = threadIdx.x; t < nl; t += 256) s_lift[t] = a.lift[t];
  __syncthreads();
  const double* sA = s_lift;
  const double* sMean = sA + r * D;
  const double* sCenter = sMean + D;
  const double* sLo = sCenter + D;
  const double* sHi = sLo + D;
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = m < a.M;
  double z[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) z[j] = (valid && j < r) ? a.Z[(size_t)m * r + j] : 0.0;
  double s_lo = 0.0, s_hi = 0.0;
  for (int i = 0; i < D; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < RB; ++j)
      if (j < r) {
        const double t = z[j] * sA[j * D + i];
        acc = acc + t;
      }
    const double x = (acc + sMean[i]) + sCenter[i];
    if (x < sLo[i]) s_lo = s_lo + (sLo[i] - x);
    if (x > sHi[i]) s_hi = s_hi + (x - sHi[i]);
  }
  const double pen = -1.0 * (s_lo + s_hi);  // -0.0 for a feasible row, like the reference's -1 * (0.0 + 0.0)
  const bool feas = valid && pen == 0.0;    // (:73 `penalty == 0`; a NaN x_ violates nothing there either)
  if (valid) a.penalty[m] = pen;
  const unsigned long long bal = __ballot(feas);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) a.blk_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// offsets[b] = feasible rows in workgroups 0 .. b - 1, offsets[nblk] = M_f.  One workgroup of 1024 threads, each owning a
// contiguous run of counts.
__global__ __launch_bounds__(1024) void k_lift_scan(const int* __restrict__ blk_count, int64_t nblk, int64_t* __restrict__ offsets) {
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
  if (t == 1023) offsets[nblk] = s[1023];
}

// same 256-row workgroups as k_lift_penalty: row m of workgroup b lands at offsets[b] + (feasible rows before it in b)
__global__ __launch_bounds__(256) void k_lift_compact(const double* __restrict__ Z, int64_t M, int r, const double* __restrict__ penalty,
                                                      const int64_t* __restrict__ offsets, double* __restrict__ Zc,
                                                      int64_t* __restrict__ map) {
  __shared__ int s_cnt[4];
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool feas = m < M && penalty[m] == 0.0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(feas);
  if (lane == 0) s_cnt[w] = __popcll(bal);
  __syncthreads();
  if (!feas) return;
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  for (int k = 0; k < w; ++k) before += s_cnt[k];
  const int64_t dst = offsets[blockIdx.x] + before;
  for (int j = 0; j < r; ++j) Zc[(size_t)dst * r + j] = Z[(size_t)m * r + j];
  map[dst] = m;
}

__global__ __launch_bounds__(256) void k_lift_fill(const double* __restrict__ penalty, int64_t M, int q, double* __restrict__ val) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const double p = penalty[m];
  for (int c = 0; c < q; ++c) val[(size_t)c * M + m] = p;
}

__global__ __launch_bounds__(256) void k_lift_merge(const double* __restrict__ acq, const int64_t* __restrict__ map, int64_t Mf,
                                                      int q, int64_t M, double* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Mf) return;
  const int64_t m = map[i];
  for (int c = 0; c < q; ++c) val[(size_t)c * M + m] = acq[(size_t)c * Mf + i];
}

size_t lift_lds_bytes(int r, int D) { return ((size_t)r * D + 4 * (size_t)D) * sizeof(double); }

hipError_t launch_lift_penalty(const LiftArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.M + 255) / 256);
  const size_t lds = lift_lds_bytes(a.r, a.D);
  if (a.r <= 8)
    hipLaunchKernelGGL(k_lift_penalty<8>, dim3(nblk), 256, lds, st, a);
  else if (a.r <= 16)
    hipLaunchKernelGGL(k_lift_penalty<16>, dim3(nblk), 256, lds, st, a);
  else if (a.r <= 32)
    hipLaunchKernelGGL(k_lift_penalty<32>, dim3(nblk), 256, lds, st, a);
  else if (a.r <= 64)
    hipLaunchKernelGGL(k_lift_penalty<64>, dim3(nblk), 256, lds, st, a);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_lift_scan(const int* blk_count, int64_t nblk, int64_t* offsets, hipStream_t st) {
  hipLaunchKernelGGL(k_lift_scan, dim3(1), 1024, 0, st, blk_count, nblk, offsets);
  return hipGetLastError();
}

hipError_t launch_lift_compact(const double* Z, int64_t M, int r, const double* penalty, const int64_t* offsets, double* Zc,
                               int64_t* map, hipStream_t st) {
  hipLaunchKernelGGL(k_lift_compact, dim3((unsigned)((M + 255) / 256)), 256, 0, st, Z, M, r, penalty, offsets, Zc, map);
  return hipGetLastError();
}

hipError_t launch_lift_merge(const double* penalty, int64_t M, const double* acq, const int64_t* map, int64_t Mf, int q,
                             double* val, hipStream_t st) {
  hipLaunchKernelGGL(k_lift_fill, dim3((unsigned)((M + 255) / 256)), 256, 0, st, penalty, M, q, val);
  if (Mf > 0) hipLaunchKernelGGL(k_lift_merge, dim3((unsigned)((Mf + 255) / 256)), 256, 0, st, acq, map, Mf, q, M, val);
  return hipGetLastError();
}

}  // namespace bogp
