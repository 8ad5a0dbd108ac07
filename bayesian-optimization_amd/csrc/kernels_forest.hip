// kernels_forest.hip -- a packed regression forest over the candidates: traversal, moments over the trees, criteria, argmax (gfx950).
//
// Replaces, per candidate row, RandomForest.predict(X, eval_MSE=True) (surrogate/random_forest.py:124-155) -- scikit-learn's
// Tree.predict on the row cast to float32 (_validate_X_predict), mean over the T trees as mu, std(ddof = 1)^2 over the trees as MSE --
// and, on these moments, AcquisitionFunction.__call__ (acquisition_fun.py:52-64, 127-135, 153-176, 208-217, 265-290) through the
// shared acq_value of bogp_device.h, and np.argmax over the rows into the per-block records k_argmax_final / the top-k passes read.
//
// Layout.  One lane = one row, 256 rows a workgroup.  The row's features sit in LDS as float32, FEATURE-major (xs[k][lane]): a
// node's feature index differs from lane to lane, which as a register-array index would land in scratch; in LDS the word of lane l
// is always in bank l mod 64 whatever k is, so the gather never conflicts.  The forest is streamed ONE TREE AT A TIME through two
// LDS buffers: while the lanes walk tree t out of one buffer, the words of tree t + 1 are in flight from L2 into registers and are
// stored into the other buffer behind the walk; one barrier a tree.  A tree is [n_nodes records | n_leaves values]:
//   record (8 bytes) = {float32 thr, uint32 w},  w = eq << 31 | feature << 16 | child;  child = 0 marks a leaf, whose thr word is
//   the index of its value; the children of an inner node are adjacent (left = child, right = child + 1: breadth-first renumbering
//   on the host), so one 16-bit field serves both.
//   eq = 0: left iff x <= thr.  x is float32, so x <= t64 is x <= (t64 rounded toward -inf to float32): the host rounds, the walk
//           compares two floats.  NaN goes right (NaN <= t is false).
//   eq = 1: left iff x != thr -- a split of a one-hot column at 0.5, rewritten by the host onto the raw column holding the level index.
// The walk of a tree is bounded by the tree's depth (found by the host's validation walk): a forest cannot hang the device.
//
// Moments.  p_t in tree order through Welford's update: delta = p_t - mean, mean += delta / (t + 1) (the reciprocal comes with the
// tree's table entry), M2 += delta (p_t - mean); mu = mean, var = M2 / (T - 1), MSE = sqrt(var)^2 (the reference squares np.std).
// Nothing cancels, whatever the first tree predicts: both moments stay within a few ulp of NumPy's pairwise mean / std, and trees
// that all agree give MSE = 0 exactly.  A row's result is a function of the row and the forest alone -- same order in every lane,
// no atomics -- so rows with equal leaves get equal bits, and exact ties resolve to the lower index as np.argmax does.
// EI's guard for a model without sigma2 is sd < 1e-10 (acquisition_fun.py:166-169); acq_value's is sd / sqrt(sigma2) < 1e-6, which
// sigma2 = 1e8 turns into sd / 1e4 < 1e-6.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

constexpr int FOREST_STAGE = 4;  // words of the next tree a lane holds in registers during the walk (256 x 4 = 1024 words; larger trees copy the rest directly)

template <bool LEAVES>
__global__ __launch_bounds__(256) void k_forest(ForestArgs a) {
  extern __shared__ unsigned long long forest_smem[];
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  unsigned long long* const buf0 = forest_smem;
  unsigned long long* const buf1 = forest_smem + a.tree_words;
  float* xs = (float*)(forest_smem + 2 * (size_t)a.tree_words);  // [d][256]
  const int tid = threadIdx.x;
  const int64_t rloc = (int64_t)blockIdx.x * 256 + tid;  // row inside this launch
  const bool valid = rloc < a.nrows;
  const int64_t row = a.row0 + rloc;

  // the workgroup's 256 x d doubles are contiguous: coalesced read, rounded to float32 as _validate_X_predict does
  {
    const int64_t e0 = (a.row0 + (int64_t)blockIdx.x * 256) * a.d;
    const int64_t e1 = min((a.row0 + min((int64_t)(blockIdx.x + 1) * 256, a.nrows)) * a.d, a.M * a.d);
    for (int e = tid; e < 256 * a.d; e += 256) {
      const int r = e / a.d, k = e - r * a.d;
      xs[k * 256 + r] = e0 + e < e1 ? (float)a.Xs[e0 + e] : 0.0f;
    }
  }
  {
    const ForestTree t0 = a.tree[0];
    const int nw = t0.n_nodes + t0.n_leaves;
    for (int i = tid; i < nw; i += 256) buf0[i] = a.words[(size_t)t0.first + i];
  }
  __syncthreads();

  double mean = 0.0, M2 = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const unsigned long long* cur = (t & 1) ? buf1 : buf0;
    unsigned long long* nxt = (t & 1) ? buf0 : buf1;
    const ForestTree tc = a.tree[t];
    unsigned long long stage[FOREST_STAGE];
    int nw_next = 0;
    const unsigned long long* g = a.words;
    if (t + 1 < a.T) {
      const ForestTree tn = a.tree[t + 1];
      nw_next = tn.n_nodes + tn.n_leaves;
      g = a.words + (size_t)tn.first;
#pragma unroll
      for (int j = 0; j < FOREST_STAGE; ++j) {
        const int i = tid + 256 * j;
        stage[j] = i < nw_next ? g[i] : 0ull;
      }
    }
    // the walk
    const uint2* nodes = (const uint2*)cur;
    uint2 nd = nodes[0];
    for (int s = 0; s < tc.depth && (nd.y & 0xffffu) != 0u; ++s) {
      const float x = xs[((nd.y >> 16) & 0x7fffu) * 256 + tid];
      const float thr = __uint_as_float(nd.x);
      const bool right = (nd.y >> 31) ? (x == thr) : !(x <= thr);
      nd = nodes[(nd.y & 0xffffu) + (right ? 1u : 0u)];
    }
    const unsigned leaf = min(nd.x, (unsigned)(tc.n_leaves - 1));  // (always nd.x on a validated forest)
    const double p = __longlong_as_double((long long)cur[tc.n_nodes + leaf]);
    if (LEAVES && valid) a.leaves_out[(size_t)rloc * a.T + t] = p;
    const double dlt = p - mean;
    mean = fma(dlt, tc.inv_count, mean);
    M2 = fma(dlt, p - mean, M2);
    if (t + 1 < a.T) {
#pragma unroll
      for (int j = 0; j < FOREST_STAGE; ++j) {
        const int i = tid + 256 * j;
        if (i < nw_next) nxt[i] = stage[j];
      }
      for (int i = tid + 256 * FOREST_STAGE; i < nw_next; i += 256) nxt[i] = g[i];
    }
    __syncthreads();
  }

  double y_hat = 0.0, sd = 0.0;
  if (valid) {
    const double mu = mean;
    double var = M2 / ((double)a.T - 1.0);
    if (!(var > 0.0)) var = 0.0;
    const double sdev = sqrt(var);
    const double mse = sdev * sdev;
    if (a.mu_out) a.mu_out[row] = mu;
    if (a.mse_out) a.mse_out[row] = mse;
    y_hat = a.minimize ? mu : -1 * mu;
    sd = sqrt(mse);
  }
  for (int c = 0; c < a.q; ++c) {
    double v = -INFINITY;
    int64_t idx = INT64_MAX;
    if (valid) {
      v = acq_value(a.acq_id[c], a.acq_par[c], y_hat, sd, a.plugin, 1e8);
      idx = row;
      if (a.acq_out) a.acq_out[(size_t)c * a.M + row] = v;
    }
    const ArgMax best = block_argmax(v, idx, sv, si);
    if (tid == 0) {
      a.blk_val[(size_t)c * a.nblk_total + blockIdx.x] = best.v;
      a.blk_idx[(size_t)c * a.nblk_total + blockIdx.x] = best.i;
    }
    __syncthreads();
  }
}

size_t forest_lds_bytes(int d, int tree_words) { return (size_t)2 * tree_words * 8 + (size_t)d * 256 * 4; }

hipError_t launch_forest(const ForestArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.nrows + 255) / 256);
  const size_t lds = forest_lds_bytes(a.d, a.tree_words);
  if (lds > 64 * 1024) {  // beyond the default dynamic LDS limit (the CU has 160 KB)
    const void* fn = a.leaves_out ? (const void*)k_forest<true> : (const void*)k_forest<false>;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (a.leaves_out)
    hipLaunchKernelGGL(k_forest<true>, dim3(nblk), 256, lds, st, a);
  else
    hipLaunchKernelGGL(k_forest<false>, dim3(nblk), 256, lds, st, a);
  return hipGetLastError();
}

}  // namespace bogp
