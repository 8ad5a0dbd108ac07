// kernels_forest_ehvi.hip -- a packed regression forest with m outputs over the candidates: traversal, moments over the trees per
// output, expected hypervolume improvement over the cells, argmax (gfx950).
//
// Replaces, per candidate row, RandomForest.predict(X, eval_MSE=True) of a forest fitted on y (N, m) (surrogate/random_forest.py:
// 141-155: mean over the T trees and std(ddof = 1)^2 over the trees, per output -- scikit-learn grows ONE tree structure whose
// leaves hold m values, tree_.value (n_nodes, m, 1)) and, on these moments, EHVI.forward (multi_objective/analytic.py:223-274)
// through ehvi_cells of bogp_device.h, the cell loop k_ehvi runs on a Gaussian process's moments; then np.argmax over the rows into
// the per-block records k_argmax_final / the top-k passes read.
//
// Layout: k_forest's (kernels_forest.hip).  One lane = one row, 256 rows a workgroup; the row's features in LDS as float32,
// feature-major; the forest streamed one tree at a time through two LDS buffers, the next tree's words staged in registers behind
// the walk, one barrier a tree; the walk bounded by the tree's depth; both node tests.  A packed tree is
//   [n_nodes records | n_leaves x MT values],  values LEAF-major: a lane reads its leaf's MT doubles from consecutive LDS words.
// A leaf record's thr word is the index of its leaf; its values start at word n_nodes + MT * index.
//
// Moments, per output k: Welford's update in tree order with the tabled reciprocal, var = M2 / (T - 1) clamped at 0,
// MSE = sqrt(var)^2 -- k_forest's arithmetic, once per output.  sd_k = sqrt(fmax(MSE_k, 1e-9)) (analytic.py:233); trees that all
// agree give MSE = 0 exactly and sd = sqrt(1e-9).  A row's result is a function of the row and the forest alone -- same order in
// every lane, no atomics -- so rows with equal leaves get equal bits, and exact ties resolve to the lower index as np.argmax does.
#include "bogp_device.h"
#include "bogp_internal.h"

namespace bogp {

constexpr int FOREST_EHVI_STAGE = 4;  // words of the next tree a lane holds in registers during the walk (as FOREST_STAGE of k_forest)

template <int MT, bool LEAVES>
__global__ __launch_bounds__(256) void k_forest_ehvi(ForestEhviArgs a) {
  extern __shared__ unsigned long long forest_ehvi_smem[];
  __shared__ double sv[4];
  __shared__ int64_t si[4];
  unsigned long long* const buf0 = forest_ehvi_smem;
  unsigned long long* const buf1 = forest_ehvi_smem + a.tree_words;
  float* xs = (float*)(forest_ehvi_smem + 2 * (size_t)a.tree_words);  // [d][256]
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
    const int nw = t0.n_nodes + MT * t0.n_leaves;
    for (int i = tid; i < nw; i += 256) buf0[i] = a.words[(size_t)t0.first + i];
  }
  __syncthreads();

  double mean[MT], M2[MT];
#pragma unroll
  for (int k = 0; k < MT; ++k) mean[k] = M2[k] = 0.0;
  for (int t = 0; t < a.T; ++t) {
    const unsigned long long* cur = (t & 1) ? buf1 : buf0;
    unsigned long long* nxt = (t & 1) ? buf0 : buf1;
    const ForestTree tc = a.tree[t];
    unsigned long long stage[FOREST_EHVI_STAGE];
    int nw_next = 0;
    const unsigned long long* g = a.words;
    if (t + 1 < a.T) {
      const ForestTree tn = a.tree[t + 1];
      nw_next = tn.n_nodes + MT * tn.n_leaves;
      g = a.words + (size_t)tn.first;
#pragma unroll
      for (int j = 0; j < FOREST_EHVI_STAGE; ++j) {
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
    const unsigned long long* lv = cur + tc.n_nodes + (size_t)MT * leaf;
#pragma unroll
    for (int k = 0; k < MT; ++k) {
      const double p = __longlong_as_double((long long)lv[k]);
      if (LEAVES && valid) a.leaves_out[((size_t)rloc * a.T + t) * MT + k] = p;
      const double dlt = p - mean[k];
      mean[k] = fma(dlt, tc.inv_count, mean[k]);
      M2[k] = fma(dlt, p - mean[k], M2[k]);
    }
    if (t + 1 < a.T) {
#pragma unroll
      for (int j = 0; j < FOREST_EHVI_STAGE; ++j) {
        const int i = tid + 256 * j;
        if (i < nw_next) nxt[i] = stage[j];
      }
      for (int i = tid + 256 * FOREST_EHVI_STAGE; i < nw_next; i += 256) nxt[i] = g[i];
    }
    __syncthreads();
  }

  double sd[MT];
#pragma unroll
  for (int k = 0; k < MT; ++k) {
    double var = M2[k] / ((double)a.T - 1.0);
    if (!(var > 0.0)) var = 0.0;
    const double sdev = sqrt(var);
    const double mse = sdev * sdev;
    if (valid) {
      if (a.mu_out) a.mu_out[(size_t)row * MT + k] = mean[k];
      if (a.mse_out) a.mse_out[(size_t)row * MT + k] = mse;
    }
    sd[k] = sqrt(fmax(mse, 1e-9));
  }
  if (a.C <= 0) return;  // moments only (uniform: a kernel argument)

  double v = -INFINITY;
  int64_t idx = INT64_MAX;
  if (valid) {
    v = ehvi_cells<MT>(a.lower, a.upper, a.C, mean, sd);
    idx = row;
    if (a.ehvi_out) a.ehvi_out[row] = v;
  }
  const ArgMax best = block_argmax(v, idx, sv, si);
  if (tid == 0) {
    a.blk_val[blockIdx.x] = best.v;
    a.blk_idx[blockIdx.x] = best.i;
  }
}

template <int MT>
static hipError_t launch_forest_ehvi_m(const ForestEhviArgs& a, hipStream_t st) {
  const unsigned nblk = (unsigned)((a.nrows + 255) / 256);
  const size_t lds = forest_lds_bytes(a.d, a.tree_words);
  auto fn = a.leaves_out ? k_forest_ehvi<MT, true> : k_forest_ehvi<MT, false>;
  if (lds > 64 * 1024) {  // beyond the default dynamic LDS limit (the CU has 160 KB)
    const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(fn, dim3(nblk), 256, lds, st, a);
  return hipGetLastError();
}

hipError_t launch_forest_ehvi(const ForestEhviArgs& a, hipStream_t st) {
  switch (a.m) {
    case 2: return launch_forest_ehvi_m<2>(a, st);
    case 3: return launch_forest_ehvi_m<3>(a, st);
    case 4: return launch_forest_ehvi_m<4>(a, st);
    case 5: return launch_forest_ehvi_m<5>(a, st);
    case 6: return launch_forest_ehvi_m<6>(a, st);
    case 7: return launch_forest_ehvi_m<7>(a, st);
    case 8: return launch_forest_ehvi_m<8>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bogp
