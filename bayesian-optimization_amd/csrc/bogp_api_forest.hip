// bogp_api_forest.hip -- the C ABI of libbogp.so (include/bogp.h) for the second model kind of a handle, a packed regression
// forest: bogp_forest_set (validation + packing, host only), bogp_forest_predict / _leaves / _sweep_topk (k_forest of
// kernels_forest.hip over the current candidates, then the argmax / top-k passes of kernels_acq.hip) and the candidate generator
// of mixed spaces, bogp_candidates_generate_mixed; and, for a forest whose leaves hold several outputs, bogp_forest_set_multi (the same
// validation and packing with m values a leaf), bogp_forest_predict_multi / _leaves_multi / _sweep_ehvi (k_forest_ehvi of
// kernels_forest_ehvi.hip, then the same argmax / top-k passes).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

bool bogp::has_dim(const bogp_handle* h) { return h->dX != nullptr || h->forest_T > 0; }

static constexpr size_t FOREST_LDS_LIMIT = 160 * 1024 - 128;  // the CU's LDS less the kernel's static words

// largest float32 that is <= t (t finite or infinite, not NaN): x <= t holds for a float32 x exactly when x <= this
static float round_down_f32(double t) {
  float f = (float)t;
  if ((double)f > t) f = std::nextafterf(f, -INFINITY);
  return f;
}

// validation walk + packing of bogp_forest_set (m = 1) and bogp_forest_set_multi (m outputs a leaf, value nodes x m row-major)
static int forest_set_impl(bogp_handle* h, const char* who, int T, int d, int m, const int64_t* tree_offset, const int32_t* feature,
                           const double* threshold, const int32_t* left, const int32_t* right, const double* value,
                           const int32_t* test) {
  if (h->dX) FAIL(h, BOGP_ERR_INVALID, "%s: the handle holds a Gaussian-process training set; a forest takes a handle of its own", who);
  if (T < 2) FAIL(h, BOGP_ERR_INVALID, "%s: T = %d trees; the variance over the trees (ddof = 1) needs T >= 2", who, T);
  if (d < 1 || d > BOGP_MAX_DIM) FAIL(h, BOGP_ERR_INVALID, "%s: d = %d outside [1, %d]", who, d, BOGP_MAX_DIM);
  if (!tree_offset || !feature || !threshold || !left || !right || !value) FAIL(h, BOGP_ERR_INVALID, "%s: tree_offset, feature, threshold, left, right and value must be non-null", who);
  if (tree_offset[0] != 0) FAIL(h, BOGP_ERR_INVALID, "%s: tree_offset[0] must be 0", who);
  std::vector<unsigned long long> words;
  std::vector<ForestTree> trees((size_t)T);
  int tree_words = 0, depth_max = 0;
  int64_t nodes_total = 0, leaves_total = 0;
  std::vector<int> order, newidx, dep;
  for (int t = 0; t < T; ++t) {
    const int64_t o = tree_offset[t], n64 = tree_offset[t + 1] - o;
    if (n64 < 1 || n64 > 65535) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d has %lld nodes (1 .. 65535)", who, t, (long long)n64);
    const int n = (int)n64;
    // breadth-first walk from the root: every node is reached at most once (no cycle, no shared subtree), the children of a
    // node get adjacent new indices, unreachable nodes are dropped, and the depth of the tree bounds the kernel's walk
    order.assign(1, 0);
    newidx.assign((size_t)n, -1);
    dep.assign((size_t)n, 0);
    newidx[0] = 0;
    int next = 1, nleaf = 0, depth = 0;
    for (size_t qi = 0; qi < order.size(); ++qi) {
      const int u = order[qi];
      const int l = left[o + u], r = right[o + u];
      if (l == -1) {
        if (r != -1) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d has a right child but no left child", who, t, u);
        for (int k = 0; k < m; ++k)
          if (!std::isfinite(value[(size_t)(o + u) * m + k])) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d leaf %d has a non-finite value", who, t, u);
        ++nleaf;
        continue;
      }
      if (l < 0 || l >= n || r < 0 || r >= n) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d has a child outside [0, %d)", who, t, u, n);
      if (l == r || newidx[l] != -1 || newidx[r] != -1) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d points at a node that is already reached (cycle or shared subtree)", who, t, u);
      if (feature[o + u] < 0 || feature[o + u] >= d) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d splits on feature %d outside [0, %d)", who, t, u, feature[o + u], d);
      const double thr = threshold[o + u];
      if (std::isnan(thr)) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d has a NaN threshold", who, t, u);
      if (test && test[o + u] != 0) {
        if (test[o + u] != 1) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d has test %d (0: x <= thr, 1: x != thr)", who, t, u, test[o + u]);
        if (!(thr >= 0 && thr < 16777216.0 && thr == std::floor(thr))) FAIL(h, BOGP_ERR_INVALID, "%s: tree %d node %d: a level index must be an integer in [0, 2^24)", who, t, u);
      }
      newidx[l] = next;
      newidx[r] = next + 1;
      next += 2;
      dep[l] = dep[r] = dep[u] + 1;
      if (dep[l] > depth) depth = dep[l];
      order.push_back(l);
      order.push_back(r);
    }
    const int nn = next;  // reachable nodes (<= n <= 65535: a child index fits 16 bits)
    const size_t base = words.size();
    const size_t nw = (size_t)nn + (size_t)m * nleaf;  // [records | leaves x m values, leaf-major]
    if (base + nw > (size_t)INT32_MAX) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the packed forest exceeds 2^31 words", who);
    words.resize(base + nw);
    int li = 0;
    for (size_t qi = 0; qi < order.size(); ++qi) {  // order[qi] has new index qi (children are appended pairwise as they are numbered)
      const int u = order[qi];
      uint32_t x, w;
      if (left[o + u] == -1) {
        x = (uint32_t)li;
        w = 0u;
        for (int k = 0; k < m; ++k) {
          double v = value[(size_t)(o + u) * m + k];
          unsigned long long bits;
          memcpy(&bits, &v, 8);
          words[base + nn + (size_t)m * li + k] = bits;
        }
        ++li;
      } else {
        const bool eq = test && test[o + u] == 1;
        const float tf = eq ? (float)threshold[o + u] : round_down_f32(threshold[o + u]);
        memcpy(&x, &tf, 4);
        w = (eq ? 0x80000000u : 0u) | ((uint32_t)feature[o + u] << 16) | (uint32_t)newidx[left[o + u]];
      }
      words[base + newidx[u]] = ((unsigned long long)w << 32) | x;  // uint2 {x, y} in memory order
    }
    trees[t] = ForestTree{(int)base, nn, nleaf, depth, 1.0 / (double)(t + 1), 0.0};
    if ((int)nw > tree_words) tree_words = (int)nw;
    if (depth > depth_max) depth_max = depth;
    nodes_total += nn;
    leaves_total += nleaf;
  }
  const size_t lds = forest_lds_bytes(d, tree_words);
  if (lds > FOREST_LDS_LIMIT)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: two buffers of the largest tree (%d words) and 256 rows of %d features need %zu bytes of LDS (limit %zu)", who, tree_words, d, lds, FOREST_LDS_LIMIT);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // a forest call in flight still reads the old forest
  int e;
  if ((e = h->dforest_words.ensure(h, words.size()))) return e;
  if ((e = h->dforest_tree.ensure(h, (size_t)T))) return e;
  HIPCHK(h, hipMemcpy(h->dforest_words, words.data(), words.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
  HIPCHK(h, hipMemcpy(h->dforest_tree, trees.data(), (size_t)T * sizeof(ForestTree), hipMemcpyHostToDevice));
  if (h->forest_T && d != h->d) {  // rows of another width are not candidates of this forest
    if (h->hXs_lazy) {
      HIPCHK(h, hipStreamSynchronize(h->stream_copy));
      h->hXs_lazy = nullptr;
    }
    h->dXs = nullptr;
    h->M = 0;
    h->h_xform.clear();
  }
  invalidate_sweep_results(h);
  h->forest_T = T;
  h->forest_m = m;
  h->d = d;
  h->forest_tree_words = tree_words;
  h->forest_depth = depth_max;
  h->forest_nodes = nodes_total;
  h->forest_leaves = leaves_total;
  return BOGP_OK;
}

extern "C" int bogp_forest_set(bogp_handle* h, int T, int d, const int64_t* tree_offset, const int32_t* feature,
                               const double* threshold, const int32_t* left, const int32_t* right, const double* value,
                               const int32_t* test) {
  if (!h) return BOGP_ERR_INVALID;
  return forest_set_impl(h, "bogp_forest_set", T, d, 1, tree_offset, feature, threshold, left, right, value, test);
}

extern "C" int bogp_forest_set_multi(bogp_handle* h, int T, int d, int m, const int64_t* tree_offset, const int32_t* feature,
                                     const double* threshold, const int32_t* left, const int32_t* right, const double* value,
                                     const int32_t* test) {
  if (!h) return BOGP_ERR_INVALID;
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_set_multi: m = %d outputs outside [2, %d] (one output: bogp_forest_set)", m, BOGP_MAX_TARGETS);
  return forest_set_impl(h, "bogp_forest_set_multi", T, d, m, tree_offset, feature, threshold, left, right, value, test);
}

extern "C" int bogp_forest_outputs(const bogp_handle* h) { return h && h->forest_T ? h->forest_m : 0; }

extern "C" int bogp_forest_info(const bogp_handle* h, int64_t* out) {
  if (!h || !out) return BOGP_ERR_INVALID;
  out[0] = h->forest_T;
  out[1] = h->forest_T ? h->d : 0;
  out[2] = h->forest_nodes;
  out[3] = h->forest_leaves;
  out[4] = h->forest_depth;
  out[5] = (h->forest_nodes + h->forest_leaves * h->forest_m) * 8 + (int64_t)h->forest_T * (int64_t)sizeof(ForestTree);
  out[6] = h->forest_T ? (int64_t)forest_lds_bytes(h->d, h->forest_tree_words) : 0;
  return BOGP_OK;
}

// one criteria span on the sweep's timer around a forest kernel (bogp_last_timing: acquisition_ms, one chunk), read when it is asked for
template <class Launch>
static int forest_span(bogp_handle* h, Launch launch) {
  h->timer.begin();
  if (int e = timed_span(h, h->timer, h->stream, T_CRITERIA, launch)) return e;
  h->n_chunks = 1; h->timing_pending = true;
  return BOGP_OK;
}

// k_forest over rows [row0, row0 + nrows) of the current candidates
static int run_forest(bogp_handle* h, const char* who, ForestArgs& a, int64_t row0, int64_t nrows) {
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "%s: no forest: call bogp_forest_set first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload / bind / generate_mixed first", who);
  if (h->hXs_lazy) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lazy upload is pending; forest calls take bogp_candidates_upload", who);
  if (row0 < 0 || nrows < 1 || row0 + nrows > h->M) FAIL(h, BOGP_ERR_INVALID, "%s: rows [%lld, %lld) outside the %lld candidates", who, (long long)row0, (long long)(row0 + nrows), (long long)h->M);
  a.Xs = h->dXs; a.M = h->M; a.row0 = row0; a.nrows = nrows; a.d = h->d;
  a.words = h->dforest_words; a.tree = h->dforest_tree; a.T = h->forest_T; a.tree_words = h->forest_tree_words;
  return forest_span(h, [&] { return launch_forest(a, h->stream); });
}

extern "C" int bogp_forest_predict(bogp_handle* h, double* mu, double* mse) {
  if (!h) return BOGP_ERR_INVALID;
  if (!mu) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_predict: mu must be non-null");
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_predict: no forest: call bogp_forest_set first");
  if (h->forest_m > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_forest_predict: the forest has %d outputs: call bogp_forest_predict_multi", h->forest_m);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_predict: no candidates");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t M = h->M;
  int e;
  if ((e = h->dmu_out.ensure(h, (size_t)M))) return e;
  if ((e = h->dmse_out.ensure(h, (size_t)M))) return e;
  ForestArgs a;
  memset(&a, 0, sizeof(a));
  a.mu_out = h->dmu_out; a.mse_out = mse ? h->dmse_out : nullptr; a.minimize = 1;
  if ((e = run_forest(h, "bogp_forest_predict", a, 0, M))) return e;
  HIPCHK(h, hipMemcpyAsync(mu, h->dmu_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (mse) HIPCHK(h, hipMemcpyAsync(mse, h->dmse_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BOGP_OK;
}

extern "C" int bogp_forest_leaves(bogp_handle* h, int64_t first_row, int n, double* per_tree) {
  if (!h) return BOGP_ERR_INVALID;
  if (!per_tree || n < 1) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_leaves: per_tree must be non-null and n > 0");
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_leaves: no forest: call bogp_forest_set first");
  if (h->forest_m > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_forest_leaves: the forest has %d outputs: call bogp_forest_leaves_multi", h->forest_m);
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)n * h->forest_T;
  int e;
  if ((e = h->dbatch.ensure(h, cnt))) return e;
  ForestArgs a;
  memset(&a, 0, sizeof(a));
  a.leaves_out = h->dbatch; a.minimize = 1;
  if ((e = run_forest(h, "bogp_forest_leaves", a, first_row, n))) return e;
  HIPCHK(h, hipMemcpyAsync(per_tree, h->dbatch, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BOGP_OK;
}

extern "C" int bogp_forest_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                                      int k, double* best_val, int64_t* best_idx, double* acq_out) {
  if (!h) return BOGP_ERR_INVALID;
  if (k <= 0 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: k = %d outside [1, %d]", k, BOGP_MAX_TOPK);
  if (q <= 0 || q > BOGP_MAX_Q || !acq_id || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: 0 < q <= %d and non-null acq_id / best_val / best_idx required", BOGP_MAX_Q);
  for (int i = 0; i < q; ++i) {
    if (acq_id[i] < 0 || acq_id[i] > 3) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: unknown acquisition id %d", acq_id[i]);
    const bool zero_ok = acq_id[i] == BOGP_ACQ_EPSILON_PI;  // epsilon = 0 is plain PI
    if (acq_id[i] != BOGP_ACQ_EI && (!acq_par || !(acq_par[i] > 0 || (zero_ok && acq_par[i] == 0))))
      FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: acquisition parameter %d must be > 0 (the reference asserts alpha/epsilon/t > 0)", i);
  }
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: no forest: call bogp_forest_set first");
  if (h->forest_m > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_forest_sweep_topk: the forest has %d outputs and the single-target criteria take one: call bogp_forest_sweep_ehvi", h->forest_m);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_sweep_topk: no candidates");
  HIPCHK(h, hipSetDevice(h->device));
  invalidate_sweep_results(h);
  const int64_t M = h->M, nblk = (M + 255) / 256;
  const bool keep = k > 1 || acq_out;
  hipStream_t st = h->stream;
  int e;
  if ((e = h->dblk_val.ensure(h, (size_t)q * (nblk + 1)))) return e;
  if ((e = h->dblk_idx.ensure(h, (size_t)q * (nblk + 1)))) return e;
  if ((e = h->dbest_val.ensure(h, BOGP_MAX_Q)) || (e = h->dbest_idx.ensure(h, BOGP_MAX_Q))) return e;
  if (keep && (e = h->dacq_out.ensure(h, (size_t)q * M))) return e;
  ForestArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q;
  for (int i = 0; i < q; ++i) {
    a.acq_id[i] = acq_id[i];
    a.acq_par[i] = acq_par ? acq_par[i] : 0.0;
  }
  a.plugin = plugin; a.minimize = minimize;
  a.acq_out = keep ? h->dacq_out : nullptr;
  a.blk_val = h->dblk_val; a.blk_idx = h->dblk_idx; a.nblk_total = nblk;
  if ((e = run_forest(h, "bogp_forest_sweep_topk", a, 0, M))) return e;
  // the block records -> the argmax per criterion (dbest_*: what bogp_exchange_argmax packs)
  HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, nblk, nblk, q, h->dbest_val, h->dbest_idx, st));
  if (acq_out) HIPCHK(h, hipMemcpyAsync(acq_out, h->dacq_out, (size_t)q * M * sizeof(double), hipMemcpyDeviceToHost, st));
  if ((e = fetch_winners(h, q, k, h->dacq_out, best_val, best_idx, st))) return e;  // (waits for the stream: acq_out is complete)
  h->last_q = q;
  if (k > 1) {
    h->last_topk_q = q;
    h->last_topk_k = k;
  }
  return BOGP_OK;
}

// ---- forests with several outputs: k_forest_ehvi (kernels_forest_ehvi.hip) -------------------------------------------------------
// the checks every multi-output call shares; launches k_forest_ehvi over rows [row0, row0 + nrows), timed as run_forest times k_forest
static int run_forest_ehvi(bogp_handle* h, const char* who, ForestEhviArgs& a, int64_t row0, int64_t nrows) {
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "%s: no forest: call bogp_forest_set_multi first", who);
  if (h->forest_m < 2) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the forest has one output: the one-output calls (bogp_forest_predict / _leaves / _sweep_topk) serve it", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload / bind / generate_mixed first", who);
  if (h->hXs_lazy) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lazy upload is pending; forest calls take bogp_candidates_upload", who);
  if (row0 < 0 || nrows < 1 || row0 + nrows > h->M) FAIL(h, BOGP_ERR_INVALID, "%s: rows [%lld, %lld) outside the %lld candidates", who, (long long)row0, (long long)(row0 + nrows), (long long)h->M);
  a.Xs = h->dXs; a.M = h->M; a.row0 = row0; a.nrows = nrows; a.d = h->d; a.m = h->forest_m;
  a.words = h->dforest_words; a.tree = h->dforest_tree; a.T = h->forest_T; a.tree_words = h->forest_tree_words;
  return forest_span(h, [&] { return launch_forest_ehvi(a, h->stream); });
}

// what run_forest_ehvi will refuse, asked before anything is allocated
static int forest_multi_ready(bogp_handle* h, const char* who) {
  if (!h->forest_T) FAIL(h, BOGP_ERR_INVALID, "%s: no forest: call bogp_forest_set_multi first", who);
  if (h->forest_m < 2) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the forest has one output: the one-output calls (bogp_forest_predict / _leaves / _sweep_topk) serve it", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload / bind / generate_mixed first", who);
  return BOGP_OK;
}

extern "C" int bogp_forest_predict_multi(bogp_handle* h, double* mu, double* mse) {
  if (!h) return BOGP_ERR_INVALID;
  if (!mu) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_predict_multi: mu must be non-null");
  int e;
  if ((e = forest_multi_ready(h, "bogp_forest_predict_multi"))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)h->M * h->forest_m;
  if ((e = h->dmu_out.ensure(h, cnt))) return e;
  if (mse && (e = h->dmse_out.ensure(h, cnt))) return e;
  ForestEhviArgs a;
  memset(&a, 0, sizeof(a));
  a.mu_out = h->dmu_out; a.mse_out = mse ? h->dmse_out : nullptr;
  if ((e = run_forest_ehvi(h, "bogp_forest_predict_multi", a, 0, h->M))) return e;
  HIPCHK(h, hipMemcpyAsync(mu, h->dmu_out, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (mse) HIPCHK(h, hipMemcpyAsync(mse, h->dmse_out, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BOGP_OK;
}

extern "C" int bogp_forest_leaves_multi(bogp_handle* h, int64_t first_row, int n, double* per_tree) {
  if (!h) return BOGP_ERR_INVALID;
  if (!per_tree || n < 1) FAIL(h, BOGP_ERR_INVALID, "bogp_forest_leaves_multi: per_tree must be non-null and n > 0");
  int e;
  if ((e = forest_multi_ready(h, "bogp_forest_leaves_multi"))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  const size_t cnt = (size_t)n * h->forest_T * h->forest_m;
  if ((e = h->dbatch.ensure(h, cnt))) return e;
  ForestEhviArgs a;
  memset(&a, 0, sizeof(a));
  a.leaves_out = h->dbatch;
  if ((e = run_forest_ehvi(h, "bogp_forest_leaves_multi", a, first_row, n))) return e;
  HIPCHK(h, hipMemcpyAsync(per_tree, h->dbatch, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BOGP_OK;
}

extern "C" int bogp_forest_sweep_ehvi(bogp_handle* h, int m, int C, const double* lower, const double* upper, int k, double* best_val,
                                      int64_t* best_idx, double* ehvi_out, double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_forest_sweep_ehvi";
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set) and EHVI has no lifted sweep: call bogp_lift_clear first", who);
  int e;
  if ((e = forest_multi_ready(h, who))) return e;
  if (m != h->forest_m) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d but the forest has %d outputs", who, m, h->forest_m);
  if (C < 1 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "%s: C = %d cells outside [1, %d]", who, C, BOGP_MAX_EHVI_CELLS);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!lower || !upper || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: lower, upper, best_val and best_idx must be non-null", who);
  const size_t nb = (size_t)C * m;
  if ((e = check_ehvi_cells(h, who, nb, lower, upper))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  invalidate_sweep_results(h);
  hipStream_t st = h->stream;
  const int64_t M = h->M, nblk = (M + 255) / 256;
  const bool keep = k > 1 || ehvi_out;
  if ((e = h->dblk_val.ensure(h, (size_t)(nblk + 1)))) return e;
  if ((e = h->dblk_idx.ensure(h, (size_t)(nblk + 1)))) return e;
  if ((e = h->dbest_val.ensure(h, BOGP_MAX_Q)) || (e = h->dbest_idx.ensure(h, BOGP_MAX_Q))) return e;
  if (keep && (e = h->dacq_out.ensure(h, (size_t)M))) return e;
  if (mu_out && (e = h->dmu_out.ensure(h, (size_t)M * m))) return e;
  if (mse_out && (e = h->dmse_out.ensure(h, (size_t)M * m))) return e;
  if ((e = stage_ehvi_cells(h, lower, upper, nb, st))) return e;
  ForestEhviArgs a;
  memset(&a, 0, sizeof(a));
  a.C = C; a.lower = h->dehvi_cells; a.upper = h->dehvi_cells + nb;
  a.ehvi_out = keep ? h->dacq_out : nullptr;
  a.mu_out = mu_out ? h->dmu_out : nullptr; a.mse_out = mse_out ? h->dmse_out : nullptr;
  a.blk_val = h->dblk_val; a.blk_idx = h->dblk_idx;
  if ((e = run_forest_ehvi(h, who, a, 0, M))) return e;
  HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, nblk, nblk, 1, h->dbest_val, h->dbest_idx, st));
  if (ehvi_out) HIPCHK(h, hipMemcpyAsync(ehvi_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mu_out) HIPCHK(h, hipMemcpyAsync(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  return fetch_winners(h, 1, k, h->dacq_out, best_val, best_idx, st);  // (waits for the stream: the three outputs are complete)
}

extern "C" int bogp_candidates_generate_mixed(bogp_handle* h, const int* kind, const double* lo, const double* hi, const int* n_levels,
                                              int64_t M, uint64_t seed, int64_t first_row) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_candidates_generate_mixed";
  if (!has_dim(h)) FAIL(h, BOGP_ERR_INVALID, "%s: call bogp_forest_set or bogp_set_train first (d is unknown)", who);
  if (!kind || !lo || !hi || !n_levels || M <= 0 || first_row < 0) FAIL(h, BOGP_ERR_INVALID, "%s: kind, lo, hi and n_levels must be non-null, M > 0, first_row >= 0", who);
  const int d = h->d;
  std::vector<double> spec((size_t)3 * d);
  for (int k = 0; k < d; ++k) {
    if (!(std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] <= hi[k])) FAIL(h, BOGP_ERR_INVALID, "%s: bad bounds in column %d", who, k);
    if (kind[k] == BOGP_COLUMN_REAL) {
      spec[2 * d + k] = 0.0;
    } else if (kind[k] == BOGP_COLUMN_DISCRETE) {
      if (n_levels[k] <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: column %d is discrete with n_levels = %d (must be > 0)", who, k, n_levels[k]);
      spec[2 * d + k] = (double)n_levels[k];
    } else {
      FAIL(h, BOGP_ERR_INVALID, "%s: column %d has kind %d (BOGP_COLUMN_REAL or BOGP_COLUMN_DISCRETE)", who, k, kind[k]);
    }
    spec[k] = lo[k];
    spec[d + k] = hi[k];
  }
  invalidate_sweep_results(h);
  HIPCHK(h, hipSetDevice(h->device));
  if (h->hXs_lazy) {  // pending copies of the old candidates must not land later
    HIPCHK(h, hipStreamSynchronize(h->stream_copy));
    h->hXs_lazy = nullptr;
  }
  int e;
  if ((e = h->dXs_owned.ensure(h, (size_t)M * d))) return e;
  if ((e = h->dbounds.ensure(h, (size_t)3 * d))) return e;
  HIPCHK(h, hipMemcpyAsync(h->dbounds, spec.data(), spec.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_generate_mixed(h->dXs_owned, M * d, d, h->dbounds, h->dbounds + d, h->dbounds + 2 * d, seed,
                                  (uint64_t)first_row * (uint64_t)d, h->stream));
  if (!h->h_xform.empty() && (int)h->h_xform.size() == 4 * d)
    HIPCHK(h, launch_candidates_transform(h->dXs_owned, M * d, d, h->dxform, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // spec is host memory of this call
  h->dXs = h->dXs_owned;
  h->M = M;
  return BOGP_OK;
}
