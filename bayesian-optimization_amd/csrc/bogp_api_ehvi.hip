// bogp_api_ehvi.hip -- the C ABI of libbogp.so (include/bogp.h) for the multi-objective criterion: bogp_sweep_ehvi, the
// expected hypervolume improvement of an m-target model over the current candidates, bogp_sweep_ehvi_grid, the same criterion
// over the grid form of the cells, and bogp_sweep_ehvi_constrained_grid, that form under modelled constraints.  All run the chunked sweep
// of bogp_api_sweep.hip (producer -> contraction per chunk) with their kernel -- k_ehvi (kernels_ehvi.hip), k_ehvi_grid
// (kernels_ehvi_grid.hip), k_ehvi_constrained_grid (kernels_ehvi_constrained_grid.hip) -- in place of k_acquisition.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

// What both entries refuse alike, in bogp_sweep_ehvi's order, in two parts: the entry's own check of its cell count stands between them
static int check_ehvi_model(bogp_handle* h, const char* who, int m) {
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set) and EHVI has no lifted sweep: call bogp_lift_clear first", who);
  if (h->n_t < 2) FAIL(h, BOGP_ERR_INVALID, "%s: the committed model has %d target; EHVI needs 2 .. %d", who, h->n_t, BOGP_MAX_TARGETS);
  if (m != h->n_t) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d but the committed model has %d targets", who, m, h->n_t);
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d outside [2, %d]", who, m, BOGP_MAX_TARGETS);
  return BOGP_OK;
}
static int check_ehvi_request(bogp_handle* h, const char* who, int m, int k, bool pointers, const char* names) {
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!pointers) FAIL(h, BOGP_ERR_INVALID, "%s: %s must be non-null", who, names);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: several targets take the constant trend only (gpr.py:787)", who);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  return BOGP_OK;
}

// ... and their common tail: the sweep with the entry's kernel (rq.eh or rq.eg set by the caller), the downloads, the k winners
static int run_ehvi_sweep(bogp_handle* h, SweepRequest& rq, int m, int k, double* best_val, int64_t* best_idx, double* ehvi_out, double* mu_out,
                          double* mse_out) {
  hipStream_t st = h->stream;
  invalidate_sweep_results(h);  // dbest_* are overwritten and hold no single-target winners afterwards
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  rq.want_out = mu_out || mse_out; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0;
  int rc = run_sweep(h, rq);
  if (rc) return rc;
  const int64_t M = h->M;
  // (the downloads are queued in front of the winners: fetch_winners waits for the stream)
  if (ehvi_out) HIPCHK(h, hipMemcpyAsync(ehvi_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mu_out) HIPCHK(h, hipMemcpyAsync(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  return fetch_winners(h, 1, k, h->dacq_out, best_val, best_idx, st);
}

// What both grid entries do alike with a grid over m axes' worth of targets (m - 1 axes and the last axis' values): its refusals in
// bogp_sweep_ehvi_grid's order, the thresholds and last_idx into dehvi_grid / dehvi_grid_idx, and the grid fields of the kernel's
// arguments (ga: EhviGridArgs or ConstrainedEhviGridArgs, zeroed by the caller) -- the kernel's variant among them
template <class GridArgs>
static int stage_ehvi_grid(bogp_handle* h, const char* who, int m, const int* n_cells, const double* edges, int V, const double* last_val,
                           const int32_t* last_idx, GridArgs& ga) {
  if (!n_cells) FAIL(h, BOGP_ERR_INVALID, "%s: n_cells must be non-null", who);
  long long C = 1;  // (every factor and every product so far is at most 65536: no wrap-around)
  for (int a = 0; a < m - 1; ++a) {
    if (n_cells[a] < 1) FAIL(h, BOGP_ERR_INVALID, "%s: axis %d has %d intervals; at least 1", who, a, n_cells[a]);
    if (n_cells[a] > BOGP_MAX_EHVI_CELLS || (C *= n_cells[a]) > BOGP_MAX_EHVI_CELLS)
      FAIL(h, BOGP_ERR_INVALID, "%s: the axes up to axis %d give more than %d columns", who, a, BOGP_MAX_EHVI_CELLS);
  }
  if (!edges || !last_val || !last_idx) FAIL(h, BOGP_ERR_INVALID, "%s: edges, last_val and last_idx must be non-null", who);
  std::vector<double> pts;  // the thresholds of a row's table: per axis its finite edges, then last_val (EhviGridArgs)
  const double* ed = edges;
  for (int a = 0; a < m - 1; ++a) {
    const int n = ga.n[a] = n_cells[a];
    ga.off[a] = (int)pts.size();
    if (!std::isfinite(ed[0])) FAIL(h, BOGP_ERR_INVALID, "%s: axis %d: the first edge is not finite", who, a);
    for (int i = 1; i <= n; ++i)
      if (!(ed[i] > ed[i - 1])) FAIL(h, BOGP_ERR_INVALID, "%s: axis %d: edge %d (%g) is not above edge %d (%g)", who, a, i, ed[i], i - 1, ed[i - 1]);
    if (!(std::isinf(ed[n]) && ed[n] > 0)) FAIL(h, BOGP_ERR_INVALID, "%s: axis %d: the last edge (%g) is not +inf", who, a, ed[n]);
    pts.insert(pts.end(), ed, ed + n);
    ed += n + 1;
  }
  if (V < 1 || V > C) FAIL(h, BOGP_ERR_INVALID, "%s: V = %d values outside [1, %lld], the columns", who, V, C);
  for (int v = 0; v < V; ++v) {
    if (!std::isfinite(last_val[v])) FAIL(h, BOGP_ERR_INVALID, "%s: last_val[%d] is not finite", who, v);
    if (v > 0 && !(last_val[v] > last_val[v - 1])) FAIL(h, BOGP_ERR_INVALID, "%s: last_val[%d] (%g) is not above last_val[%d] (%g)", who, v, last_val[v], v - 1, last_val[v - 1]);
  }
  for (long long c = 0; c < C; ++c)
    if (last_idx[c] < 0 || last_idx[c] >= V) FAIL(h, BOGP_ERR_INVALID, "%s: last_idx[%lld] = %d outside [0, %d)", who, c, (int)last_idx[c], V);
  ga.off[m - 1] = (int)pts.size();
  pts.insert(pts.end(), last_val, last_val + V);
  ga.E = (int)pts.size(); ga.C = (int)C;
  // the kernel's variant is a function of E alone (kernels_ehvi_grid.hip: ORDER); step: the group's size in the columns' mixed radix
  ga.group = ga.E <= 12 * 16 ? 16 : 64;
  ga.tabled = ga.E <= 12 * ga.group;
  for (int a = m - 2, rem = ga.group; a >= 0; --a) {
    ga.step[a] = rem % ga.n[a];
    rem /= ga.n[a];
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  static_assert(sizeof(int) == sizeof(int32_t), "last_idx is copied as it stands");
  int e;
  if ((e = h->dehvi_grid.ensure(h, pts.size())) || (e = h->dehvi_grid_idx.ensure(h, (size_t)C))) return e;
  // (the grid is the kernel's argument: copied in stream order, before the kernels that read it, and waited for -- pts dies here)
  HIPCHK(h, hipMemcpyAsync(h->dehvi_grid, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(h->dehvi_grid_idx, last_idx, (size_t)C * sizeof(int), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));
  ga.pts = h->dehvi_grid; ga.last_idx = h->dehvi_grid_idx;
  return BOGP_OK;
}

extern "C" int bogp_sweep_ehvi(bogp_handle* h, int m, int C, const double* lower, const double* upper, int k, double* best_val,
                               int64_t* best_idx, double* ehvi_out, double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_ehvi";
  int e;
  if ((e = check_ehvi_model(h, who, m))) return e;
  if (C < 1 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: C = %d cells outside [1, %d]", C, BOGP_MAX_EHVI_CELLS);
  if ((e = check_ehvi_request(h, who, m, k, lower && upper && best_val && best_idx, "lower, upper, best_val and best_idx"))) return e;
  const size_t nb = (size_t)C * m;
  if ((e = check_ehvi_cells(h, who, nb, lower, upper))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  if ((e = stage_ehvi_cells(h, lower, upper, nb, h->stream))) return e;
  EhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  multi_target_model(h, ea);
  ea.C = C; ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + nb;
  SweepRequest rq;
  rq.eh = &ea;
  return run_ehvi_sweep(h, rq, m, k, best_val, best_idx, ehvi_out, mu_out, mse_out);
}

extern "C" int bogp_sweep_ehvi_grid(bogp_handle* h, int m, const int* n_cells, const double* edges, int V, const double* last_val,
                                    const int32_t* last_idx, int k, double* best_val, int64_t* best_idx, double* ehvi_out, double* mu_out,
                                    double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_ehvi_grid";
  int e;
  if ((e = check_ehvi_model(h, who, m)) || (e = check_ehvi_request(h, who, m, k, best_val && best_idx, "best_val and best_idx"))) return e;
  EhviGridArgs ga;
  memset(&ga, 0, sizeof(ga));
  if ((e = stage_ehvi_grid(h, who, m, n_cells, edges, V, last_val, last_idx, ga))) return e;
  multi_target_model(h, ga);
  SweepRequest rq;
  rq.eg = &ga;
  return run_ehvi_sweep(h, rq, m, k, best_val, best_idx, ehvi_out, mu_out, mse_out);
}

// feasibility-weighted EHVI over the grid of the feasible front's cells: bogp_sweep_ehvi_constrained's refusals
// (bogp_api_ehvi_constrained.hip) and then the grid's, over the m_obj objectives; k_ehvi_constrained_grid in the chunk loop
extern "C" int bogp_sweep_ehvi_constrained_grid(bogp_handle* h, int m_obj, const int* n_cells, const double* edges, int V, const double* last_val,
                                                const int32_t* last_idx, int n_con, const double* lo, const double* hi, int k, double* best_val,
                                                int64_t* best_idx, double* val_out, double* pof_out, double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_ehvi_constrained_grid";
  int e;
  if ((e = check_ehvi_constrained_model(h, who, m_obj, n_con))) return e;
  const int m = h->n_t;
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!lo || !hi || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: lo, hi, best_val and best_idx must be non-null", who);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  if ((e = check_constraint_bounds(h, who, n_con, lo, hi))) return e;
  ConstrainedEhviGridArgs ga;
  memset(&ga, 0, sizeof(ga));
  if ((e = stage_ehvi_grid(h, who, m_obj, n_cells, edges, V, last_val, last_idx, ga))) return e;
  if (pof_out && (e = h->dpof_out.ensure(h, (size_t)h->M))) return e;
  ga.gamma = h->dgamma_base; ga.ld_gamma = h->Np; ga.N = h->N; ga.m = m; ga.m_obj = m_obj;
  for (int t = 0; t < m; ++t) ga.sigma2[t] = h->sigma2_t[t];
  for (int j = 0; j < n_con; ++j) { ga.lo[j] = lo[j]; ga.hi[j] = hi[j]; }
  ga.pof_out = pof_out ? h->dpof_out.ptr : nullptr;
  SweepRequest rq;
  rq.ecg = &ga;
  return run_ehvi_constrained_sweep(h, rq, m, k, best_val, best_idx, val_out, pof_out, mu_out, mse_out);
}
