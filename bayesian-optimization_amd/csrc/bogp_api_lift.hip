// bogp_api_lift.hip -- the C ABI of libbogp.so (include/bogp.h) for searches in a REDUCED space (PCA-BO, extension.py:56-86,
// 113-133): bogp_lift_set / bogp_lift_clear / bogp_lift_sweep_topk / bogp_lift_last.  A lifted sweep decides the box
// feasibility of all M candidates first (kernels_lift.hip), runs the posterior sweep of bogp_api_sweep.hip on the feasible rows
// only, and ranks criterion values and penalties together.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

extern "C" int bogp_lift_set(bogp_handle* h, int D, const double* A, const double* mean, const double* center, const double* lo,
                             const double* hi) {
  if (!h) return BOGP_ERR_INVALID;
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_set: the handle carries a forest model; a lift serves a Gaussian process only");
  if (!h->dX || h->d <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: call bogp_set_train first (the reduced dimension r is the model's d)");
  if (!A || !mean || !lo || !hi) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: A, mean, lo and hi must be non-null");
  const int r = h->d;
  if (D < 1) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: D = %d must be positive", D);
  if (D > BOGP_MAX_DIM) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_set: D = %d exceeds BOGP_MAX_DIM = %d", D, BOGP_MAX_DIM);
  if (r > BOGP_LIFT_MAX_R) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_set: r = %d reduced dimensions exceed BOGP_LIFT_MAX_R = %d (a candidate row is held in registers)", r, BOGP_LIFT_MAX_R);
  if ((long long)r * D > BOGP_LIFT_MAX_RD) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_set: r x D = %d x %d exceeds BOGP_LIFT_MAX_RD = %d (A is staged in LDS)", r, D, BOGP_LIFT_MAX_RD);
  for (int i = 0; i < r * D; ++i)
    if (!std::isfinite(A[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: A[%d][%d] is not finite", i / D, i % D);
  for (int i = 0; i < D; ++i) {
    if (!std::isfinite(mean[i]) || (center && !std::isfinite(center[i]))) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: mean / center %d is not finite", i);
    if (std::isnan(lo[i]) || std::isnan(hi[i]) || !(lo[i] <= hi[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_set: bad bounds in dimension %d", i);
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<double> blk((size_t)r * D + 4 * (size_t)D, 0.0);
  double* p = blk.data();
  memcpy(p, A, (size_t)r * D * sizeof(double));
  p += (size_t)r * D;
  memcpy(p, mean, D * sizeof(double));
  if (center) memcpy(p + D, center, D * sizeof(double));
  memcpy(p + 2 * D, lo, D * sizeof(double));
  memcpy(p + 3 * D, hi, D * sizeof(double));
  h->lift_D = 0;
  int e = h->dlift.ensure(h, blk.size());
  if (e) return e;
  HIPCHK(h, hipStreamSynchronize(h->stream));  // (a queued sweep may still read the old block)
  HIPCHK(h, hipMemcpy(h->dlift, blk.data(), blk.size() * sizeof(double), hipMemcpyHostToDevice));
  h->lift_D = D;
  h->lift_r = r;
  return BOGP_OK;
}

extern "C" int bogp_lift_clear(bogp_handle* h) {
  if (!h) return BOGP_ERR_INVALID;
  h->lift_D = h->lift_r = 0;
  return BOGP_OK;
}

extern "C" int bogp_lift_last(bogp_handle* h, int64_t* n_feasible, double* filter_ms, double* merge_ms) {
  if (!h) return BOGP_ERR_INVALID;
  if (n_feasible) *n_feasible = h->lift_n_feasible;
  if (filter_ms) *filter_ms = h->lift_filter_ms;
  if (merge_ms) *merge_ms = h->lift_merge_ms;
  return BOGP_OK;
}

namespace {
// the compact buffer stands in for the handle's candidates while run_sweep works on the survivors; put back on every exit path
struct CandidateSwap {
  bogp_handle* h;
  const double* dXs;
  int64_t M;
  CandidateSwap(bogp_handle* h_, const double* Zc, int64_t Mf) : h(h_), dXs(h_->dXs), M(h_->M) {
    h->dXs = Zc;
    h->M = Mf;
  }
  ~CandidateSwap() {
    h->dXs = dXs;
    h->M = M;
  }
};
}  // namespace

extern "C" int bogp_lift_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                                    int k, double* best_val, int64_t* best_idx, int64_t* n_feasible, double* value_out,
                                    double* penalty_out) {
  if (!h) return BOGP_ERR_INVALID;
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_sweep_topk: the handle carries a forest model; a lifted sweep serves a Gaussian process only");
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_lift_sweep_topk: a lifted sweep runs on one rank (the communicator has %d)", h->comm_world);
  if (h->lift_D <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_sweep_topk: no lift: call bogp_lift_set first");
  if (k <= 0 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_sweep_topk: k = %d outside [1, %d]", k, BOGP_MAX_TOPK);
  if (q <= 0 || q > BOGP_MAX_Q || !acq_id || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_sweep_topk: 0 < q <= %d and non-null acq_id/best_val/best_idx required", BOGP_MAX_Q);
  if (int ec = check_criteria(h, q, acq_id, acq_par)) return ec;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "no committed model: call bogp_commit first");
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "no candidates: call bogp_candidates_upload/bind first");
  if (h->lift_r != h->d) FAIL(h, BOGP_ERR_INVALID, "bogp_lift_sweep_topk: the lift was set for r = %d, the model has d = %d: call bogp_lift_set again", h->lift_r, h->d);
  HIPCHK(h, hipSetDevice(h->device));
  invalidate_sweep_results(h);
  int e = candidates_ready(h);  // the filter reads every row
  if (e) return e;
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  const int r = h->d;
  const int64_t nblk = (M + 255) / 256;
  enum { L_FILTER, L_MERGE };  // kinds of the spans on h->lift_timer
  SpanTimer& tm = h->lift_timer;
  tm.begin();
  int f0 = 0, f1 = 0, m0 = 0, m1 = 0;
  if ((e = h->dlift_pen.ensure(h, (size_t)M))) return e;
  if ((e = h->dlift_cnt.ensure(h, (size_t)nblk))) return e;
  if ((e = h->dlift_off.ensure(h, (size_t)nblk + 1))) return e;
  if ((e = h->dlift_val.ensure(h, (size_t)q * M))) return e;

  // 1. feasibility of all M rows, the scan of the workgroup counts, M_f to the host (it sizes the compact buffers and the sweep)
  LiftArgs la;
  la.Z = h->dXs; la.M = M; la.r = r; la.D = h->lift_D; la.lift = h->dlift; la.penalty = h->dlift_pen; la.blk_count = h->dlift_cnt;
  if ((e = tm.mark(h, st, &f0))) return e;
  HIPCHK(h, launch_lift_penalty(la, st));
  HIPCHK(h, launch_lift_scan(h->dlift_cnt, nblk, h->dlift_off, st));
  int64_t Mf = 0;
  HIPCHK(h, hipMemcpyAsync(&Mf, h->dlift_off + nblk, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (Mf < 0 || Mf > M) FAIL(h, BOGP_ERR_HIP, "bogp_lift_sweep_topk: the scan returned %lld feasible rows of %lld", (long long)Mf, (long long)M);
  // 2. the feasible rows in their original order
  if (Mf > 0) {
    if ((e = h->dlift_Z.ensure(h, (size_t)Mf * r))) return e;
    if ((e = h->dlift_map.ensure(h, (size_t)Mf))) return e;
    HIPCHK(h, launch_lift_compact(h->dXs, M, r, h->dlift_pen, h->dlift_off, h->dlift_Z, h->dlift_map, st));
  }
  if ((e = tm.mark(h, st, &f1))) return e;
  tm.span(L_FILTER, f0, f1);
  // 3. the posterior sweep on the survivors, its q x M_f values kept on the device
  if (Mf > 0) {
    CandidateSwap swap(h, h->dlift_Z, Mf);
    SweepRequest rq;
    rq.q = q; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin; rq.minimize = minimize;
    rq.want_acq_out = true; rq.sync = false;
    const int rc = run_sweep(h, rq);
    if (rc) return rc;
  } else {
    clear_sweep_timing(h);
  }
  // 4. criterion values and penalties side by side over all M rows, ranked as bogp_sweep_topk ranks
  if ((e = tm.mark(h, st, &m0))) return e;
  HIPCHK(h, launch_lift_merge(h->dlift_pen, M, h->dacq_out, h->dlift_map, Mf, q, h->dlift_val, st));
  if ((e = rank_stored_values(h, h->dlift_val, M, q, k, st))) return e;
  if ((e = tm.mark(h, st, &m1))) return e;
  tm.span(L_MERGE, m0, m1);
  HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)q * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)q * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  pad_short_ranks(best_val, best_idx, q * k);
  h->lift_n_feasible = Mf;
  h->lift_filter_ms = tm.sum(L_FILTER);
  h->lift_merge_ms = tm.sum(L_MERGE);
  if (n_feasible) *n_feasible = Mf;
  if (value_out) HIPCHK(h, hipMemcpy(value_out, h->dlift_val, (size_t)q * M * sizeof(double), hipMemcpyDeviceToHost));
  if (penalty_out) HIPCHK(h, hipMemcpy(penalty_out, h->dlift_pen, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}
