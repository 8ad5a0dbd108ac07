// bogp_api_ehvi.hip -- the C ABI of libbogp.so (include/bogp.h) for the multi-objective criterion: bogp_sweep_ehvi, the
// expected hypervolume improvement of an m-target model over the current candidates.  It runs the chunked sweep of
// bogp_api_sweep.hip (producer -> contraction per chunk) with k_ehvi (kernels_ehvi.hip) in place of k_acquisition.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

extern "C" int bogp_sweep_ehvi(bogp_handle* h, int m, int C, const double* lower, const double* upper, int k, double* best_val,
                               int64_t* best_idx, double* ehvi_out, double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: no committed model: call bogp_commit first");
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: no candidates: call bogp_candidates_upload/bind first");
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_ehvi: a lift is set (bogp_lift_set) and EHVI has no lifted sweep: call bogp_lift_clear first");
  if (h->n_t < 2) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: the committed model has %d target; EHVI needs 2 .. %d", h->n_t, BOGP_MAX_TARGETS);
  if (m != h->n_t) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: m = %d but the committed model has %d targets", m, h->n_t);
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: m = %d outside [2, %d]", m, BOGP_MAX_TARGETS);
  if (C < 1 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: C = %d cells outside [1, %d]", C, BOGP_MAX_EHVI_CELLS);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: k = %d outside [1, %d]", k, BOGP_MAX_TOPK);
  if (!lower || !upper || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: lower, upper, best_val and best_idx must be non-null");
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_ehvi: several targets take the constant trend only (gpr.py:787)");
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: the commit holds %d target variances", (int)h->sigma2_t.size());
  const size_t nb = (size_t)C * m;
  for (size_t i = 0; i < nb; ++i) {
    if (!std::isfinite(lower[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: lower bound %zu is not finite", i);
    if (std::isnan(upper[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: upper bound %zu is NaN", i);
    if (!(upper[i] >= lower[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_ehvi: upper bound %zu (%g) is below its lower bound (%g)", i, upper[i], lower[i]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  int e;
  ehvi_cells_forget(h);  // (bogp_point_eval_ehvi keeps a host copy of what it left in this buffer)
  if ((e = h->dehvi_cells.ensure(h, 2 * nb))) return e;
  // (the cells are the kernel's arguments: copied in stream order, before the first chunk's kernels that read them)
  HIPCHK(h, hipMemcpyAsync(h->dehvi_cells, lower, nb * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(h->dehvi_cells + nb, upper, nb * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));  // the caller's arrays are not needed past this call
  EhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.gamma = h->dgamma_base; ea.ld_gamma = h->Np; ea.N = h->N; ea.m = m; ea.C = C;
  for (int t = 0; t < m; ++t) ea.sigma2[t] = h->sigma2_t[t];
  ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + nb;
  invalidate_sweep_results(h);  // dbest_* are overwritten and hold no single-target winners afterwards
  const bool want_out = mu_out || mse_out;
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  SweepRequest rq;
  rq.want_out = want_out; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0; rq.eh = &ea;
  int rc = run_sweep(h, rq);
  if (rc) return rc;
  const int64_t M = h->M;
  if (k == 1) {  // the chunk loop's own argmax
    HIPCHK(h, hipMemcpy(best_val, h->dbest_val, sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(best_idx, h->dbest_idx, sizeof(int64_t), hipMemcpyDeviceToHost));
  } else {  // ranks 0 .. k-1 over the stored values, as bogp_sweep_topk ranks one criterion
    const int64_t nblk = (M + 255) / 256;
    if ((e = h->dblk_val.ensure(h, (size_t)(nblk + 1)))) return e;
    if ((e = h->dblk_idx.ensure(h, (size_t)(nblk + 1)))) return e;
    if ((e = h->dtopk_val.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return e;
    if ((e = h->dtopk_idx.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return e;
    HIPCHK(h, launch_topk(h->dacq_out, M, 1, k, h->dblk_val, h->dblk_idx, h->dtopk_val, h->dtopk_idx, st));
    HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
  }
  for (int i = 0; i < k; ++i)
    if (best_idx[i] == INT64_MAX) {  // fewer candidates than k: pad with (-inf, -1)
      best_val[i] = -INFINITY;
      best_idx[i] = -1;
    }
  if (ehvi_out) HIPCHK(h, hipMemcpy(ehvi_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  if (mu_out) HIPCHK(h, hipMemcpy(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost));
  if (mse_out) HIPCHK(h, hipMemcpy(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}
