// bogp_api_ehvi_constrained.hip -- the C ABI of libbogp.so (include/bogp.h) for modelled constraints of a multi-objective run:
// bogp_sweep_ehvi_constrained, the expected hypervolume improvement of the first m_obj targets of an m-target model weighted by the
// probability that the remaining n_con targets are feasible, over the current candidates.  It runs the chunked sweep of
// bogp_api_sweep.hip (producer -> contraction per chunk) with k_ehvi_constrained (kernels_ehvi_constrained.hip) in place of k_acquisition.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

extern "C" int bogp_sweep_ehvi_constrained(bogp_handle* h, int m_obj, int C, const double* lower, const double* upper, int n_con, const double* lo,
                                           const double* hi, int k, double* best_val, int64_t* best_idx, double* val_out, double* pof_out,
                                           double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_ehvi_constrained";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest; modelled constraints take a multi-target Gaussian process", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set) and constrained EHVI has no lifted sweep: call bogp_lift_clear first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: several targets take the constant trend only (gpr.py:787)", who);
  const int m = h->n_t;
  if (m_obj < 2) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj = %d objectives; EHVI needs at least 2", who, m_obj);
  if (n_con < 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d constraints; without one this is bogp_sweep_ehvi", who, n_con);
  if (m > BOGP_MAX_TARGETS || m_obj + n_con != m) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj + n_con = %d + %d but the committed model has %d targets (at most %d)", who, m_obj, n_con, m, BOGP_MAX_TARGETS);
  if (C < 0 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "%s: C = %d cells outside [0, %d]", who, C, BOGP_MAX_EHVI_CELLS);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if ((C > 0 && (!lower || !upper)) || !lo || !hi || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: lower and upper (C > 0), lo, hi, best_val and best_idx must be non-null", who);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  const size_t nb = (size_t)C * m_obj;
  for (size_t i = 0; i < nb; ++i) {
    if (!std::isfinite(lower[i])) FAIL(h, BOGP_ERR_INVALID, "%s: lower bound %zu is not finite", who, i);
    if (std::isnan(upper[i])) FAIL(h, BOGP_ERR_INVALID, "%s: upper bound %zu is NaN", who, i);
    if (!(upper[i] >= lower[i])) FAIL(h, BOGP_ERR_INVALID, "%s: upper bound %zu (%g) is below its lower bound (%g)", who, i, upper[i], lower[i]);
  }
  for (int j = 0; j < n_con; ++j) {
    if (std::isnan(lo[j]) || std::isnan(hi[j])) FAIL(h, BOGP_ERR_INVALID, "%s: a bound of constraint %d is NaN", who, j);
    if (hi[j] < lo[j]) FAIL(h, BOGP_ERR_INVALID, "%s: the upper bound of constraint %d (%g) is below its lower bound (%g)", who, j, hi[j], lo[j]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  int e;
  ehvi_cells_forget(h);  // (bogp_point_eval_ehvi keeps a host copy of what it left in this buffer)
  if (nb > 0) {
    if ((e = h->dehvi_cells.ensure(h, 2 * nb))) return e;
    // (the cells are the kernel's arguments: copied in stream order, before the first chunk's kernels that read them)
    HIPCHK(h, hipMemcpyAsync(h->dehvi_cells, lower, nb * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->dehvi_cells + nb, upper, nb * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));  // the caller's arrays are not needed past this call
  }
  if (pof_out && (e = h->dpof_out.ensure(h, (size_t)M))) return e;
  ConstrainedEhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.gamma = h->dgamma_base; ea.ld_gamma = h->Np; ea.N = h->N; ea.m = m; ea.m_obj = m_obj; ea.C = C;
  for (int t = 0; t < m; ++t) ea.sigma2[t] = h->sigma2_t[t];
  for (int j = 0; j < n_con; ++j) { ea.lo[j] = lo[j]; ea.hi[j] = hi[j]; }
  if (nb > 0) { ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + nb; }
  ea.pof_out = pof_out ? h->dpof_out.ptr : nullptr;
  invalidate_sweep_results(h);  // dbest_* are overwritten and hold no single-target winners afterwards
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  SweepRequest rq;
  rq.want_out = mu_out || mse_out; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0; rq.ec = &ea;
  int rc = run_sweep(h, rq);
  if (rc) return rc;
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
  if (val_out) HIPCHK(h, hipMemcpy(val_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  if (pof_out) HIPCHK(h, hipMemcpy(pof_out, h->dpof_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost));
  if (mu_out) HIPCHK(h, hipMemcpy(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost));
  if (mse_out) HIPCHK(h, hipMemcpy(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}
