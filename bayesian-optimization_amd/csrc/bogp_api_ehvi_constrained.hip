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
  int e;
  if ((e = check_ehvi_cells(h, who, nb, lower, upper))) return e;
  if ((e = check_constraint_bounds(h, who, n_con, lo, hi))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  if ((e = stage_ehvi_cells(h, lower, upper, nb, st))) return e;
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
  // (the downloads are queued in front of the winners: fetch_winners waits for the stream)
  if (val_out) HIPCHK(h, hipMemcpyAsync(val_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (pof_out) HIPCHK(h, hipMemcpyAsync(pof_out, h->dpof_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mu_out) HIPCHK(h, hipMemcpyAsync(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  return fetch_winners(h, 1, k, h->dacq_out, best_val, best_idx, st);
}
