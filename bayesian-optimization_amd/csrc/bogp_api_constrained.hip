// bogp_api_constrained.hip -- the C ABI of libbogp.so (include/bogp.h) for modelled constraints: bogp_sweep_constrained, q
// feasibility-weighted criteria of an m-target model (target 0 the objective, targets 1 .. m - 1 the constraints) over the current
// candidates, and bogp_feasibility / bogp_feasibility_grad, the factor one constraint contributes and its derivatives, on the host.  The sweep is the chunked sweep of
// bogp_api_sweep.hip (producer -> contraction per chunk) with k_constrained (kernels_constrained.hip) in place of k_acquisition.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/bogp.h"
#include "bogp_device.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

extern "C" double bogp_feasibility(double mu, double mse, double sigma2, double lo, double hi) { return feasibility(mu, mse, sigma2, lo, hi); }

extern "C" int bogp_feasibility_grad(double mu, double mse, double sigma2, double lo, double hi, double* out3) {
  if (!out3) return BOGP_ERR_INVALID;
  feasibility_grad(mu, mse, sigma2, lo, hi, &out3[0], &out3[1], &out3[2]);
  return BOGP_OK;
}

int bogp::check_constrained_request(bogp_handle* h, const char* who, int q, const int* acq_id, const double* acq_par, int n_con,
                                    const double* lo, const double* hi) {
  const int m = h->n_t;
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "%s: the committed model has %d target(s); an objective and its constraints need 2 .. %d", who, m, BOGP_MAX_TARGETS);
  if (n_con != m - 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d but the committed model has %d targets (one objective, %d constraints)", who, n_con, m, m - 1);
  if (q < 1 || q > BOGP_MAX_Q) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d outside [1, %d]", who, q, BOGP_MAX_Q);
  if (!acq_id || !lo || !hi) FAIL(h, BOGP_ERR_INVALID, "%s: acq_id, lo and hi must be non-null", who);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  for (int c = 0; c < q; ++c) {
    const int id = acq_id[c];
    if (id == BOGP_ACQ_UCB) FAIL(h, BOGP_ERR_INVALID, "%s: criterion %d is UCB, which changes sign: its product with a probability orders nothing (EI, EpsilonPI, MGFI or BOGP_ACQ_NONE)", who, c);
    if (id != BOGP_ACQ_EI && id != BOGP_ACQ_EPSILON_PI && id != BOGP_ACQ_MGFI && id != BOGP_ACQ_NONE) FAIL(h, BOGP_ERR_INVALID, "%s: unknown acquisition id %d", who, id);
    if (id == BOGP_ACQ_EPSILON_PI && (!acq_par || !(acq_par[c] >= 0))) FAIL(h, BOGP_ERR_INVALID, "%s: acquisition parameter %d must be >= 0 (epsilon = 0 is plain PI)", who, c);
    if (id == BOGP_ACQ_MGFI && (!acq_par || !(acq_par[c] > 0))) FAIL(h, BOGP_ERR_INVALID, "%s: acquisition parameter %d must be > 0 (the reference asserts t > 0)", who, c);
  }
  return check_constraint_bounds(h, who, n_con, lo, hi);
}

int bogp::check_constraint_bounds(bogp_handle* h, const char* who, int n_con, const double* lo, const double* hi) {
  for (int j = 0; j < n_con; ++j) {
    if (std::isnan(lo[j]) || std::isnan(hi[j])) FAIL(h, BOGP_ERR_INVALID, "%s: a bound of constraint %d is NaN", who, j);
    if (hi[j] < lo[j]) FAIL(h, BOGP_ERR_INVALID, "%s: the upper bound of constraint %d (%g) is below its lower bound (%g)", who, j, hi[j], lo[j]);
  }
  return BOGP_OK;
}

extern "C" int bogp_sweep_constrained(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize, int n_con,
                                      const double* lo, const double* hi, int k, double* best_val, int64_t* best_idx, double* acq_out,
                                      double* pof_out, double* mu_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_constrained";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest; modelled constraints take a multi-target Gaussian process", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set) and modelled constraints have no lifted sweep: call bogp_lift_clear first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: several targets take the constant trend only (gpr.py:787)", who);
  // (every check from here on returns BOGP_ERR_INVALID: the sweep's own two stand before the shared ones, which name three pointers only)
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!acq_id || !lo || !hi || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: acq_id, lo, hi, best_val and best_idx must be non-null", who);
  int e = check_constrained_request(h, who, q, acq_id, acq_par, n_con, lo, hi);
  if (e) return e;
  const int m = h->n_t;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  if (pof_out && (e = h->dpof_out.ensure(h, (size_t)M))) return e;
  ConstrainedArgs ca;
  memset(&ca, 0, sizeof(ca));
  multi_target_model(h, ca);
  for (int j = 0; j < n_con; ++j) { ca.lo[j + 1] = lo[j]; ca.hi[j + 1] = hi[j]; }
  ca.q = q;
  for (int c = 0; c < q; ++c) { ca.acq_id[c] = acq_id[c]; ca.acq_par[c] = acq_par ? acq_par[c] : 0.0; }
  ca.plugin = plugin; ca.minimize = minimize; ca.pof_out = pof_out ? h->dpof_out.ptr : nullptr;
  invalidate_sweep_results(h);  // dbest_* are overwritten and hold no single-target winners afterwards
  SweepRequest rq;  // (q sizes the chunk loop's block records and dacq_out; the criteria themselves travel in ca)
  rq.want_out = mu_out || mse_out; rq.want_acq_out = true; rq.q = q; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin;
  rq.minimize = minimize; rq.cn = &ca;
  int rc = run_sweep(h, rq);
  if (rc) return rc;
  // (the downloads are queued in front of the winners: fetch_winners waits for the stream)
  if (acq_out) HIPCHK(h, hipMemcpyAsync(acq_out, h->dacq_out, (size_t)q * M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (pof_out) HIPCHK(h, hipMemcpyAsync(pof_out, h->dpof_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mu_out) HIPCHK(h, hipMemcpyAsync(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  return fetch_winners(h, q, k, h->dacq_out, best_val, best_idx, st);
}
