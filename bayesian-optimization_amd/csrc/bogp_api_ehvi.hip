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
  int e;
  if ((e = check_ehvi_cells(h, "bogp_sweep_ehvi", nb, lower, upper))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  if ((e = stage_ehvi_cells(h, lower, upper, nb, st))) return e;
  EhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  multi_target_model(h, ea);
  ea.C = C; ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + nb;
  invalidate_sweep_results(h);  // dbest_* are overwritten and hold no single-target winners afterwards
  const bool want_out = mu_out || mse_out;
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  SweepRequest rq;
  rq.want_out = want_out; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0; rq.eh = &ea;
  int rc = run_sweep(h, rq);
  if (rc) return rc;
  const int64_t M = h->M;
  // (the downloads are queued in front of the winners: fetch_winners waits for the stream)
  if (ehvi_out) HIPCHK(h, hipMemcpyAsync(ehvi_out, h->dacq_out, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mu_out) HIPCHK(h, hipMemcpyAsync(mu_out, h->dmu_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToHost, st));
  return fetch_winners(h, 1, k, h->dacq_out, best_val, best_idx, st);
}
