// bogp_api_thompson.hip -- the C ABI of libbogp.so (include/bogp.h) for Thompson-sampling batches: bogp_sweep_thompson, q sample paths
// of the committed surrogate over the current candidates, each with its k best rows.  The reference declares
// GaussianProcess.sampling_prior / sampling_posterior and leaves both as `pass` (gpr.py:312-316); the paths here have the mean and
// MSE of its predictor (gpr.py:486-510) by pathwise conditioning on a random-Fourier-feature draw that the HOST supplies.
//   1  s = z(X) + sqrt(sigma2 (diag(R) - 1)) E      k_thompson's feature part over the N training rows (mode 0)
//   2  A = V^T (V s) = R^-1 s                       the kernels of believed_solve, N x q; with w = R^-1 1 (the committed L^-T Ft)
//      b_j = w . s_j / sum(w) (ordinary kriging, else 0), g_j = A_j - b_j w -- N q numbers, on the host
//   3  per candidate chunk: the producer with its store, then k_thompson (kernels_thompson.hip)
//   4  the argmax / top-k tail of bogp_sweep_topk
// No contraction launch anywhere.
// bogp_sweep_thompson_constrained (below): q members' joint paths of the m targets of a multi-target model -- the same four steps over
// q m columns, k_thompson_constrained in step 3 and 2 q scores in step 4.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

namespace {

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// the candidate rows of n ranked slots into best_x (n x d); a slot without a row (fewer candidates than ranks) is a NaN row
int fetch_rows(bogp_handle* h, const int64_t* best_idx, int n, double* best_x, hipStream_t st) {
  const int d = h->d;
  for (int i = 0; i < n; ++i) {
    double* dst = best_x + (size_t)i * d;
    if (best_idx[i] < 0 || best_idx[i] >= h->M) {
      for (int t = 0; t < d; ++t) dst[t] = NAN;
      continue;
    }
    HIPCHK(h, hipMemcpyAsync(dst, h->dXs + (size_t)best_idx[i] * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  return BOGP_OK;
}

}  // namespace

extern "C" int bogp_sweep_thompson(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                                   const double* eps, int conditioned, int minimize, int k, double* best_val, int64_t* best_idx,
                                   double* best_x, double* paths_out, double* coef_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_thompson";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior paths to draw", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (q < 1 || q > BOGP_MAX_PATHS) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d outside [1, %d]", who, q, BOGP_MAX_PATHS);
  if (L < 16 || L > BOGP_MAX_FEATURES || L % 16 != 0)
    FAIL(h, BOGP_ERR_INVALID, "%s: L = %d: a multiple of 16 in [16, %d] is required", who, L, BOGP_MAX_FEATURES);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!omega || !phase || !weights || !best_val || !best_idx)
    FAIL(h, BOGP_ERR_INVALID, "%s: omega, phase, weights, best_val and best_idx must be non-null", who);
  const int d = h->d, N = h->N, Np = h->Np;
  if (!all_finite(omega, (size_t)L * d)) FAIL(h, BOGP_ERR_INVALID, "%s: omega has a non-finite entry", who);
  if (!all_finite(phase, (size_t)L)) FAIL(h, BOGP_ERR_INVALID, "%s: phase has a non-finite entry", who);
  if (!all_finite(weights, (size_t)L * q)) FAIL(h, BOGP_ERR_INVALID, "%s: weights has a non-finite entry", who);
  if (eps && !all_finite(eps, (size_t)N * q)) FAIL(h, BOGP_ERR_INVALID, "%s: eps has a non-finite entry", who);
  if (h->mode != BOGP_MODE_NOISELESS)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: %s mode: the reference pairs an unscaled r(x) with a rescaled R there (gpr.py:949-979), which is no Gaussian process's conditional law",
         who, h->mode == BOGP_MODE_NOISY ? "noisy" : "noise-estimating");
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  if (h->n_t != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: one target only (the committed model has %d)", who, h->n_t);
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: no spectral draw is defined for the %s kernel", who, h->kernel == BOGP_KERNEL_CUBIC ? "cubic" : "generalized-exponential");
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  int rc;
  if ((rc = candidates_ready(h))) return rc;
  invalidate_sweep_results(h);  // dacq_out and the records are overwritten
  const int64_t M = h->M;
  const int N4 = (N + 3) & ~3;

  // ---- geometry: the sweep's own for a constant-trend model; one block record per 64 rows
  SweepGeometry geo;
  if ((rc = sweep_geometry(h, Np, &geo))) return rc;
  const int64_t Mc = geo.Mc, nchunk = geo.nchunk, nblk_total = (M + 63) / 64 + nchunk, nblk256 = (M + 255) / 256;
  const int S = geo.S;
  const bool store = k > 1 || paths_out != nullptr;

  // dth_small: omega (L d) | phase (L) | W (16 L) | -g (16 N4) | s (N q) | V s (N q) | R^-1 s (N q)
  const size_t n_small = (size_t)L * d + L + (size_t)16 * L + (size_t)16 * N4 + (size_t)3 * N * q;
  if ((rc = h->dth_small.ensure(h, n_small))) return rc;
  double* domega = h->dth_small;
  double* dphase = domega + (size_t)L * d;
  double* dW = dphase + L;
  double* dng = dW + (size_t)16 * L;
  double* ds = dng + (size_t)16 * N4;
  double* dvs = ds + (size_t)N * q;
  double* da = dvs + (size_t)N * q;
  if (conditioned) {
    if ((rc = h->drT[0].ensure(h, (size_t)Np * Mc))) return rc;
    if ((rc = h->dmu_part[0].ensure(h, (size_t)S * Mc))) return rc;
    if ((rc = h->dw_part[0].ensure(h, (size_t)S * Mc))) return rc;
  }
  if ((rc = h->dblk_val.ensure(h, (size_t)q * std::max(nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dblk_idx.ensure(h, (size_t)q * std::max(nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dtopk_val.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return rc;
  if ((rc = h->dtopk_idx.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return rc;
  if (store)
    if ((rc = h->dacq_out.ensure(h, (size_t)q * M))) return rc;

  // ---- the draw: W scaled by sqrt(2 sigma2 / L) and padded to 16 columns
  const double scale = std::sqrt(2.0 * h->sigma2 / (double)L);
  std::vector<double> hW((size_t)16 * L, 0.0);
  for (int l = 0; l < L; ++l)
    for (int j = 0; j < q; ++j) hW[(size_t)l * 16 + j] = scale * weights[(size_t)l * q + j];
  HIPCHK(h, hipMemcpyAsync(domega, omega, (size_t)L * d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(dphase, phase, (size_t)L * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(dW, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, st));

  ThompsonArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.d = d; ta.L = L; ta.N = N; ta.q = q; ta.omega = domega; ta.phase = dphase; ta.W = dW;

  enum { TH_SOLVE, TH_PRODUCER, TH_PATHS };  // kinds of the spans on h->th_timer
  SpanTimer& tm = h->th_timer;
  tm.begin();
  int s0 = 0, s1 = 0;
  if ((rc = tm.mark(h, st, &s0))) return rc;
  std::vector<double> hb(16, 0.0), hg((size_t)N * q, 0.0);
  if (conditioned) {
    // ---- 1: the draw at the training rows, plus what the nugget adds to an observation
    ta.X = h->dX; ta.row0 = 0; ta.mcount = N; ta.mode = 0; ta.minimize = 0; ta.vals = ds; ta.M = N;
    HIPCHK(h, launch_thompson(ta, st));
    std::vector<double> hs((size_t)N * q), ha((size_t)N * q), hw((size_t)N);
    HIPCHK(h, hipMemcpyAsync(hs.data(), ds, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hw.data(), h->dw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    const double nug = h->sigma2 * (h->R_diag - 1.0);
    if (eps && nug > 0.0) {
      const double sn = std::sqrt(nug);
      for (int j = 0; j < q; ++j)
        for (int n = 0; n < N; ++n) hs[(size_t)j * N + n] += sn * eps[(size_t)n * q + j];
      HIPCHK(h, hipMemcpyAsync(ds, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, st));
    }
    // ---- 2: R^-1 s for the q columns, then b and g on the host
    HIPCHK(h, launch_gemm(0, 0, N, q, N, 1.0, h->dV, h->ldr, ds, N, 0.0, dvs, N, st, 1));   // V s
    HIPCHK(h, launch_gemm(1, 0, N, q, N, 1.0, h->dV, h->ldr, dvs, N, 0.0, da, N, st, 2));   // V^T (V s)
    HIPCHK(h, hipMemcpyAsync(ha.data(), da, ha.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    double wsum = 0.0;
    for (int n = 0; n < N; ++n) wsum += hw[n];  // 1^T R^-1 1
    std::vector<double> hng((size_t)16 * N4, 0.0);
    for (int j = 0; j < q; ++j) {
      double ws = 0.0;
      for (int n = 0; n < N; ++n) ws += hw[n] * hs[(size_t)j * N + n];
      hb[j] = h->estimate_trend ? ws / wsum : 0.0;
      for (int n = 0; n < N; ++n) {
        const double g = h->estimate_trend ? ha[(size_t)j * N + n] - hb[j] * hw[n] : ha[(size_t)j * N + n];
        hg[(size_t)n * q + j] = g;
        hng[(size_t)n * 16 + j] = -1 * g;
      }
    }
    HIPCHK(h, hipMemcpyAsync(dng, hng.data(), hng.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));  // (hng leaves scope)
  }
  if ((rc = tm.mark(h, st, &s1))) return rc;
  tm.span(TH_SOLVE, s0, s1);
  if (coef_out) {
    memcpy(coef_out, hg.data(), (size_t)N * q * sizeof(double));
    for (int j = 0; j < q; ++j) coef_out[(size_t)N * q + j] = hb[j];
  }

  // ---- 3: the candidate chunks
  ta.X = h->dXs; ta.mode = conditioned ? 2 : 1; ta.minimize = minimize ? 1 : 0; ta.vals = store ? h->dacq_out : nullptr; ta.M = M;
  ta.rT = h->drT[0]; ta.ld = Mc; ta.ngt = dng; ta.mu_part = h->dmu_part[0]; ta.S = S; ta.beta = h->beta;
  for (int j = 0; j < 16; ++j) ta.bt[j] = hb[j];
  ta.blk_val = h->dblk_val; ta.blk_idx = h->dblk_idx; ta.nblk_total = nblk_total;
  int64_t blk_offset = 0;
  for (int64_t c = 0; c < nchunk; ++c) {
    const int64_t m0 = c * Mc, mcount = std::min<int64_t>(Mc, M - m0), Mc_eff = ((mcount + 63) / 64) * 64;
    int c0 = 0, c1 = 0, c2 = 0;
    if ((rc = tm.mark(h, st, &c0))) return rc;
    if (conditioned) HIPCHK(h, launch_corr_chunk(h->kernel, corr_chunk_args(h, geo, m0, 0), (int)(Mc_eff / 64), S, st));
    if ((rc = tm.mark(h, st, &c1))) return rc;
    ta.row0 = m0; ta.mcount = mcount; ta.blk_offset = blk_offset;
    HIPCHK(h, launch_thompson(ta, st));
    if ((rc = tm.mark(h, st, &c2))) return rc;
    tm.span(TH_PRODUCER, c0, c1); tm.span(TH_PATHS, c1, c2);
    blk_offset += (mcount + 63) / 64;
  }

  // ---- 4: the winners.  Rank 0 alone is the reduction of the kernel's records; k ranks are bogp_sweep_topk's passes over the stored values
  if (k == 1)
    HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, blk_offset, nblk_total, q, h->dtopk_val, h->dtopk_idx, st));
  else if ((rc = rank_stored_values(h, h->dacq_out, M, q, k, st)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)q * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)q * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (paths_out) HIPCHK(h, hipMemcpyAsync(paths_out, h->dacq_out, (size_t)q * M * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  if (paths_out && minimize)  // stored in the criterion's sign: back to the path's own
    for (size_t i = 0; i < (size_t)q * M; ++i) paths_out[i] = -1 * paths_out[i];
  pad_short_ranks(best_val, best_idx, q * k);
  if (best_x && (rc = fetch_rows(h, best_idx, q * k, best_x, st))) return rc;

  h->th_solve_ms = tm.sum(TH_SOLVE); h->th_corr_ms = tm.sum(TH_PRODUCER); h->th_paths_ms = tm.sum(TH_PATHS);
  h->th_chunks = (int)nchunk;
  return BOGP_OK;
}

extern "C" int bogp_thompson_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks) {
  if (!h) return BOGP_ERR_INVALID;
  if (corr_ms) *corr_ms = h->th_corr_ms;
  if (solve_ms) *solve_ms = h->th_solve_ms;
  if (paths_ms) *paths_ms = h->th_paths_ms;
  if (n_chunks) *n_chunks = h->th_chunks;
  return BOGP_OK;
}

// ---- Thompson batches under modelled constraints -------------------------------------------------------------------------------------
// q batch members' JOINT paths of the m = 1 + n_con targets of a multi-target model (target 0 the objective, target t >= 1 a constraint):
// q m <= 16 columns over shared features.  The model's targets share R and are a priori independent, and its trend is a fixed constant,
// so column (j, t) is the plain simple-kriging path
//   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x),      g_{j,t} = R^-1 (z_{j,t}(X) + sqrt(sigma2_t (diag R - 1)) E[:, (j,t)])
//   1  the draw at the training rows: k_thompson in mode 0 over the q m columns, W scaled per column by sqrt(2 sigma2_t / L)
//   2  R^-1 s by the two gemms above; gamma_t from dgamma_base; gamma_t - g on the host
//   3  per candidate chunk: the producer with its store, then k_thompson_constrained (kernels_thompson_constrained.hip)
//   4  the argmax / top-k tail over the 2 q scores (A_j: the objective where the drawn constraints hold; B_j: minus the violation)
// ABI column j m + t, DEVICE column t q + j (the kernel's gather).
extern "C" int bogp_sweep_thompson_constrained(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                                               const double* eps, int minimize, int n_con, const double* lo, const double* hi, int k,
                                               double* best_val, int64_t* best_idx, double* best_x, double* paths_out, double* coef_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_thompson_constrained";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior paths to draw", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  const int m = h->n_t;
  if (m < 2) FAIL(h, BOGP_ERR_INVALID, "%s: the committed model has one target and so no modelled constraint: bogp_sweep_thompson serves it", who);
  if (n_con != m - 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d, but the committed model has %d targets (one objective and %d constraints)", who, n_con, m, m - 1);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  if (q < 1 || q * m > BOGP_MAX_PATHS) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d members of %d targets: 1 <= q and q m <= %d columns", who, q, m, BOGP_MAX_PATHS);
  if (L < 16 || L > BOGP_MAX_FEATURES || L % 16 != 0)
    FAIL(h, BOGP_ERR_INVALID, "%s: L = %d: a multiple of 16 in [16, %d] is required", who, L, BOGP_MAX_FEATURES);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  if (!omega || !phase || !weights || !lo || !hi || !best_val || !best_idx)
    FAIL(h, BOGP_ERR_INVALID, "%s: omega, phase, weights, lo, hi, best_val and best_idx must be non-null", who);
  int rc;
  if ((rc = check_constraint_bounds(h, who, n_con, lo, hi))) return rc;
  const int d = h->d, N = h->N, Np = h->Np, qm = q * m;
  if (!all_finite(omega, (size_t)L * d)) FAIL(h, BOGP_ERR_INVALID, "%s: omega has a non-finite entry", who);
  if (!all_finite(phase, (size_t)L)) FAIL(h, BOGP_ERR_INVALID, "%s: phase has a non-finite entry", who);
  if (!all_finite(weights, (size_t)L * qm)) FAIL(h, BOGP_ERR_INVALID, "%s: weights has a non-finite entry", who);
  if (eps && !all_finite(eps, (size_t)N * qm)) FAIL(h, BOGP_ERR_INVALID, "%s: eps has a non-finite entry", who);
  if (h->mode != BOGP_MODE_NOISELESS)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: %s mode: the reference pairs an unscaled r(x) with a rescaled R there (gpr.py:949-979), which is no Gaussian process's conditional law",
         who, h->mode == BOGP_MODE_NOISY ? "noisy" : "noise-estimating");
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: no spectral draw is defined for the %s kernel", who, h->kernel == BOGP_KERNEL_CUBIC ? "cubic" : "generalized-exponential");
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  if ((rc = candidates_ready(h))) return rc;
  invalidate_sweep_results(h);  // dacq_out and the records are overwritten
  const int64_t M = h->M;
  const int N4 = (N + 3) & ~3;
  const auto dcol = [&](int j, int t) { return t * q + j; };  // the device column of ABI column j m + t

  SweepGeometry geo;
  if ((rc = sweep_geometry(h, Np, &geo))) return rc;
  const int64_t Mc = geo.Mc, nchunk = geo.nchunk, nblk_total = (M + 63) / 64 + nchunk, nblk256 = (M + 255) / 256;
  const int S = geo.S;
  const bool ranked = k > 1;

  // dth_small: omega (L d) | phase (L) | W (16 L) | gamma - g (16 N4) | s (N qm) | V s (N qm) | R^-1 s (N qm)
  const size_t n_small = (size_t)L * d + L + (size_t)16 * L + (size_t)16 * N4 + (size_t)3 * N * qm;
  if ((rc = h->dth_small.ensure(h, n_small))) return rc;
  double* domega = h->dth_small;
  double* dphase = domega + (size_t)L * d;
  double* dW = dphase + L;
  double* dcoef = dW + (size_t)16 * L;
  double* ds = dcoef + (size_t)16 * N4;
  double* dvs = ds + (size_t)N * qm;
  double* da = dvs + (size_t)N * qm;
  if ((rc = h->drT[0].ensure(h, (size_t)Np * Mc))) return rc;
  if ((rc = h->dmu_part[0].ensure(h, (size_t)S * Mc))) return rc;
  if ((rc = h->dw_part[0].ensure(h, (size_t)S * Mc))) return rc;
  if ((rc = h->dblk_val.ensure(h, (size_t)2 * q * std::max(nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dblk_idx.ensure(h, (size_t)2 * q * std::max(nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dtopk_val.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return rc;
  if ((rc = h->dtopk_idx.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return rc;
  // dacq_out: the [2 q][M] scores (k > 1), then the [q m][M] path values (on request)
  const size_t n_scores = ranked ? (size_t)2 * q * M : 0, n_paths = paths_out ? (size_t)qm * M : 0;
  if (n_scores + n_paths > 0)
    if ((rc = h->dacq_out.ensure(h, n_scores + n_paths))) return rc;

  // ---- the draw: W scaled per column by sqrt(2 sigma2_t / L), permuted to the device's columns and padded to 16
  std::vector<double> hW((size_t)16 * L, 0.0);
  for (int t = 0; t < m; ++t) {
    const double scale = std::sqrt(2.0 * h->sigma2_t[t] / (double)L);
    for (int l = 0; l < L; ++l)
      for (int j = 0; j < q; ++j) hW[(size_t)l * 16 + dcol(j, t)] = scale * weights[(size_t)l * qm + j * m + t];
  }
  HIPCHK(h, hipMemcpyAsync(domega, omega, (size_t)L * d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(dphase, phase, (size_t)L * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(dW, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, st));

  enum { TH_SOLVE, TH_PRODUCER, TH_PATHS };  // kinds of the spans on h->th_timer
  SpanTimer& tm = h->th_timer;
  tm.begin();
  int s0 = 0, s1 = 0;
  if ((rc = tm.mark(h, st, &s0))) return rc;
  // ---- 1: the draw at the training rows (device columns), plus what the nugget adds to an observation
  ThompsonArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.d = d; ta.L = L; ta.N = N; ta.q = qm; ta.omega = domega; ta.phase = dphase; ta.W = dW;
  ta.X = h->dX; ta.row0 = 0; ta.mcount = N; ta.mode = 0; ta.minimize = 0; ta.vals = ds; ta.M = N;
  HIPCHK(h, launch_thompson(ta, st));
  std::vector<double> hs((size_t)N * qm), ha((size_t)N * qm), hgamma((size_t)m * Np);
  HIPCHK(h, hipMemcpyAsync(hgamma.data(), h->dgamma_base.ptr, hgamma.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (eps && h->R_diag - 1.0 > 0.0) {
    HIPCHK(h, hipMemcpyAsync(hs.data(), ds, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    for (int t = 0; t < m; ++t) {
      const double sn = std::sqrt(h->sigma2_t[t] * (h->R_diag - 1.0));
      for (int j = 0; j < q; ++j)
        for (int n = 0; n < N; ++n) hs[(size_t)dcol(j, t) * N + n] += sn * eps[(size_t)n * qm + j * m + t];
    }
    HIPCHK(h, hipMemcpyAsync(ds, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  // ---- 2: R^-1 s for the q m columns, then gamma_t - g on the host
  HIPCHK(h, launch_gemm(0, 0, N, qm, N, 1.0, h->dV, h->ldr, ds, N, 0.0, dvs, N, st, 1));   // V s
  HIPCHK(h, launch_gemm(1, 0, N, qm, N, 1.0, h->dV, h->ldr, dvs, N, 0.0, da, N, st, 2));   // V^T (V s)
  HIPCHK(h, hipMemcpyAsync(ha.data(), da, ha.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  std::vector<double> hcoef((size_t)16 * N4, 0.0);
  for (int t = 0; t < m; ++t)
    for (int j = 0; j < q; ++j) {
      const int c = dcol(j, t);
      for (int n = 0; n < N; ++n) {
        const double g = ha[(size_t)c * N + n];
        hcoef[(size_t)n * 16 + c] = hgamma[(size_t)t * Np + n] - g;
        if (coef_out) coef_out[(size_t)n * qm + j * m + t] = g;
      }
    }
  HIPCHK(h, hipMemcpyAsync(dcoef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));  // (hcoef leaves scope)
  if ((rc = tm.mark(h, st, &s1))) return rc;
  tm.span(TH_SOLVE, s0, s1);

  // ---- 3: the candidate chunks
  ThompsonConstrainedArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.X = h->dXs; ca.d = d; ca.L = L; ca.N = N; ca.q = q; ca.m = m; ca.omega = domega; ca.phase = dphase; ca.W = dW;
  ca.rT = h->drT[0]; ca.ld = Mc; ca.coef = dcoef; ca.beta = h->beta; ca.minimize = minimize ? 1 : 0; ca.M = M;
  for (int t = 1; t < m; ++t) {
    ca.lo[t] = lo[t - 1]; ca.hi[t] = hi[t - 1];
    ca.inv_sd[t] = 1.0 / std::sqrt(h->sigma2_t[t]);
  }
  double* dscores = ranked ? h->dacq_out.ptr : nullptr;
  double* dpaths = paths_out ? h->dacq_out.ptr + n_scores : nullptr;
  ca.scores = dscores; ca.paths = dpaths;
  ca.blk_val = h->dblk_val; ca.blk_idx = h->dblk_idx; ca.nblk_total = nblk_total;
  int64_t blk_offset = 0;
  for (int64_t c = 0; c < nchunk; ++c) {
    const int64_t m0 = c * Mc, mcount = std::min<int64_t>(Mc, M - m0), Mc_eff = ((mcount + 63) / 64) * 64;
    int c0 = 0, c1 = 0, c2 = 0;
    if ((rc = tm.mark(h, st, &c0))) return rc;
    HIPCHK(h, launch_corr_chunk(h->kernel, corr_chunk_args(h, geo, m0, 0), (int)(Mc_eff / 64), S, st));
    if ((rc = tm.mark(h, st, &c1))) return rc;
    ca.row0 = m0; ca.mcount = mcount; ca.blk_offset = blk_offset;
    HIPCHK(h, launch_thompson_constrained(ca, st));
    if ((rc = tm.mark(h, st, &c2))) return rc;
    tm.span(TH_PRODUCER, c0, c1); tm.span(TH_PATHS, c1, c2);
    blk_offset += (mcount + 63) / 64;
  }

  // ---- 4: the winners of the 2 q scores: [q][2][k], member j's A ranks, then its B ranks
  const int nq = 2 * q;
  if (k == 1)
    HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, blk_offset, nblk_total, nq, h->dtopk_val, h->dtopk_idx, st));
  else if ((rc = rank_stored_values(h, dscores, M, nq, k, st)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (paths_out) HIPCHK(h, hipMemcpyAsync(paths_out, dpaths, (size_t)qm * M * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  pad_short_ranks(best_val, best_idx, nq * k);
  if (best_x && (rc = fetch_rows(h, best_idx, nq * k, best_x, st))) return rc;

  h->thc_solve_ms = tm.sum(TH_SOLVE); h->thc_corr_ms = tm.sum(TH_PRODUCER); h->thc_paths_ms = tm.sum(TH_PATHS);
  h->thc_chunks = (int)nchunk;
  return BOGP_OK;
}

extern "C" int bogp_thompson_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks) {
  if (!h) return BOGP_ERR_INVALID;
  if (corr_ms) *corr_ms = h->thc_corr_ms;
  if (solve_ms) *solve_ms = h->thc_solve_ms;
  if (paths_ms) *paths_ms = h->thc_paths_ms;
  if (n_chunks) *n_chunks = h->thc_chunks;
  return BOGP_OK;
}
