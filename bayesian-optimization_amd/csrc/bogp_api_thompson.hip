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
// The steps are written once (begin_pass, upload_draw, solve_at_training_rows, for_each_chunk, winners); an entry keeps its refusals in
// its own order, the host arithmetic between the steps and its kernel's arguments.
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

enum { TH_SOLVE, TH_PRODUCER, TH_PATHS };  // kinds of the spans on h->th_timer

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// ---- the refusals both entries make, each called where the entry's own order has it
int check_ready(bogp_handle* h, const char* who) {
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior paths to draw", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  return BOGP_OK;
}
int check_features_and_ranks(bogp_handle* h, const char* who, int L, int k) {
  if (L < 16 || L > BOGP_MAX_FEATURES || L % 16 != 0)
    FAIL(h, BOGP_ERR_INVALID, "%s: L = %d: a multiple of 16 in [16, %d] is required", who, L, BOGP_MAX_FEATURES);
  if (k < 1 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "%s: k = %d outside [1, %d]", who, k, BOGP_MAX_TOPK);
  return BOGP_OK;
}
int check_draw_finite_and_mode(bogp_handle* h, const char* who, int L, int ncol, const double* omega, const double* phase,
                               const double* weights, const double* eps) {
  if (!all_finite(omega, (size_t)L * h->d)) FAIL(h, BOGP_ERR_INVALID, "%s: omega has a non-finite entry", who);
  if (!all_finite(phase, (size_t)L)) FAIL(h, BOGP_ERR_INVALID, "%s: phase has a non-finite entry", who);
  if (!all_finite(weights, (size_t)L * ncol)) FAIL(h, BOGP_ERR_INVALID, "%s: weights has a non-finite entry", who);
  if (eps && !all_finite(eps, (size_t)h->N * ncol)) FAIL(h, BOGP_ERR_INVALID, "%s: eps has a non-finite entry", who);
  if (h->mode != BOGP_MODE_NOISELESS)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: %s mode: the reference pairs an unscaled r(x) with a rescaled R there (gpr.py:949-979), which is no Gaussian process's conditional law",
         who, h->mode == BOGP_MODE_NOISY ? "noisy" : "noise-estimating");
  return BOGP_OK;
}
int refuse_trend(bogp_handle* h, const char* who) {
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  return BOGP_OK;
}
int refuse_lift(bogp_handle* h, const char* who) {
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  return BOGP_OK;
}
// the last refusals of both entries: the kernel, a lift (the constrained entry's order has that one further up, so it never fires there), the ranks
int refuse_kernel_lift_ranks(bogp_handle* h, const char* who) {
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: no spectral draw is defined for the %s kernel", who, h->kernel == BOGP_KERNEL_CUBIC ? "cubic" : "generalized-exponential");
  if (int rc = refuse_lift(h, who)) return rc;
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  return BOGP_OK;
}

// ---- the steps
// What a call over ncol columns (q, or q m) works in: the sweep's own chunk geometry for a constant-trend model, one block record per 64
// rows -- nblk of nblk_total written by the chunks -- the first mark of th_timer, and
// dth_small: omega (L d) | phase (L) | W (16 L) | coef (16 N4) | s (N ncol) | V s (N ncol) | R^-1 s (N ncol)
struct ThompsonPass { SweepGeometry geo; int64_t nblk, nblk_total; int s0; double *omega, *phase, *W, *coef, *s, *vs, *a; };

// the refusals are behind: the candidates finished, the geometry, and every buffer but dacq_out (nscore rows of block records)
int begin_pass(bogp_handle* h, int L, int ncol, int nscore, bool with_producer, ThompsonPass* P) {
  HIPCHK(h, hipSetDevice(h->device));
  int rc;
  if ((rc = candidates_ready(h))) return rc;
  invalidate_sweep_results(h);  // dacq_out and the records are overwritten
  if ((rc = sweep_geometry(h, h->Np, &P->geo))) return rc;
  const int64_t Mc = P->geo.Mc, nblk256 = (h->M + 255) / 256;
  const size_t d = h->d, N = h->N, N4 = (h->N + 3) & ~3;
  P->nblk = 0; P->nblk_total = (h->M + 63) / 64 + P->geo.nchunk;
  if ((rc = h->dth_small.ensure(h, L * d + L + (size_t)16 * L + 16 * N4 + 3 * N * ncol))) return rc;
  P->omega = h->dth_small; P->phase = P->omega + L * d; P->W = P->phase + L; P->coef = P->W + (size_t)16 * L;
  P->s = P->coef + 16 * N4; P->vs = P->s + N * ncol; P->a = P->vs + N * ncol;
  if (with_producer) {
    if ((rc = h->drT[0].ensure(h, (size_t)h->Np * Mc))) return rc;
    if ((rc = h->dmu_part[0].ensure(h, (size_t)P->geo.S * Mc))) return rc;
    if ((rc = h->dw_part[0].ensure(h, (size_t)P->geo.S * Mc))) return rc;
  }
  if ((rc = h->dblk_val.ensure(h, (size_t)nscore * std::max(P->nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dblk_idx.ensure(h, (size_t)nscore * std::max(P->nblk_total, nblk256 + 1)))) return rc;
  if ((rc = h->dtopk_val.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return rc;
  return h->dtopk_idx.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK);
}

// omega, phase and the entry's scaled weights hW ([L][16], device column order, zero padded); behind them the call's timing starts
int upload_draw(bogp_handle* h, ThompsonPass& P, int L, const double* omega, const double* phase, const std::vector<double>& hW, hipStream_t st) {
  HIPCHK(h, hipMemcpyAsync(P.omega, omega, (size_t)L * h->d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(P.phase, phase, (size_t)L * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(P.W, hW.data(), hW.size() * sizeof(double), hipMemcpyHostToDevice, st));
  h->th_timer.begin();
  return h->th_timer.mark(h, st, &P.s0);
}

struct ColNoise { double sd; int src; };  // what the nugget adds to a device column's observation: sd * eps[:, src]

// Steps 1 and 2 over ncol device columns: the draw at the training rows (k_thompson, mode 0), `noise` (one entry per column, or none)
// added on the host, and R^-1 s by the two gemms into ha, waited for.  hs is read back where `need_s` says so or there is noise; what
// the caller queued on st before (its own read of w or gamma) has arrived on return.
int solve_at_training_rows(bogp_handle* h, const ThompsonPass& P, int L, int ncol, bool need_s, const std::vector<ColNoise>& noise,
                           const double* eps, std::vector<double>& hs, std::vector<double>& ha, hipStream_t st) {
  const int N = h->N;
  ThompsonArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.d = h->d; ta.L = L; ta.N = N; ta.q = ncol; ta.omega = P.omega; ta.phase = P.phase; ta.W = P.W;
  ta.X = h->dX; ta.row0 = 0; ta.mcount = N; ta.mode = 0; ta.minimize = 0; ta.vals = P.s; ta.M = N;
  HIPCHK(h, launch_thompson(ta, st));
  if (need_s || !noise.empty()) {
    HIPCHK(h, hipMemcpyAsync(hs.data(), P.s, hs.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
  }
  if (!noise.empty()) {
    for (int c = 0; c < ncol; ++c)
      for (int n = 0; n < N; ++n) hs[(size_t)c * N + n] += noise[c].sd * eps[(size_t)n * ncol + noise[c].src];
    HIPCHK(h, hipMemcpyAsync(P.s, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  }
  HIPCHK(h, launch_gemm(0, 0, N, ncol, N, 1.0, h->dV, h->ldr, P.s, N, 0.0, P.vs, N, st, 1));   // V s
  HIPCHK(h, launch_gemm(1, 0, N, ncol, N, 1.0, h->dV, h->ldr, P.vs, N, 0.0, P.a, N, st, 2));   // V^T (V s)
  HIPCHK(h, hipMemcpyAsync(ha.data(), P.a, ha.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return BOGP_OK;
}

// Step 3: per chunk the producer (where the paths are conditioned) and the family's kernel -- `launch` on `a`, whose three per-chunk
// fields are set here -- between marks of th_timer.  P.nblk: the block records written.
template <class Args>
int for_each_chunk(bogp_handle* h, ThompsonPass& P, bool with_producer, hipStream_t st, Args& a, hipError_t (*launch)(const Args&, hipStream_t)) {
  SpanTimer& tm = h->th_timer;
  int rc;
  for (int64_t c = 0; c < P.geo.nchunk; ++c) {
    const int64_t m0 = c * P.geo.Mc, mcount = std::min<int64_t>(P.geo.Mc, h->M - m0), Mc_eff = ((mcount + 63) / 64) * 64;
    int c0 = 0, c1 = 0, c2 = 0;
    if ((rc = tm.mark(h, st, &c0))) return rc;
    if (with_producer) HIPCHK(h, launch_corr_chunk(h->kernel, corr_chunk_args(h, P.geo, m0, 0), (int)(Mc_eff / 64), P.geo.S, st));
    if ((rc = tm.mark(h, st, &c1))) return rc;
    a.row0 = m0; a.mcount = mcount; a.blk_offset = P.nblk;
    HIPCHK(h, launch(a, st));
    if ((rc = tm.mark(h, st, &c2))) return rc;
    tm.span(TH_PRODUCER, c0, c1); tm.span(TH_PATHS, c1, c2);
    P.nblk += (mcount + 63) / 64;
  }
  return BOGP_OK;
}

// Step 4: the winners of nscore score rows and their candidate rows.  Rank 0 alone is the reduction of the kernel's records; k ranks are
// bogp_sweep_topk's passes over the stored dscores.  Whatever the caller queued on st before (its paths_out copy) has arrived on return.
int winners(bogp_handle* h, const ThompsonPass& P, int nscore, int k, const double* dscores, double* best_val, int64_t* best_idx,
            double* best_x, hipStream_t st) {
  int rc;
  if (k == 1)
    HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, P.nblk, P.nblk_total, nscore, h->dtopk_val, h->dtopk_idx, st));
  else if ((rc = rank_stored_values(h, dscores, h->M, nscore, k, st)))
    return rc;
  HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)nscore * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)nscore * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  pad_short_ranks(best_val, best_idx, nscore * k);
  if (!best_x) return BOGP_OK;
  const int d = h->d;  // a slot without a row (fewer candidates than ranks) is a NaN row
  for (int i = 0; i < nscore * k; ++i) {
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

void store_last(SpanTimer& tm, int64_t nchunk, ThompsonLast* dst) {
  dst->solve_ms = tm.sum(TH_SOLVE); dst->corr_ms = tm.sum(TH_PRODUCER); dst->paths_ms = tm.sum(TH_PATHS);
  dst->chunks = (int)nchunk;
}

int read_last(const ThompsonLast& last, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks) {
  if (corr_ms) *corr_ms = last.corr_ms;
  if (solve_ms) *solve_ms = last.solve_ms;
  if (paths_ms) *paths_ms = last.paths_ms;
  if (n_chunks) *n_chunks = last.chunks;
  return BOGP_OK;
}

}  // namespace

extern "C" int bogp_sweep_thompson(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                                   const double* eps, int conditioned, int minimize, int k, double* best_val, int64_t* best_idx,
                                   double* best_x, double* paths_out, double* coef_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_thompson";
  int rc;
  if ((rc = check_ready(h, who))) return rc;
  if (q < 1 || q > BOGP_MAX_PATHS) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d outside [1, %d]", who, q, BOGP_MAX_PATHS);
  if ((rc = check_features_and_ranks(h, who, L, k))) return rc;
  if (!omega || !phase || !weights || !best_val || !best_idx)
    FAIL(h, BOGP_ERR_INVALID, "%s: omega, phase, weights, best_val and best_idx must be non-null", who);
  if ((rc = check_draw_finite_and_mode(h, who, L, q, omega, phase, weights, eps))) return rc;
  if ((rc = refuse_trend(h, who))) return rc;
  if (h->n_t != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: one target only (the committed model has %d)", who, h->n_t);
  if ((rc = refuse_kernel_lift_ranks(h, who))) return rc;
  const int N = h->N, N4 = (N + 3) & ~3;
  hipStream_t st = h->stream;
  ThompsonPass P;
  if ((rc = begin_pass(h, L, q, q, conditioned != 0, &P))) return rc;
  const int64_t M = h->M;
  const bool store = k > 1 || paths_out != nullptr;
  if (store)
    if ((rc = h->dacq_out.ensure(h, (size_t)q * M))) return rc;

  // ---- the draw: W scaled by sqrt(2 sigma2 / L) and padded to 16 columns
  const double scale = std::sqrt(2.0 * h->sigma2 / (double)L);
  std::vector<double> hW((size_t)16 * L, 0.0);
  for (int l = 0; l < L; ++l)
    for (int j = 0; j < q; ++j) hW[(size_t)l * 16 + j] = scale * weights[(size_t)l * q + j];
  if ((rc = upload_draw(h, P, L, omega, phase, hW, st))) return rc;

  SpanTimer& tm = h->th_timer;
  std::vector<double> hb(16, 0.0), hg((size_t)N * q, 0.0);
  if (conditioned) {
    // ---- 1, 2: the draw at the training rows, plus what the nugget adds to an observation; R^-1 s for the q columns
    std::vector<double> hs((size_t)N * q), ha((size_t)N * q), hw((size_t)N);
    HIPCHK(h, hipMemcpyAsync(hw.data(), h->dw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    const double nug = h->sigma2 * (h->R_diag - 1.0);
    std::vector<ColNoise> noise;
    if (eps && nug > 0.0)
      for (int j = 0; j < q; ++j) noise.push_back({std::sqrt(nug), j});
    if ((rc = solve_at_training_rows(h, P, L, q, true, noise, eps, hs, ha, st))) return rc;
    // ---- then b and g on the host
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
    HIPCHK(h, hipMemcpyAsync(P.coef, hng.data(), hng.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipStreamSynchronize(st));  // (hng leaves scope)
  }
  int s1 = 0;
  if ((rc = tm.mark(h, st, &s1))) return rc;
  tm.span(TH_SOLVE, P.s0, s1);
  if (coef_out) {
    memcpy(coef_out, hg.data(), (size_t)N * q * sizeof(double));
    for (int j = 0; j < q; ++j) coef_out[(size_t)N * q + j] = hb[j];
  }

  // ---- 3: the candidate chunks
  ThompsonArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.d = h->d; ta.L = L; ta.N = N; ta.q = q; ta.omega = P.omega; ta.phase = P.phase; ta.W = P.W;
  ta.X = h->dXs; ta.mode = conditioned ? 2 : 1; ta.minimize = minimize ? 1 : 0; ta.vals = store ? h->dacq_out : nullptr; ta.M = M;
  ta.rT = h->drT[0]; ta.ld = P.geo.Mc; ta.ngt = P.coef; ta.mu_part = h->dmu_part[0]; ta.S = P.geo.S; ta.beta = h->beta;
  for (int j = 0; j < 16; ++j) ta.bt[j] = hb[j];
  ta.blk_val = h->dblk_val; ta.blk_idx = h->dblk_idx; ta.nblk_total = P.nblk_total;
  if ((rc = for_each_chunk(h, P, conditioned != 0, st, ta, launch_thompson))) return rc;

  // ---- 4: the winners, and the stored values in the paths' own sign
  if (paths_out) HIPCHK(h, hipMemcpyAsync(paths_out, h->dacq_out, (size_t)q * M * sizeof(double), hipMemcpyDeviceToHost, st));
  if ((rc = winners(h, P, q, k, h->dacq_out, best_val, best_idx, best_x, st))) return rc;
  if (paths_out && minimize)  // stored in the criterion's sign: back to the path's own
    for (size_t i = 0; i < (size_t)q * M; ++i) paths_out[i] = -1 * paths_out[i];
  store_last(tm, P.geo.nchunk, &h->th_last);
  return BOGP_OK;
}

extern "C" int bogp_thompson_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks) {
  return h ? read_last(h->th_last, corr_ms, solve_ms, paths_ms, n_chunks) : BOGP_ERR_INVALID;
}

// ---- Thompson batches under modelled constraints -------------------------------------------------------------------------------------
// q batch members' JOINT paths of the m = 1 + n_con targets of a multi-target model (target 0 the objective, target t >= 1 a constraint):
// q m <= 16 columns over shared features.  The model's targets share R and are a priori independent, and its trend is a fixed constant,
// so column (j, t) is the plain simple-kriging path
//   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x),      g_{j,t} = R^-1 (z_{j,t}(X) + sqrt(sigma2_t (diag R - 1)) E[:, (j,t)])
//   1  the draw at the training rows: k_thompson in mode 0 over the q m columns, W scaled per column by sqrt(2 sigma2_t / L)
//   2  R^-1 s by the two gemms; gamma_t from dgamma_base; gamma_t - g on the host
//   3  per candidate chunk: the producer with its store, then k_thompson_constrained (kernels_thompson_constrained.hip)
//   4  the argmax / top-k tail over the 2 q scores (A_j: the objective where the drawn constraints hold; B_j: minus the violation)
// ABI column j m + t, DEVICE column t q + j (the kernel's gather).
extern "C" int bogp_sweep_thompson_constrained(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                                               const double* eps, int minimize, int n_con, const double* lo, const double* hi, int k,
                                               double* best_val, int64_t* best_idx, double* best_x, double* paths_out, double* coef_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_thompson_constrained";
  int rc;
  if ((rc = check_ready(h, who))) return rc;
  if ((rc = refuse_lift(h, who))) return rc;
  if ((rc = refuse_trend(h, who))) return rc;
  const int m = h->n_t;
  if (m < 2) FAIL(h, BOGP_ERR_INVALID, "%s: the committed model has one target and so no modelled constraint: bogp_sweep_thompson serves it", who);
  if (n_con != m - 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d, but the committed model has %d targets (one objective and %d constraints)", who, n_con, m, m - 1);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  if (q < 1 || q * m > BOGP_MAX_PATHS) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d members of %d targets: 1 <= q and q m <= %d columns", who, q, m, BOGP_MAX_PATHS);
  if ((rc = check_features_and_ranks(h, who, L, k))) return rc;
  if (!omega || !phase || !weights || !lo || !hi || !best_val || !best_idx)
    FAIL(h, BOGP_ERR_INVALID, "%s: omega, phase, weights, lo, hi, best_val and best_idx must be non-null", who);
  if ((rc = check_constraint_bounds(h, who, n_con, lo, hi))) return rc;
  const int N = h->N, Np = h->Np, qm = q * m;
  if ((rc = check_draw_finite_and_mode(h, who, L, qm, omega, phase, weights, eps))) return rc;
  if ((rc = refuse_kernel_lift_ranks(h, who))) return rc;
  const int N4 = (N + 3) & ~3;
  const auto dcol = [&](int j, int t) { return t * q + j; };  // the device column of ABI column j m + t
  hipStream_t st = h->stream;
  ThompsonPass P;
  if ((rc = begin_pass(h, L, qm, 2 * q, true, &P))) return rc;
  const int64_t M = h->M;
  const bool ranked = k > 1;
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
  if ((rc = upload_draw(h, P, L, omega, phase, hW, st))) return rc;

  SpanTimer& tm = h->th_timer;
  // ---- 1, 2: the draw at the training rows (device columns), plus what the nugget adds to an observation; R^-1 s for the q m columns
  std::vector<double> hs((size_t)N * qm), ha((size_t)N * qm), hgamma((size_t)m * Np);
  HIPCHK(h, hipMemcpyAsync(hgamma.data(), h->dgamma_base.ptr, hgamma.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<ColNoise> noise;
  if (eps && h->R_diag - 1.0 > 0.0)
    for (int t = 0; t < m; ++t) {
      const double sn = std::sqrt(h->sigma2_t[t] * (h->R_diag - 1.0));
      for (int j = 0; j < q; ++j) noise.push_back({sn, j * m + t});  // (in device column order: t q + j)
    }
  if ((rc = solve_at_training_rows(h, P, L, qm, false, noise, eps, hs, ha, st))) return rc;
  // ---- then gamma_t - g on the host
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
  HIPCHK(h, hipMemcpyAsync(P.coef, hcoef.data(), hcoef.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));  // (hcoef leaves scope)
  int s1 = 0;
  if ((rc = tm.mark(h, st, &s1))) return rc;
  tm.span(TH_SOLVE, P.s0, s1);

  // ---- 3: the candidate chunks
  ThompsonConstrainedArgs ca;
  memset(&ca, 0, sizeof(ca));
  ca.X = h->dXs; ca.d = h->d; ca.L = L; ca.N = N; ca.q = q; ca.m = m; ca.omega = P.omega; ca.phase = P.phase; ca.W = P.W;
  ca.rT = h->drT[0]; ca.ld = P.geo.Mc; ca.coef = P.coef; ca.beta = h->beta; ca.minimize = minimize ? 1 : 0; ca.M = M;
  for (int t = 1; t < m; ++t) {
    ca.lo[t] = lo[t - 1]; ca.hi[t] = hi[t - 1];
    ca.inv_sd[t] = 1.0 / std::sqrt(h->sigma2_t[t]);
  }
  double* dscores = ranked ? h->dacq_out.ptr : nullptr;
  double* dpaths = paths_out ? h->dacq_out.ptr + n_scores : nullptr;
  ca.scores = dscores; ca.paths = dpaths;
  ca.blk_val = h->dblk_val; ca.blk_idx = h->dblk_idx; ca.nblk_total = P.nblk_total;
  if ((rc = for_each_chunk(h, P, true, st, ca, launch_thompson_constrained))) return rc;

  // ---- 4: the winners of the 2 q scores: [q][2][k], member j's A ranks, then its B ranks
  if (paths_out) HIPCHK(h, hipMemcpyAsync(paths_out, dpaths, (size_t)qm * M * sizeof(double), hipMemcpyDeviceToHost, st));
  if ((rc = winners(h, P, 2 * q, k, dscores, best_val, best_idx, best_x, st))) return rc;
  store_last(tm, P.geo.nchunk, &h->thc_last);
  return BOGP_OK;
}

extern "C" int bogp_thompson_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks) {
  return h ? read_last(h->thc_last, corr_ms, solve_ms, paths_ms, n_chunks) : BOGP_ERR_INVALID;
}
