// bogp_api_believer.hip -- the C ABI of libbogp.so (include/bogp.h) for Kriging-believer batches: bogp_sweep_believer, q proposals from q
// criteria where step j sees the variance conditioned on the pending points and on the winners of the steps before it.
//   pass 0            the plain sweep of bogp_api_sweep.hip (run_sweep): mu, MSE_0 = sigma2 max(0, s_0) per candidate, and -- without pending
//                     points -- step 0's criterion and argmax, which are therefore bogp_sweep's bit for bit
//   per believed p    a solve a = V^T (V r(p)) with the kernels of bogp_gradient, the p-by-p terms on the host (at most 32 x 32), then ONE
//                     pass over the candidates: producer per chunk -> k_believer (kernels_believer.hip); when one chunk holds every
//                     candidate the producer runs for the first believed point only
// A row that is a winner keeps its criterion value in the outputs but leaves the argmax of the later steps.
// The running variance is kept as sigma2 s, started from the sweep's clamped MSE_0: where s_0 < 0 the clamp changes nothing that is
// returned (s only decreases, and every output is max(0, .) of it).
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

void bogp::believer_release(bogp_handle* h) {
  dfree(h->dbel_s); dfree(h->dbel_C); dfree(h->dbel_row); dfree(h->dbel_small);
  h->bel_s_cap = h->bel_C_cap = h->bel_row_cap = h->bel_small_cap = 0;
  for (auto e : h->bel_ev) (void)hipEventDestroy(e);
  h->bel_ev.clear();
}

namespace {

constexpr double PIVOT_FLOOR = 1e-12;  // the noise floor of a unit prior variance: a point at or below it is already determined

struct Believed {  // host side of the recursion: row i of L holds c_k(p_i) for k < i and sqrt(pivot_i) at k = i (0 for a guarded pivot)
  int n = 0;
  std::vector<double> r, a, u;  // [n][N], [n][N], [n]
  double L[BOGP_MAX_BELIEVED][BOGP_MAX_BELIEVED];
  int slot[BOGP_MAX_BELIEVED];  // column of dbel_C, -1: guarded or never stored
};

hipEvent_t bel_event(bogp_handle* h, size_t i) {
  while (h->bel_ev.size() <= i) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    h->bel_ev.push_back(e);
  }
  return h->bel_ev[i];
}

struct Plan {  // chunking of the candidate passes: the producer's geometry of run_sweep for a constant-trend model
  int64_t Mc, nchunk, nblk_total;
  int S;
};

}  // namespace

extern "C" int bogp_sweep_believer(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                                   int believe_plugin, const double* pending, int n_pending, double* best_val, int64_t* best_idx,
                                   double* best_x, double* pivots, double* acq_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: no committed model: call bogp_commit first");
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: no candidates: call bogp_candidates_upload/bind first");
  if (q < 1 || n_pending < 0 || q + n_pending > BOGP_MAX_BELIEVED)
    FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: q = %d, n_pending = %d: q >= 1 and q + n_pending <= %d", q, n_pending, BOGP_MAX_BELIEVED);
  if (!acq_id || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: acq_id, best_val and best_idx must be non-null");
  if (n_pending > 0 && !pending) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: n_pending = %d but pending is null", n_pending);
  for (int i = 0; i < q; ++i) {
    if (acq_id[i] < 0 || acq_id[i] > 3) FAIL(h, BOGP_ERR_INVALID, "unknown acquisition id %d", acq_id[i]);
    const bool zero_ok = acq_id[i] == BOGP_ACQ_EPSILON_PI;  // epsilon = 0 is plain PI
    if (acq_id[i] != BOGP_ACQ_EI && (!acq_par || !(acq_par[i] > 0 || (zero_ok && acq_par[i] == 0))))
      FAIL(h, BOGP_ERR_INVALID, "acquisition parameter %d must be > 0 (the reference asserts alpha/epsilon/t > 0)", i);
  }
  const int d = h->d, N = h->N, Np = h->Np;
  if (q > h->M) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: q = %d proposals from %lld candidates (every step takes a row no step before it took)", q, (long long)h->M);
  for (size_t i = 0; i < (size_t)n_pending * d; ++i)
    if (!std::isfinite(pending[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: pending entry %zu is not finite", i);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: constant trend basis only (the committed basis has %d columns)", h->p);
  if (h->n_t != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: one target only (the committed model has %d)", h->n_t);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: a lift is set (bogp_lift_set): call bogp_lift_clear first");
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: runs on one rank (the communicator has %d)", h->comm_world);
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  const int P = n_pending, Btot = P + q;
  invalidate_sweep_results(h);  // dbest_* are overwritten

  // ---- pass 0: the plain sweep; with pending points only the moments (step 0 is evaluated behind the last pending point)
  int rc = P == 0 ? run_sweep(h, true, 1, acq_id, acq_par, plugin, minimize, true, true, true)
                  : run_sweep(h, true, 0, nullptr, nullptr, 0.0, minimize, false, true, true);
  if (rc) return rc;
  if ((rc = candidates_ready(h))) return rc;

  // ---- geometry of the later passes (run_sweep's for p = 1: chunk bytes, slices of 8 x 32 training rows)
  Plan pl;
  {
    size_t chunk_bytes = (size_t)1 << 30;
    if (const char* env = getenv("BOGP_CHUNK_MB")) chunk_bytes = (size_t)std::max(1, atoi(env)) << 20;
    const int64_t Mpad = ((M + 63) / 64) * 64;
    int64_t Mc = (int64_t)(chunk_bytes / ((size_t)Np * sizeof(double)) / 64) * 64;
    pl.Mc = std::max<int64_t>(64, std::min<int64_t>(Mc, Mpad));
    pl.nchunk = (M + pl.Mc - 1) / pl.Mc;
    pl.nblk_total = (M + 63) / 64 + pl.nchunk;
    pl.S = (Np / 32 + 7) / 8;
  }
  const size_t small_n = (size_t)d + 3 * (size_t)N + 2 * BOGP_MAX_BELIEVED + (size_t)BOGP_MAX_BELIEVED * d;
  if ((rc = ensure(h, &h->dbel_s, &h->bel_s_cap, (size_t)M))) return rc;
  if ((rc = ensure(h, &h->dbel_row, &h->bel_row_cap, (size_t)2 * M))) return rc;
  if ((rc = ensure(h, &h->dbel_small, &h->bel_small_cap, small_n))) return rc;
  if (Btot > 2)
    if ((rc = ensure(h, &h->dbel_C, &h->bel_C_cap, (size_t)(Btot - 2) * M))) return rc;  // the last winner runs no pass, the point before it stores no column
  if ((rc = ensure(h, &h->drT[0], &h->rT_cap[0], (size_t)Np * pl.Mc))) return rc;
  if ((rc = ensure(h, &h->dmu_part[0], &h->mu_part_cap[0], (size_t)pl.S * pl.Mc))) return rc;
  if ((rc = ensure(h, &h->dw_part[0], &h->w_part_cap[0], (size_t)pl.S * pl.Mc))) return rc;
  if ((rc = ensure(h, &h->dblk_val, &h->blk_val_cap, (size_t)pl.nblk_total))) return rc;
  if ((rc = ensure(h, &h->dblk_idx, &h->blk_idx_cap, (size_t)pl.nblk_total))) return rc;
  if (!h->dbest_val) HIPCHK(h, hipMalloc((void**)&h->dbest_val, BOGP_MAX_Q * sizeof(double)));
  if (!h->dbest_idx) HIPCHK(h, hipMalloc((void**)&h->dbest_idx, BOGP_MAX_Q * sizeof(int64_t)));
  double* dpt = h->dbel_small;          // d
  double* dr = dpt + d;                 // N
  double* dvr = dr + N;                 // N
  double* da = dvr + N;                 // N
  double* dkk = da + N;                 // 32 correlations of the point with the believed rows, 32 distances
  double* drows = dkk + 2 * BOGP_MAX_BELIEVED;  // 32 x d believed rows
  double* dacq_row = h->dbel_row;
  double* dmse_row = h->dbel_row + M;

  HIPCHK(h, hipMemcpyAsync(h->dbel_s, h->dmse_out, (size_t)M * sizeof(double), hipMemcpyDeviceToDevice, st));
  std::vector<double> hgamma((size_t)N), hw((size_t)N), hrow((size_t)d), hk(BOGP_MAX_BELIEVED);
  HIPCHK(h, hipMemcpyAsync(hgamma.data(), h->dgamma, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(hw.data(), h->dw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));

  Believed bl;
  bl.r.resize((size_t)Btot * N);
  bl.a.resize((size_t)Btot * N);
  bl.u.resize(Btot);
  memset(bl.L, 0, sizeof(bl.L));
  int slots = 0;
  bool chunk_resident = false;  // all candidates fit one chunk and the producer has filled it: r(x) and the w-sums stay for the later points
  size_t nev = 0;
  std::vector<size_t> ev_solve, ev_chunk;  // event indices: (begin, end) per solve; (begin, producer end, end) per chunk
  h->bel_passes = 0;
  double plug = plugin;
  auto believe_mean = [&](double mu) {
    if (!believe_plugin) return;
    const double y_hat = minimize ? mu : -1 * mu;  // the plugin arrives in the criterion's own sign (already negated when maximising)
    if (y_hat < plug) plug = y_hat;
  };

  // One believed point: solve, the host's row of the recursion, and -- unless the pivot is guarded and no step follows -- a candidate pass.
  // `step` >= 0: the pass also evaluates that step's criterion and leaves its winner in dbest_*[0]; `pass`: false for the last winner, whose
  // pivot alone is reported.  `is_pending`: mu(p) as the host forms it joins the plugin before the pass (a winner's mean is read from the
  // sweep's array by the caller).  `row`: the candidate row a winner is (its variance becomes exactly 0), -1 for a pending point.
  auto believe = [&](const double* x, int step, bool pass, bool is_pending, int64_t row) -> int {
    const int i = bl.n;
    hipEvent_t e0 = bel_event(h, nev), e1 = bel_event(h, nev + 1);
    if (!e0 || !e1) FAIL(h, BOGP_ERR_HIP, "hipEventCreate failed");
    ev_solve.push_back(nev);
    nev += 2;
    HIPCHK(h, hipEventRecord(e0, st));
    HIPCHK(h, hipMemcpyAsync(dpt, x, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(drows + (size_t)i * d, x, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_batch_corr(h->kernel, h->dX, N, d, h->dtheta, dpt, 1, dr, dvr, st));  // (dvr: the distances, overwritten next)
    HIPCHK(h, launch_gemm(0, 0, N, 1, N, 1.0, h->dV, h->ldr, dr, N, 0.0, dvr, N, st, 1));   // V r
    HIPCHK(h, launch_gemm(1, 0, N, 1, N, 1.0, h->dV, h->ldr, dvr, N, 0.0, da, N, st, 2));   // a = V^T (V r) = R^-1 r
    HIPCHK(h, launch_batch_corr(h->kernel, drows, i + 1, d, h->dtheta, dpt, 1, dkk, dkk + BOGP_MAX_BELIEVED, st));  // k(p, p_k), k <= i
    double* ri = &bl.r[(size_t)i * N];
    double* ai = &bl.a[(size_t)i * N];
    HIPCHK(h, hipMemcpyAsync(ri, dr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(ai, da, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hk.data(), dkk, (size_t)(i + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipEventRecord(e1, st));
    HIPCHK(h, hipStreamSynchronize(st));
    double rg = 0.0, rw = 0.0;
    for (int n = 0; n < N; ++n) {
      rg += ri[n] * hgamma[n];
      rw += ri[n] * hw[n];
    }
    if (is_pending) believe_mean(h->beta + rg);
    bl.u[i] = h->estimate_trend ? (rw - 1.0) / h->G : 0.0;
    // row i of the recursion: kappa0(p_i, p_k) = k - r_i . a_k + u_i u_k, orthogonalised against the rows before
    for (int k = 0; k <= i; ++k) {
      const double* ak = &bl.a[(size_t)k * N];
      double dot = 0.0;
      for (int n = 0; n < N; ++n) dot += ri[n] * ak[n];
      double b = hk[k] - dot + bl.u[i] * bl.u[k];
      for (int l = 0; l < k; ++l) b -= bl.L[i][l] * bl.L[k][l];
      if (k < i) {
        bl.L[i][k] = bl.L[k][k] > 0.0 ? b / bl.L[k][k] : 0.0;
      } else {
        if (pivots) pivots[i] = b;
        bl.L[i][i] = b > PIVOT_FLOOR ? std::sqrt(b) : 0.0;  // (NaN fails the comparison: guarded)
      }
    }
    bl.slot[i] = -1;
    bl.n = i + 1;
    const bool active = bl.L[i][i] > 0.0;
    if (!pass || (!active && step < 0)) return BOGP_OK;
    const bool store = active && (bl.n < Btot - 1);  // a later pass will read this column
    if (store) bl.slot[i] = slots++;
    BelieverArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.Xs = h->dXs; ba.theta = h->dtheta; ba.pt = dpt; ba.rT = h->drT[0]; ba.w_part = h->dw_part[0]; ba.avec = da;
    ba.d = d; ba.N = N; ba.S = pl.S; ba.Mc = pl.Mc; ba.M = M;
    ba.update = active ? 1 : 0;
    ba.self_row = row;
    ba.u_p = bl.u[i]; ba.inv_root = active ? 1.0 / bl.L[i][i] : 0.0; ba.G = h->G; ba.estimate_trend = h->estimate_trend;
    for (int k = 0; k < i; ++k)
      if (bl.slot[k] >= 0 && bl.L[k][k] > 0.0) {
        ba.prev_slot[ba.nprev] = bl.slot[k];
        ba.prev_c[ba.nprev] = bl.L[i][k];
        ++ba.nprev;
      }
    ba.C = h->dbel_C; ba.c_out = store ? h->dbel_C + (size_t)bl.slot[i] * M : nullptr; ba.s = h->dbel_s; ba.sigma2 = h->sigma2;
    ba.eval = step >= 0 ? 1 : 0;
    if (step >= 0) {
      ba.acq_id = acq_id[step]; ba.acq_par = acq_par ? acq_par[step] : 0.0; ba.plugin = plug; ba.minimize = minimize;
      ba.n_taken = step;  // the winners of steps 0 .. step - 1
      for (int k = 0; k < step; ++k) ba.taken[k] = best_idx[k];
    }
    ba.mu = h->dmu_out; ba.acq_out = dacq_row; ba.mse_out = dmse_row; ba.blk_val = h->dblk_val; ba.blk_idx = h->dblk_idx;
    int64_t blk_offset = 0;
    for (int64_t c = 0; c < pl.nchunk; ++c) {
      const int64_t m0 = c * pl.Mc, mcount = std::min<int64_t>(pl.Mc, M - m0), Mc_eff = ((mcount + 63) / 64) * 64;
      hipEvent_t c0 = bel_event(h, nev), c1 = bel_event(h, nev + 1), c2 = bel_event(h, nev + 2);
      if (!c0 || !c1 || !c2) FAIL(h, BOGP_ERR_HIP, "hipEventCreate failed");
      ev_chunk.push_back(nev);
      nev += 3;
      HIPCHK(h, hipEventRecord(c0, st));
      if (active && !chunk_resident) {
        CorrArgs ca;
        ca.Xs = h->dXs; ca.M = M; ca.m0 = m0; ca.Mc = pl.Mc; ca.d = d; ca.Np = Np; ca.nblk_per_split = 8;
        ca.sqrt_theta = h->dsqrt_theta; ca.XthT = h->dXthT; ca.xnorm = h->dXnorm; ca.gamma = h->dgamma; ca.wvec = h->dw;
        ca.rT = h->drT[0]; ca.mu_part = h->dmu_part[0]; ca.w_part = h->dw_part[0];
        HIPCHK(h, launch_corr_chunk(h->kernel, ca, (int)(Mc_eff / 64), pl.S, st));
        chunk_resident = pl.nchunk == 1;
      }
      HIPCHK(h, hipEventRecord(c1, st));
      ba.m0 = m0; ba.mcount = mcount; ba.blk_offset = blk_offset;
      HIPCHK(h, launch_believer(h->kernel, ba, st));
      HIPCHK(h, hipEventRecord(c2, st));
      blk_offset += (mcount + 63) / 64;
    }
    ++h->bel_passes;
    if (step >= 0) HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, blk_offset, pl.nblk_total, 1, h->dbest_val, h->dbest_idx, st));
    return BOGP_OK;
  };

  for (int i = 0; i < P; ++i) {
    if ((rc = believe(pending + (size_t)i * d, i == P - 1 ? 0 : -1, true, true, -1))) return rc;
  }

  for (int j = 0; j < q; ++j) {
    // the winner of step j is in dbest_*[0]; its criterion values / MSE in the sweep's own arrays (step 0 without pending points) or the row buffers
    const bool from_sweep = j == 0 && P == 0;
    int64_t idx = 0;
    HIPCHK(h, hipMemcpyAsync(&best_val[j], h->dbest_val, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(&idx, h->dbest_idx, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (acq_out) HIPCHK(h, hipMemcpyAsync(acq_out + (size_t)j * M, from_sweep ? h->dacq_out : dacq_row, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    if (mse_out) HIPCHK(h, hipMemcpyAsync(mse_out + (size_t)j * M, from_sweep ? h->dmse_out : dmse_row, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    best_idx[j] = idx;
    if (idx < 0 || idx >= M) FAIL(h, BOGP_ERR_HIP, "bogp_sweep_believer: step %d returned row %lld outside [0, %lld)", j, (long long)idx, (long long)M);
    double mu_w = 0.0;
    HIPCHK(h, hipMemcpyAsync(hrow.data(), h->dXs + (size_t)idx * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(&mu_w, h->dmu_out + idx, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (best_x) memcpy(best_x + (size_t)j * d, hrow.data(), (size_t)d * sizeof(double));
    believe_mean(mu_w);
    if (j == q - 1) {
      if (pivots && (rc = believe(hrow.data(), -1, false, false, idx))) return rc;
      break;
    }
    if ((rc = believe(hrow.data(), j + 1, true, false, idx))) return rc;
  }

  // times of the solves and of the passes (everything is complete: the last step was read back)
  HIPCHK(h, hipStreamSynchronize(st));
  h->bel_corr_ms = h->bel_solve_ms = h->bel_pass_ms = 0;
  for (size_t k : ev_solve) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->bel_ev[k], h->bel_ev[k + 1]);
    h->bel_solve_ms += ms;
  }
  for (size_t k : ev_chunk) {
    float a = 0, b = 0;
    (void)hipEventElapsedTime(&a, h->bel_ev[k], h->bel_ev[k + 1]);
    (void)hipEventElapsedTime(&b, h->bel_ev[k + 1], h->bel_ev[k + 2]);
    h->bel_corr_ms += a;
    h->bel_pass_ms += b;
  }
  return BOGP_OK;
}

extern "C" int bogp_believer_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* believer_ms, int* n_passes) {
  if (!h) return BOGP_ERR_INVALID;
  if (corr_ms) *corr_ms = h->bel_corr_ms;
  if (solve_ms) *solve_ms = h->bel_solve_ms;
  if (believer_ms) *believer_ms = h->bel_pass_ms;
  if (n_passes) *n_passes = h->bel_passes;
  return BOGP_OK;
}
