// bogp_api_believer.hip -- the C ABI of libbogp.so (include/bogp.h) for Kriging-believer batches: q proposals from q steps where step j
// sees the variance conditioned on the pending points and on the winners of the steps before it.  Four entries, ONE recursion
// (believer_run): an entry keeps its argument checks, its pass 0 (run_sweep with the family's request: mu, the clamped MSE_0 and --
// without pending points -- step 0's criterion and argmax, the family's plain sweep bit for bit) and hands over what differs.
//   per believed p    a solve a = V^T (V r(p)) with the kernels of bogp_gradient, the p-by-p terms on the host (at most 32 x 32), then ONE
//                     pass over the candidates: producer per chunk -> k_believer (kernels_believer.hip); when one chunk holds every
//                     candidate the producer runs for the first believed point only
// A row that is a winner keeps its criterion value in the outputs but leaves the argmax of the later steps.  The running variance
// is kept as sigma2 s, started from the sweep's clamped MSE_0: where s_0 < 0 the clamp changes nothing that is returned (s only
// decreases, and every output is max(0, .) of it).
//                                 bogp_sweep_believer            bogp_sweep_believer_ehvi               bogp_sweep_believer_constrained        bogp_sweep_believer_ehvi_constrained
//   a believed mean               lowers the plugin              joins the front (m-vector)             lowers the plugin if feasible          its objectives join the front if feasible
//   a step's criterion            k_believer itself, per chunk   k_believer_ehvi, one launch, after     k_believer_constrained, likewise       k_believer_ehvi_constrained, likewise
//                                 (one record per 64 rows)       k_believer stored c(x) in unit variance (one record per 256 rows)
//   a column c_k(x) is stored     when a later pass reads it     for every point past the guard         likewise                               likewise
//   a guarded pivot before a step k_believer without the update  the criterion kernel alone (c = null)  likewise                               likewise
//   before a step                 --                             the front's cells, rebuilt + uploaded  --                                     the feasible front's cells, likewise
//   a winner's mean is believed   also behind the last step      between two steps only                 likewise                               likewise
// The m targets share the bracket of gpr.py:502-510, so ONE downdate in correlation units serves them all.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_handle.h"
#include "bogp_internal.h"

using namespace bogp;

namespace {

constexpr double PIVOT_FLOOR = 1e-12;  // the noise floor of a unit prior variance: a point at or below it is already determined

struct Believed {  // host side of the recursion: row i of L holds c_k(p_i) for k < i and sqrt(pivot_i) at k = i (0 for a guarded pivot)
  int n = 0;
  std::vector<double> r, a, u;  // [n][N], [n][N], [n]
  double L[BOGP_MAX_BELIEVED][BOGP_MAX_BELIEVED];
  int slot[BOGP_MAX_BELIEVED];  // column of dbel_C, -1: guarded or never stored
};

struct SolveBufs {  // dbel_small: the point, r(p), V r(p), R^-1 r(p), the point's correlations with the believed rows, those rows
  double *dpt, *dr, *dvr, *da, *dkk, *drows;
  static size_t doubles(int d, int N) { return (size_t)d + 3 * (size_t)N + 2 * BOGP_MAX_BELIEVED + (size_t)BOGP_MAX_BELIEVED * d; }
  SolveBufs(double* base, int d, int N) {
    dpt = base;                          // d
    dr = dpt + d;                        // N
    dvr = dr + N;                        // N
    da = dvr + N;                        // N
    dkk = da + N;                        // 32 correlations of the point with the believed rows, 32 distances
    drows = dkk + 2 * BOGP_MAX_BELIEVED;  // 32 x d believed rows
  }
};

// kinds of the spans on h->bel_timer: the solves, the chunks' producer and k_believer launches, the family's criterion kernel (m > 1)
enum { B_SOLVE, B_PRODUCER, B_PASS, B_CRITERION };

// The solve of one believed point x -- a = V^T (V r(x)) = R^-1 r(x) with the kernels of bogp_gradient, one solve span -- and the
// host's row of the recursion: bl gains r, a, u and row bl.n of L, pivots[bl.n] (if given) the pivot.  hw: L^-T Ft.
int believed_solve(bogp_handle* h, Believed& bl, const SolveBufs& sb, const double* x, const std::vector<double>& hw, std::vector<double>& hk,
                   double* pivots) {
  const int i = bl.n, d = h->d, N = h->N;
  hipStream_t st = h->stream;
  int e0 = 0, e1 = 0;
  if (int e = h->bel_timer.mark(h, st, &e0)) return e;
  HIPCHK(h, hipMemcpyAsync(sb.dpt, x, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(sb.drows + (size_t)i * d, x, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_batch_corr(h->kernel, h->dX, N, d, h->dtheta, sb.dpt, 1, sb.dr, sb.dvr, st));  // (dvr: the distances, overwritten next)
  HIPCHK(h, launch_gemm(0, 0, N, 1, N, 1.0, h->dV, h->ldr, sb.dr, N, 0.0, sb.dvr, N, st, 1));   // V r
  HIPCHK(h, launch_gemm(1, 0, N, 1, N, 1.0, h->dV, h->ldr, sb.dvr, N, 0.0, sb.da, N, st, 2));   // a = V^T (V r) = R^-1 r
  HIPCHK(h, launch_batch_corr(h->kernel, sb.drows, i + 1, d, h->dtheta, sb.dpt, 1, sb.dkk, sb.dkk + BOGP_MAX_BELIEVED, st));  // k(p, p_k), k <= i
  double* ri = &bl.r[(size_t)i * N];
  double* ai = &bl.a[(size_t)i * N];
  HIPCHK(h, hipMemcpyAsync(ri, sb.dr, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(ai, sb.da, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(hk.data(), sb.dkk, (size_t)(i + 1) * sizeof(double), hipMemcpyDeviceToHost, st));
  if (int e = h->bel_timer.mark(h, st, &e1)) return e;
  h->bel_timer.span(B_SOLVE, e0, e1);
  HIPCHK(h, hipStreamSynchronize(st));
  double rw = 0.0;
  for (int n = 0; n < N; ++n) rw += ri[n] * hw[n];
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
  return BOGP_OK;
}

// One chunk of a candidate pass: the producer (where `produce`), then k_believer over rows [ba.m0, ba.m0 + ba.mcount); three marks,
// a producer and a pass span.
int believer_chunk(bogp_handle* h, const SweepGeometry& pl, const BelieverArgs& ba, bool produce) {
  hipStream_t st = h->stream;
  SpanTimer& tm = h->bel_timer;
  int e, c0 = 0, c1 = 0, c2 = 0;
  if ((e = tm.mark(h, st, &c0))) return e;
  if (produce) HIPCHK(h, launch_corr_chunk(h->kernel, corr_chunk_args(h, pl, ba.m0, 0), (int)((ba.mcount + 63) / 64), pl.S, st));
  if ((e = tm.mark(h, st, &c1))) return e;
  HIPCHK(h, launch_believer(h->kernel, ba, st));
  if ((e = tm.mark(h, st, &c2))) return e;
  tm.span(B_PRODUCER, c0, c1); tm.span(B_PASS, c1, c2);
  return BOGP_OK;
}

// ---- the recursion, once ----------------------------------------------------------------------------------------------------------
// The handle's believer arrays are shared by the four families and laid out per call (M candidates, m targets, B = n_pending + q
// believed points; every call sizes and fills them anew, nothing is carried from the call before):
//                  dbel_s    dbel_row: `lead` rows of M, then the MSE block        dbel_C [columns][M] c_k(x)
//   one target     [M]       [values | MSE M]                          lead 1      B - 2: the last winner runs no pass, the point before
//                                                                                  it stores no column (no pass reads it)
//   EHVI           [M][m]    [EHVI | scratch | MSE M x m]              lead 2      B - 1: the criterion kernel reads every column
//   constrained    [M][m]    [values | PoF | scratch | MSE M x m]      lead 3      B - 1
//   constr. EHVI   [M][m]    [values | PoF | scratch | MSE M x m]      lead 3      B - 1   (m = objectives + constraints)
// dbel_s is sigma2_k s_B(x), unclamped below the sweep's own clamp of s_0; `scratch` is k_believer's own s in unit variance (m > 1: not
// used); dbel_small is SolveBufs; dehvi_cells ([lower C x m | upper C x m], m the objectives) is the two EHVI entries' alone.

struct StepRows {  // rows of step j for the caller: out + j n <- the sweep's own array (step 0 without pending points) or dbel_row + at M
  double* out;     // null: not wanted
  const DevBuf<double>* sweep;
  int at, width;   // in units of M doubles; n = width M
};

// What a family hands the recursion: its layout, its outputs and what differs in code.
struct BelieverFamily {
  const char* who;
  int m = 1;  // targets.  1: k_believer itself evaluates a step, with the four fields below; > 1: it stores c(x), then `criterion` runs
  const int* acq_id = nullptr;
  const double* acq_par = nullptr;  // null: zeros
  int minimize = 0;
  const double* plugin = nullptr;   // the running plugin, as `mean` leaves it
  int lead = 1;                     // rows of dbel_row in front of the MSE block (the table above)
  double* best_val = nullptr;
  int64_t* best_idx = nullptr;
  double *best_x = nullptr, *best_mu = nullptr, *pivots = nullptr;  // each may be null
  StepRows rows[3] = {};
  std::function<void(const double* mu)> mean;  // a believed mean (m values): a pending point's as the host forms it, a winner's from the sweep's array
  std::function<int(int step)> step_begin;     // (may be empty) in front of a step's pass, behind the believed mean
  // m > 1: the launch over all M rows behind the column pass.  The step arrives filled (BelieverStep, bogp_internal.h); with `eval` set,
  // n_taken is the step's number and the values go to dbel_row, the MSE block to dbel_row + lead M.  The family copies it into its
  // argument block, adds what is its own and launches.
  std::function<hipError_t(const BelieverStep& bs)> criterion;
};

// Behind pass 0 (dmu_out, dmse_out and -- without pending points -- step 0's winner in dbest_*[0] are in place): the pending points,
// then per step the read-back of its winner and the pass that believes it.
int believer_run(bogp_handle* h, const BelieverFamily& f, int q, const double* pending, int P) {
  const int d = h->d, N = h->N, Np = h->Np, m = f.m, Btot = P + q;
  const bool one = m == 1;
  const int64_t M = h->M;
  hipStream_t st = h->stream;
  int rc;
  SweepGeometry pl;  // the sweep's own for a constant-trend model
  if ((rc = sweep_geometry(h, Np, &pl))) return rc;
  const int64_t nblk_total = one ? (M + 63) / 64 + pl.nchunk : (M + 255) / 256;
  const int ncol = Btot - (one ? 2 : 1);
  if ((rc = h->dbel_s.ensure(h, (size_t)M * m))) return rc;
  if ((rc = h->dbel_row.ensure(h, (size_t)(f.lead + m) * M))) return rc;
  if ((rc = h->dbel_small.ensure(h, SolveBufs::doubles(d, N)))) return rc;
  if (ncol > 0)
    if ((rc = h->dbel_C.ensure(h, (size_t)ncol * M))) return rc;
  if ((rc = h->drT[0].ensure(h, (size_t)Np * pl.Mc))) return rc;
  if ((rc = h->dmu_part[0].ensure(h, (size_t)pl.S * pl.Mc))) return rc;
  if ((rc = h->dw_part[0].ensure(h, (size_t)pl.S * pl.Mc))) return rc;
  if ((rc = ensure_sweep_outputs(h, 1, nblk_total, 0, false))) return rc;
  const SolveBufs sb(h->dbel_small, d, N);
  double* dscratch = h->dbel_row + (size_t)(f.lead - 1) * M;  // (m > 1)
  double* dmse_row = h->dbel_row + (size_t)f.lead * M;

  HIPCHK(h, hipMemcpyAsync(h->dbel_s, h->dmse_out, (size_t)M * m * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (!one) HIPCHK(h, hipMemsetAsync(dscratch, 0, (size_t)M * sizeof(double), st));
  const size_t n_gamma = one ? (size_t)N : (size_t)m * Np;  // the active target's gamma, or every target's with Np a row
  std::vector<double> hgamma(n_gamma), hw((size_t)N), hrow((size_t)d), hk(BOGP_MAX_BELIEVED), hmu((size_t)m);
  HIPCHK(h, hipMemcpyAsync(hgamma.data(), one ? h->dgamma : h->dgamma_base.ptr, n_gamma * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(hw.data(), h->dw, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));

  Believed bl;
  bl.r.resize((size_t)Btot * N);
  bl.a.resize((size_t)Btot * N);
  bl.u.resize(Btot);
  memset(bl.L, 0, sizeof(bl.L));
  int slots = 0;
  bool chunk_resident = false;  // all candidates fit one chunk and the producer has filled it: r(x) and the w-sums stay for the later points
  h->bel_timer.begin();
  h->bel_passes = 0;

  // One believed point: solve, the host's row of the recursion, and -- unless the pivot is guarded and no step follows -- a candidate pass.
  // `step` >= 0: the pass also evaluates that step's criterion and leaves its winner in dbest_*[0]; `pass`: false for the last winner, whose
  // pivot alone is reported.  `is_pending`: mu(p) = beta + r . gamma_k as the host forms it is believed before the pass (a winner's mean is
  // read from the sweep's array by the winner loop).  `row`: the candidate row a winner is, -1 for a pending point.
  auto believe = [&](const double* x, int step, bool pass, bool is_pending, int64_t row) -> int {
    const int i = bl.n;
    if (int rs = believed_solve(h, bl, sb, x, hw, hk, f.pivots)) return rs;
    if (is_pending) {
      const double* ri = &bl.r[(size_t)i * N];
      for (int t = 0; t < m; ++t) {
        double rg = 0.0;
        for (int n = 0; n < N; ++n) rg += ri[n] * hgamma[(size_t)t * Np + n];
        hmu[t] = h->beta + rg;
      }
      f.mean(hmu.data());
    }
    const bool active = bl.L[i][i] > 0.0;
    if (!pass || (!active && step < 0)) return BOGP_OK;
    if (step >= 0 && f.step_begin)
      if (int rs = f.step_begin(step)) return rs;
    const bool store = active && (!one || bl.n < Btot - 1);  // one target: only where a later pass will read this column
    if (store) bl.slot[i] = slots++;
    double* col = store ? h->dbel_C + (size_t)bl.slot[i] * M : nullptr;
    int64_t blk_offset = 0;
    if (one || active) {  // m > 1 behind a guarded pivot: no column to form, the criterion launch alone
      BelieverArgs ba;
      memset(&ba, 0, sizeof(ba));
      ba.Xs = h->dXs; ba.theta = h->dtheta; ba.pt = sb.dpt; ba.rT = h->drT[0]; ba.w_part = h->dw_part[0]; ba.avec = sb.da;
      ba.d = d; ba.N = N; ba.S = pl.S; ba.Mc = pl.Mc; ba.M = M;
      ba.update = active ? 1 : 0;
      ba.self_row = one ? row : -1;
      ba.u_p = bl.u[i]; ba.inv_root = active ? 1.0 / bl.L[i][i] : 0.0; ba.G = h->G; ba.estimate_trend = h->estimate_trend;
      for (int k = 0; k < i; ++k)
        if (bl.slot[k] >= 0 && bl.L[k][k] > 0.0) {
          ba.prev_slot[ba.nprev] = bl.slot[k];
          ba.prev_c[ba.nprev] = bl.L[i][k];
          ++ba.nprev;
        }
      ba.C = h->dbel_C; ba.c_out = col;
      ba.s = one ? h->dbel_s.ptr : dscratch; ba.sigma2 = one ? h->sigma2 : 1.0;
      if (one) {
        ba.eval = step >= 0 ? 1 : 0;
        if (step >= 0) {
          ba.acq_id = f.acq_id[step]; ba.acq_par = f.acq_par ? f.acq_par[step] : 0.0; ba.plugin = *f.plugin; ba.minimize = f.minimize;
          ba.n_taken = step;  // the winners of steps 0 .. step - 1
          for (int k = 0; k < step; ++k) ba.taken[k] = f.best_idx[k];
        }
        ba.mu = h->dmu_out; ba.acq_out = h->dbel_row; ba.mse_out = dmse_row; ba.blk_val = h->dblk_val; ba.blk_idx = h->dblk_idx;
      }
      for (int64_t c = 0; c < pl.nchunk; ++c) {
        ba.m0 = c * pl.Mc; ba.mcount = std::min<int64_t>(pl.Mc, M - ba.m0); ba.blk_offset = blk_offset;
        if (int rs = believer_chunk(h, pl, ba, active && !chunk_resident)) return rs;
        if (active) chunk_resident = pl.nchunk == 1;
        if (one) blk_offset += (ba.mcount + 63) / 64;  // one record per 64 rows of every chunk
      }
    }
    if (!one) {
      BelieverStep bs;
      memset(&bs, 0, sizeof(bs));
      bs.M = M; bs.m = m; bs.update = col ? 1 : 0; bs.c = col;  // (col null: a guarded pivot, the criterion alone)
      bs.self_row = row; bs.s = h->dbel_s;
      for (int t = 0; t < m; ++t) bs.sigma2[t] = h->sigma2_t[t];
      bs.eval = step >= 0 ? 1 : 0;
      if (step >= 0) {
        bs.n_taken = step;  // the winners of steps 0 .. step - 1
        for (int k = 0; k < step; ++k) bs.taken[k] = f.best_idx[k];
      }
      bs.mu = h->dmu_out; bs.mse_out = dmse_row; bs.blk_val = h->dblk_val; bs.blk_idx = h->dblk_idx;
      if (int rs = timed_span(h, h->bel_timer, st, B_CRITERION, [&] { return f.criterion(bs); })) return rs;
    }
    ++h->bel_passes;
    if (step >= 0)
      HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, one ? blk_offset : nblk_total, nblk_total, 1, h->dbest_val, h->dbest_idx, st));
    return BOGP_OK;
  };

  for (int i = 0; i < P; ++i)
    if ((rc = believe(pending + (size_t)i * d, i == P - 1 ? 0 : -1, true, true, -1))) return rc;

  for (int j = 0; j < q; ++j) {
    // the winner of step j is in dbest_*[0]; its rows in the sweep's own arrays (step 0 without pending points) or in dbel_row
    const bool from_sweep = j == 0 && P == 0;
    int64_t idx = 0;
    HIPCHK(h, hipMemcpyAsync(&f.best_val[j], h->dbest_val, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(&idx, h->dbest_idx, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    for (const StepRows& r : f.rows) {
      const size_t n = (size_t)r.width * M;
      if (r.out) HIPCHK(h, hipMemcpyAsync(r.out + (size_t)j * n, from_sweep ? r.sweep->ptr : h->dbel_row + (size_t)r.at * M, n * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(h, hipStreamSynchronize(st));
    f.best_idx[j] = idx;
    if (idx < 0 || idx >= M) FAIL(h, BOGP_ERR_HIP, "%s: step %d returned row %lld outside [0, %lld)", f.who, j, (long long)idx, (long long)M);
    HIPCHK(h, hipMemcpyAsync(hrow.data(), h->dXs + (size_t)idx * d, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hmu.data(), h->dmu_out + (size_t)idx * m, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (f.best_x) memcpy(f.best_x + (size_t)j * d, hrow.data(), (size_t)d * sizeof(double));
    if (f.best_mu) memcpy(f.best_mu + (size_t)j * m, hmu.data(), (size_t)m * sizeof(double));
    if (one || j < q - 1) f.mean(hmu.data());  // (one target believes the last winner's mean too; no step reads the plugin after it)
    if (j == q - 1) {
      if (f.pivots && (rc = believe(hrow.data(), -1, false, false, idx))) return rc;
      break;
    }
    if ((rc = believe(hrow.data(), j + 1, true, false, idx))) return rc;
  }

  // times of the solves and of the passes (everything is complete: the last step was read back)
  HIPCHK(h, hipStreamSynchronize(st));
  h->bel_solve_ms = h->bel_timer.sum(B_SOLVE); h->bel_corr_ms = h->bel_timer.sum(B_PRODUCER); h->bel_pass_ms = h->bel_timer.sum(B_PASS);
  if (!one) h->bel_criterion_ms = h->bel_timer.sum(B_CRITERION);
  return BOGP_OK;
}

// bogp_believer_ehvi_last, _constrained_last and _ehvi_constrained_last: the spans of the last believer call
int believer_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* criterion_ms, int* n_passes) {
  if (!h) return BOGP_ERR_INVALID;
  if (corr_ms) *corr_ms = h->bel_corr_ms;
  if (solve_ms) *solve_ms = h->bel_solve_ms;
  if (update_ms) *update_ms = h->bel_pass_ms;
  if (criterion_ms) *criterion_ms = h->bel_criterion_ms;
  if (n_passes) *n_passes = h->bel_passes;
  return BOGP_OK;
}

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
  if (int ec = check_criteria(h, q, acq_id, acq_par)) return ec;
  if (q > h->M) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: q = %d proposals from %lld candidates (every step takes a row no step before it took)", q, (long long)h->M);
  for (size_t i = 0; i < (size_t)n_pending * h->d; ++i)
    if (!std::isfinite(pending[i])) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_believer: pending entry %zu is not finite", i);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: constant trend basis only (the committed basis has %d columns)", h->p);
  if (h->n_t != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: one target only (the committed model has %d): EHVI batches are bogp_sweep_believer_ehvi", h->n_t);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: a lift is set (bogp_lift_set): call bogp_lift_clear first");
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_sweep_believer: runs on one rank (the communicator has %d)", h->comm_world);
  HIPCHK(h, hipSetDevice(h->device));
  invalidate_sweep_results(h);  // dbest_* are overwritten

  // ---- pass 0: the plain sweep; with pending points only the moments (step 0 is evaluated behind the last pending point)
  SweepRequest rq;
  rq.want_out = true; rq.minimize = minimize;
  if (n_pending == 0) { rq.q = 1; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin; rq.want_acq_out = true; }
  int rc = run_sweep(h, rq);
  if (rc) return rc;
  if ((rc = candidates_ready(h))) return rc;

  double plug = plugin;
  BelieverFamily f;
  f.who = "bogp_sweep_believer";
  f.acq_id = acq_id; f.acq_par = acq_par; f.minimize = minimize; f.plugin = &plug;
  f.best_val = best_val; f.best_idx = best_idx; f.best_x = best_x; f.pivots = pivots;
  f.rows[0] = {acq_out, &h->dacq_out, 0, 1};
  f.rows[1] = {mse_out, &h->dmse_out, 1, 1};
  f.mean = [&](const double* mu) {
    if (!believe_plugin) return;
    const double y_hat = minimize ? mu[0] : -1 * mu[0];  // the plugin arrives in the criterion's own sign (already negated when maximising)
    if (y_hat < plug) plug = y_hat;
  };
  return believer_run(h, f, q, pending, n_pending);
}

extern "C" int bogp_believer_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* believer_ms, int* n_passes) {
  if (!h) return BOGP_ERR_INVALID;
  if (corr_ms) *corr_ms = h->bel_corr_ms;
  if (solve_ms) *solve_ms = h->bel_solve_ms;
  if (believer_ms) *believer_ms = h->bel_pass_ms;
  if (n_passes) *n_passes = h->bel_passes;
  return BOGP_OK;
}

// ---- believer batches for EHVI: bogp_sweep_believer_ehvi ---------------------------------------------------------------------------
// k_believer_ehvi (kernels_believer_ehvi.hip) takes sigma2_k c^2 off every target's MSE and evaluates EHVI.  The believed mean mu(p) is
// an m-vector that joins the front, so the cells are rebuilt on the host between the steps (bogp_ehvi_grid_cells' decomposition).
namespace {

// pareto.pareto_front: the rows no other row dominates (of identical rows the first) that lie strictly above r in every objective
std::vector<double> pareto_front_rows(int m, int64_t n, const double* Y, const double* r) {
  std::vector<char> keep((size_t)n, 1);
  for (int64_t i = 0; i < n; ++i) {
    const double* yi = Y + (size_t)i * m;
    for (int64_t j = 0; j < n && keep[i]; ++j) {
      const double* yj = Y + (size_t)j * m;
      bool ge = true, gt = false;
      for (int k = 0; k < m; ++k) {
        ge = ge && yj[k] >= yi[k];
        gt = gt || yj[k] > yi[k];
      }
      if (ge && gt) keep[i] = 0;
    }
    for (int64_t j = 0; j < i && keep[i]; ++j)
      if (keep[j] && std::equal(yi, yi + m, Y + (size_t)j * m)) keep[i] = 0;
  }
  std::vector<double> P;
  for (int64_t i = 0; i < n; ++i) {
    if (!keep[i]) continue;
    const double* yi = Y + (size_t)i * m;
    bool above = true;
    for (int k = 0; k < m; ++k) above = above && yi[k] > r[k];
    if (above) P.insert(P.end(), yi, yi + m);
  }
  return P;
}

// pareto.hypercell_bounds on a front P (np rows): the grid's edges along the first m - 1 axes and the cell count, -1 past `limit`
int64_t grid_edges(int m, const std::vector<double>& P, const double* r, int64_t limit, std::vector<std::vector<double>>& edges) {
  const size_t np = P.size() / m;
  edges.assign(m - 1, {});
  int64_t count = 1;
  for (int k = 0; k < m - 1; ++k) {
    std::vector<double> v(np);
    for (size_t i = 0; i < np; ++i) v[i] = P[i * m + k];
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    edges[k].push_back(r[k]);
    edges[k].insert(edges[k].end(), v.begin(), v.end());
    edges[k].push_back(INFINITY);
    if (count >= 0) {
      count *= (int64_t)v.size() + 1;  // (both factors at most 2^31 here: no wrap-around before the check)
      if (count > limit) count = -1;
    }
  }
  return count;
}

// the exact count of a grid past the limit, for the message (saturates at INT64_MAX)
long long grid_count_saturated(const std::vector<std::vector<double>>& edges) {
  long long c = 1;
  for (const auto& e : edges) {
    const long long f = (long long)e.size() - 1;
    c = c > INT64_MAX / f ? INT64_MAX : c * f;
  }
  return c;
}

// the cells in itertools.product order (last grid axis fastest): lower / upper are count x m
void grid_fill(int m, const std::vector<double>& P, const double* r, const std::vector<std::vector<double>>& edges, int64_t count,
               double* lower, double* upper) {
  const size_t np = P.size() / m;
  std::vector<size_t> ix(m - 1, 0);
  for (int64_t c = 0; c < count; ++c) {
    double* lo = lower + (size_t)c * m;
    double* hi = upper + (size_t)c * m;
    for (int k = 0; k < m - 1; ++k) {
      lo[k] = edges[k][ix[k]];
      hi[k] = edges[k][ix[k] + 1];
    }
    double last = r[m - 1];
    for (size_t i = 0; i < np; ++i) {  // the front points that cover the whole column: the largest last coordinate (every one is > r)
      bool cover = true;
      for (int k = 0; k < m - 1; ++k) cover = cover && P[i * m + k] >= hi[k];
      if (cover && P[i * m + m - 1] > last) last = P[i * m + m - 1];
    }
    lo[m - 1] = last;
    hi[m - 1] = INFINITY;
    for (int k = m - 2; k >= 0; --k) {
      if (++ix[k] + 1 < edges[k].size()) break;
      ix[k] = 0;
    }
  }
}

}  // namespace

extern "C" int bogp_ehvi_grid_cells(int m, int n, const double* Y, const double* ref_point, double* lower, double* upper, int64_t cap) {
  if (m < 2 || m > BOGP_MAX_TARGETS || n < 0 || !ref_point || (n > 0 && !Y) || (!lower != !upper)) return BOGP_ERR_INVALID;
  for (int k = 0; k < m; ++k)
    if (!std::isfinite(ref_point[k])) return BOGP_ERR_INVALID;
  for (size_t i = 0; i < (size_t)n * m; ++i)
    if (!std::isfinite(Y[i])) return BOGP_ERR_INVALID;
  const std::vector<double> P = pareto_front_rows(m, n, Y, ref_point);
  std::vector<std::vector<double>> edges;
  const int64_t count = grid_edges(m, P, ref_point, BOGP_MAX_EHVI_CELLS, edges);
  if (count < 0) return BOGP_ERR_INVALID;
  if (!lower) return (int)count;
  if (count > cap) return BOGP_ERR_INVALID;  // (checked before anything is written)
  grid_fill(m, P, ref_point, edges, count, lower, upper);
  return (int)count;
}

extern "C" int bogp_sweep_believer_ehvi(bogp_handle* h, int m, int q, const double* ref_point, const double* front, int n_front,
                                        int believe_front, const double* pending, int n_pending, double* best_val, int64_t* best_idx,
                                        double* best_x, double* best_mu, double* pivots, int* n_cells, double* ehvi_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_believer_ehvi";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior correlation to condition on", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  if (m != h->n_t) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d but the committed model has %d target(s)", who, m, h->n_t);
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d outside [2, %d]", who, m, BOGP_MAX_TARGETS);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  if (q < 1 || n_pending < 0 || q + n_pending > BOGP_MAX_BELIEVED)
    FAIL(h, BOGP_ERR_INVALID, "%s: q = %d, n_pending = %d: q >= 1 and q + n_pending <= %d", who, q, n_pending, BOGP_MAX_BELIEVED);
  if (q > h->M) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d proposals from %lld candidates (every step takes a row no step before it took)", who, q, (long long)h->M);
  if (!ref_point || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: ref_point, best_val and best_idx must be non-null", who);
  if (n_front < 0 || (n_front > 0 && !front)) FAIL(h, BOGP_ERR_INVALID, "%s: n_front = %d and front is %s", who, n_front, front ? "given" : "null");
  if (n_pending > 0 && !pending) FAIL(h, BOGP_ERR_INVALID, "%s: n_pending = %d but pending is null", who, n_pending);
  const int d = h->d;
  for (int k = 0; k < m; ++k)
    if (!std::isfinite(ref_point[k])) FAIL(h, BOGP_ERR_INVALID, "%s: ref_point entry %d is not finite", who, k);
  for (size_t i = 0; i < (size_t)n_front * m; ++i)
    if (!std::isfinite(front[i])) FAIL(h, BOGP_ERR_INVALID, "%s: front entry %zu is not finite", who, i);
  for (size_t i = 0; i < (size_t)n_pending * d; ++i)
    if (!std::isfinite(pending[i])) FAIL(h, BOGP_ERR_INVALID, "%s: pending entry %zu is not finite", who, i);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  const int P = n_pending;

  // ---- the front and its cells (host): F_0 now, one believed mean more per step when believe_front is set
  std::vector<double> F = pareto_front_rows(m, n_front, front, ref_point);
  std::vector<std::vector<double>> edges;
  std::vector<double> cells;  // [lower C x m | upper C x m] of the step evaluated next
  int C = 0;
  auto build_cells = [&](int step) -> int {
    const int64_t count = grid_edges(m, F, ref_point, BOGP_MAX_EHVI_CELLS, edges);
    if (count < 0)
      FAIL(h, BOGP_ERR_INVALID, "%s: step %d: the front of %zu points in %d objectives gives %lld cells (more than %d)", who, step,
           F.size() / m, m, grid_count_saturated(edges), BOGP_MAX_EHVI_CELLS);
    C = (int)count;
    cells.resize(2 * (size_t)C * m);
    grid_fill(m, F, ref_point, edges, count, cells.data(), cells.data() + (size_t)C * m);
    return BOGP_OK;
  };
  int rc;
  if ((rc = build_cells(0))) return rc;  // before any device work (with pending points: the cells of F_0, which step 0 extends)

  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  auto upload_cells = [&]() -> int {  // in stream order, before the pass that reads them; `cells` stays as it is until that pass is complete
    const size_t nb = (size_t)C * m;
    if (int e = h->dehvi_cells.ensure(h, std::max<size_t>(2 * nb, 2))) return e;  // (allocated for a pass over no cells too)
    return stage_ehvi_cells(h, cells.data(), cells.data() + nb, nb, st);
  };

  // ---- pass 0: bogp_sweep_ehvi's sweep; with pending points over no cells, for the moments only
  const int C0 = P == 0 ? C : 0;
  if (P > 0) C = 0;
  if ((rc = upload_cells())) return rc;
  EhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  multi_target_model(h, ea);
  ea.C = C0; ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + (size_t)C0 * m;
  invalidate_sweep_results(h);  // dbest_* are overwritten
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  SweepRequest rq;
  rq.want_out = true; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0; rq.eh = &ea;
  if ((rc = run_sweep(h, rq))) return rc;
  if ((rc = candidates_ready(h))) return rc;
  if (P == 0 && n_cells) n_cells[0] = C0;

  BelieverFamily f;
  f.who = who; f.m = m; f.lead = 2;
  f.best_val = best_val; f.best_idx = best_idx; f.best_x = best_x; f.best_mu = best_mu; f.pivots = pivots;
  f.rows[0] = {ehvi_out, &h->dacq_out, 0, 1};
  f.rows[1] = {mse_out, &h->dmse_out, 2, m};
  f.mean = [&](const double* mu) {  // F <- pareto_front(F u {mu})
    if (!believe_front) return;
    F.insert(F.end(), mu, mu + m);
    F = pareto_front_rows(m, (int64_t)(F.size() / m), F.data(), ref_point);
  };
  f.step_begin = [&](int step) -> int {  // the step's cells are those of the front as it stands here
    if (int rs = build_cells(step)) return rs;
    if (int rs = upload_cells()) return rs;
    if (n_cells) n_cells[step] = C;
    return BOGP_OK;
  };
  f.criterion = [&](const BelieverStep& bs) {
    BelieverEhviArgs be;
    memset(&be, 0, sizeof(be));
    be.M = bs.M; be.m = bs.m; be.update = bs.update; be.c = bs.c; be.self_row = bs.self_row; be.s = bs.s;  // (its own field order)
    memcpy(be.sigma2, bs.sigma2, sizeof(be.sigma2));
    be.eval = bs.eval; be.n_taken = bs.n_taken;
    memcpy(be.taken, bs.taken, sizeof(be.taken));
    be.mu = bs.mu; be.mse_out = bs.mse_out; be.blk_val = bs.blk_val; be.blk_idx = bs.blk_idx;
    if (bs.eval) { be.lower = h->dehvi_cells; be.upper = h->dehvi_cells + (size_t)C * m; be.C = C; }
    be.ehvi_out = h->dbel_row;
    return launch_believer_ehvi(be, st);
  };
  return believer_run(h, f, q, pending, P);
}

extern "C" int bogp_believer_ehvi_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* ehvi_ms, int* n_passes) {
  return believer_last(h, corr_ms, solve_ms, update_ms, ehvi_ms, n_passes);
}

// ---- believer batches under modelled constraints: bogp_sweep_believer_constrained --------------------------------------------------
// Pass 0 is the constrained sweep (k_constrained) with criterion 0; k_believer_constrained (kernels_believer_constrained.hip) takes
// sigma2_k c^2 off every target's MSE and evaluates the step's criterion: target 0 the objective, the others constraints.  The plugin
// follows the believed points that are feasible by belief; the criteria, the bounds, the hyper-parameters and sigma2_k stay fixed.
extern "C" int bogp_sweep_believer_constrained(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                                               int believe_plugin, int n_con, const double* lo, const double* hi, const double* pending,
                                               int n_pending, double* best_val, int64_t* best_idx, double* best_x, double* best_mu,
                                               double* pivots, double* plugin_out, double* acq_out, double* pof_out, double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_believer_constrained";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior correlation to condition on", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  if (q < 1 || n_pending < 0 || q + n_pending > BOGP_MAX_BELIEVED)
    FAIL(h, BOGP_ERR_INVALID, "%s: q = %d, n_pending = %d: q >= 1 and q + n_pending <= %d", who, q, n_pending, BOGP_MAX_BELIEVED);
  if (q > h->M) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d proposals from %lld candidates (every step takes a row no step before it took)", who, q, (long long)h->M);
  if (!acq_id || !lo || !hi || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: acq_id, lo, hi, best_val and best_idx must be non-null", who);
  if (n_pending > 0 && !pending) FAIL(h, BOGP_ERR_INVALID, "%s: n_pending = %d but pending is null", who, n_pending);
  int rc = check_constrained_request(h, who, q, acq_id, acq_par, n_con, lo, hi);
  if (rc) return rc;
  const int m = h->n_t;
  for (size_t i = 0; i < (size_t)n_pending * h->d; ++i)
    if (!std::isfinite(pending[i])) FAIL(h, BOGP_ERR_INVALID, "%s: pending entry %zu is not finite", who, i);
  const int64_t M = h->M;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;

  // ---- pass 0: bogp_sweep_constrained's sweep with criterion 0; with pending points it serves the moments only
  if ((rc = h->dpof_out.ensure(h, (size_t)M))) return rc;
  ConstrainedArgs ca;
  memset(&ca, 0, sizeof(ca));
  multi_target_model(h, ca);
  for (int j = 0; j < n_con; ++j) { ca.lo[j + 1] = lo[j]; ca.hi[j + 1] = hi[j]; }
  ca.q = 1; ca.acq_id[0] = acq_id[0]; ca.acq_par[0] = acq_par ? acq_par[0] : 0.0;
  ca.plugin = plugin; ca.minimize = minimize; ca.pof_out = h->dpof_out.ptr;
  invalidate_sweep_results(h);  // dbest_* are overwritten
  SweepRequest rq;
  rq.want_out = true; rq.want_acq_out = true; rq.q = 1; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin; rq.minimize = minimize;
  rq.cn = &ca;
  if ((rc = run_sweep(h, rq))) return rc;
  if ((rc = candidates_ready(h))) return rc;

  double plug = plugin;
  BelieverFamily f;
  f.who = who; f.m = m; f.lead = 3;
  f.best_val = best_val; f.best_idx = best_idx; f.best_x = best_x; f.best_mu = best_mu; f.pivots = pivots;
  f.rows[0] = {acq_out, &h->dacq_out, 0, 1};
  f.rows[1] = {pof_out, &h->dpof_out, 1, 1};
  f.rows[2] = {mse_out, &h->dmse_out, 3, m};
  // a believed point that is feasible by belief -- every constraint's mean inside its interval -- may lower the plugin, which
  // arrives in the criterion's own sign (already negated when maximising); an infeasible one leaves it
  f.mean = [&](const double* mu) {
    if (!believe_plugin) return;
    for (int k = 1; k < m; ++k)
      if (!(lo[k - 1] <= mu[k] && mu[k] <= hi[k - 1])) return;
    const double y_hat = minimize ? mu[0] : -1 * mu[0];
    if (y_hat < plug) plug = y_hat;
  };
  f.criterion = [&](const BelieverStep& bs) {
    BelieverConstrainedArgs bc;
    memset(&bc, 0, sizeof(bc));
    bc.step = bs;
    for (int t = 0; t < m; ++t) { bc.lo[t] = ca.lo[t]; bc.hi[t] = ca.hi[t]; }
    if (bs.eval) {
      const int step = bs.n_taken;
      bc.acq_id = acq_id[step]; bc.acq_par = acq_par ? acq_par[step] : 0.0; bc.plugin = plug; bc.minimize = minimize;
      if (plugin_out) plugin_out[step] = plug;
    }
    bc.acq_out = h->dbel_row; bc.pof_out = h->dbel_row + M;
    return launch_believer_constrained(bc, st);
  };
  if (n_pending == 0 && plugin_out) plugin_out[0] = plugin;
  return believer_run(h, f, q, pending, n_pending);
}

extern "C" int bogp_believer_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* criterion_ms,
                                              int* n_passes) {
  return believer_last(h, corr_ms, solve_ms, update_ms, criterion_ms, n_passes);
}

// ---- believer batches for constrained EHVI: bogp_sweep_believer_ehvi_constrained ---------------------------------------------------
// Pass 0 is the constrained EHVI sweep (k_ehvi_constrained); k_believer_ehvi_constrained (kernels_believer_ehvi_constrained.hip) takes
// sigma2_k c^2 off every target's MSE and evaluates EHVI of the objectives times the constraints' feasibility.  A believed mean is the
// full (m_obj + n_con)-vector: its objective part joins the feasible front if and only if every constraint mean lies in its closed
// interval -- the test bogp_sweep_believer_constrained uses for the plugin; a point infeasible by belief conditions the variances only.
// A feasibility-only call (no feasible observation: C = 0, the probability of feasibility alone) stays so for all q steps.
extern "C" int bogp_sweep_believer_ehvi_constrained(bogp_handle* h, int m_obj, int q, const double* ref_point, const double* front, int n_front,
                                                    int feasibility_only, int believe_front, int n_con, const double* lo, const double* hi,
                                                    const double* pending, int n_pending, double* best_val, int64_t* best_idx, double* best_x,
                                                    double* best_mu, double* pivots, int* n_cells, double* val_out, double* pof_out,
                                                    double* mse_out) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_sweep_believer_ehvi_constrained";
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no posterior correlation to condition on", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: no candidates: call bogp_candidates_upload/bind first", who);
  if (h->lift_D > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: a lift is set (bogp_lift_set): call bogp_lift_clear first", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: constant trend basis only (the committed basis has %d columns)", who, h->p);
  if (h->comm_world > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: runs on one rank (the communicator has %d)", who, h->comm_world);
  const int m = h->n_t;
  if (m_obj < 2) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj = %d objectives; EHVI needs at least 2", who, m_obj);
  if (n_con < 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d constraints; without one this is bogp_sweep_believer_ehvi", who, n_con);
  if (m > BOGP_MAX_TARGETS || m_obj + n_con != m) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj + n_con = %d + %d but the committed model has %d targets (at most %d)", who, m_obj, n_con, m, BOGP_MAX_TARGETS);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  if (q < 1 || n_pending < 0 || q + n_pending > BOGP_MAX_BELIEVED)
    FAIL(h, BOGP_ERR_INVALID, "%s: q = %d, n_pending = %d: q >= 1 and q + n_pending <= %d", who, q, n_pending, BOGP_MAX_BELIEVED);
  if (q > h->M) FAIL(h, BOGP_ERR_INVALID, "%s: q = %d proposals from %lld candidates (every step takes a row no step before it took)", who, q, (long long)h->M);
  if (!ref_point || !lo || !hi || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "%s: ref_point, lo, hi, best_val and best_idx must be non-null", who);
  if (n_front < 0 || (n_front > 0 && !front)) FAIL(h, BOGP_ERR_INVALID, "%s: n_front = %d and front is %s", who, n_front, front ? "given" : "null");
  if (n_pending > 0 && !pending) FAIL(h, BOGP_ERR_INVALID, "%s: n_pending = %d but pending is null", who, n_pending);
  if (feasibility_only && n_front > 0) FAIL(h, BOGP_ERR_INVALID, "%s: feasibility_only means no feasible observation, but n_front = %d", who, n_front);
  const int d = h->d;
  for (int k = 0; k < m_obj; ++k)
    if (!std::isfinite(ref_point[k])) FAIL(h, BOGP_ERR_INVALID, "%s: ref_point entry %d is not finite", who, k);
  for (size_t i = 0; i < (size_t)n_front * m_obj; ++i)
    if (!std::isfinite(front[i])) FAIL(h, BOGP_ERR_INVALID, "%s: front entry %zu is not finite", who, i);
  for (size_t i = 0; i < (size_t)n_pending * d; ++i)
    if (!std::isfinite(pending[i])) FAIL(h, BOGP_ERR_INVALID, "%s: pending entry %zu is not finite", who, i);
  int rc;
  if ((rc = check_constraint_bounds(h, who, n_con, lo, hi))) return rc;
  const int64_t M = h->M;
  const int P = n_pending;

  // ---- the feasible front and its cells (host): F_0 now, one believed mean more per step where it is feasible by belief
  std::vector<double> F = pareto_front_rows(m_obj, n_front, front, ref_point);
  std::vector<std::vector<double>> edges;
  std::vector<double> cells;  // [lower C x m_obj | upper C x m_obj] of the step evaluated next
  int C = 0;
  auto build_cells = [&](int step) -> int {
    if (feasibility_only) return BOGP_OK;  // (C stays 0: no cells in any step)
    const int64_t count = grid_edges(m_obj, F, ref_point, BOGP_MAX_EHVI_CELLS, edges);
    if (count < 0)
      FAIL(h, BOGP_ERR_INVALID, "%s: step %d: the front of %zu points in %d objectives gives %lld cells (more than %d)", who, step,
           F.size() / m_obj, m_obj, grid_count_saturated(edges), BOGP_MAX_EHVI_CELLS);
    C = (int)count;
    cells.resize(2 * (size_t)C * m_obj);
    grid_fill(m_obj, F, ref_point, edges, count, cells.data(), cells.data() + (size_t)C * m_obj);
    return BOGP_OK;
  };
  if ((rc = build_cells(0))) return rc;  // before any device work (with pending points: the cells of F_0, which step 0 extends)

  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  auto upload_cells = [&]() -> int {  // in stream order, before the pass that reads them; `cells` stays as it is until that pass is complete
    const size_t nb = (size_t)C * m_obj;
    if (int e = h->dehvi_cells.ensure(h, std::max<size_t>(2 * nb, 2))) return e;  // (allocated for a pass over no cells too)
    return stage_ehvi_cells(h, cells.data(), cells.data() + nb, nb, st);
  };

  // ---- pass 0: bogp_sweep_ehvi_constrained's sweep; with pending points over no cells, for the moments only
  const int C0 = P == 0 ? C : 0;
  if (P > 0) C = 0;
  if ((rc = upload_cells())) return rc;
  if ((rc = h->dpof_out.ensure(h, (size_t)M))) return rc;
  ConstrainedEhviArgs ea;
  memset(&ea, 0, sizeof(ea));
  ea.gamma = h->dgamma_base; ea.ld_gamma = h->Np; ea.N = h->N; ea.m = m; ea.m_obj = m_obj; ea.C = C0;
  for (int t = 0; t < m; ++t) ea.sigma2[t] = h->sigma2_t[t];
  for (int j = 0; j < n_con; ++j) { ea.lo[j] = lo[j]; ea.hi[j] = hi[j]; }
  if (C0 > 0) { ea.lower = h->dehvi_cells; ea.upper = h->dehvi_cells + (size_t)C0 * m_obj; }
  ea.pof_out = h->dpof_out.ptr;
  invalidate_sweep_results(h);  // dbest_* are overwritten
  const int one_id = BOGP_ACQ_EI;  // (q = 1 sizes the chunk loop's block records; the id itself is not evaluated)
  SweepRequest rq;
  rq.want_out = true; rq.want_acq_out = true; rq.q = 1; rq.acq_id = &one_id; rq.minimize = 0; rq.ec = &ea;
  if ((rc = run_sweep(h, rq))) return rc;
  if ((rc = candidates_ready(h))) return rc;
  if (P == 0 && n_cells) n_cells[0] = C0;

  BelieverFamily f;
  f.who = who; f.m = m; f.lead = 3;
  f.best_val = best_val; f.best_idx = best_idx; f.best_x = best_x; f.best_mu = best_mu; f.pivots = pivots;
  f.rows[0] = {val_out, &h->dacq_out, 0, 1};
  f.rows[1] = {pof_out, &h->dpof_out, 1, 1};
  f.rows[2] = {mse_out, &h->dmse_out, 3, m};
  // a believed point that is feasible by belief -- every constraint's mean inside its closed interval -- joins the front with its
  // objective part, F <- pareto_front(F u {mu_0 .. mu_{m_obj-1}}); an infeasible one leaves it
  f.mean = [&](const double* mu) {
    if (!believe_front || feasibility_only) return;
    for (int j = 0; j < n_con; ++j)
      if (!(lo[j] <= mu[m_obj + j] && mu[m_obj + j] <= hi[j])) return;
    F.insert(F.end(), mu, mu + m_obj);
    F = pareto_front_rows(m_obj, (int64_t)(F.size() / m_obj), F.data(), ref_point);
  };
  f.step_begin = [&](int step) -> int {  // the step's cells are those of the feasible front as it stands here
    if (int rs = build_cells(step)) return rs;
    if (int rs = upload_cells()) return rs;
    if (n_cells) n_cells[step] = C;
    return BOGP_OK;
  };
  f.criterion = [&](const BelieverStep& bs) {
    BelieverEhviConstrainedArgs be;
    memset(&be, 0, sizeof(be));
    be.step = bs; be.m_obj = m_obj;
    for (int j = 0; j < n_con; ++j) { be.lo[j] = lo[j]; be.hi[j] = hi[j]; }
    if (bs.eval) { be.lower = h->dehvi_cells; be.upper = h->dehvi_cells + (size_t)C * m_obj; be.C = C; }
    be.val_out = h->dbel_row; be.pof_out = h->dbel_row + M;
    return launch_believer_ehvi_constrained(be, st);
  };
  return believer_run(h, f, q, pending, P);
}

extern "C" int bogp_believer_ehvi_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* criterion_ms,
                                                   int* n_passes) {
  return believer_last(h, corr_ms, solve_ms, update_ms, criterion_ms, n_passes);
}
