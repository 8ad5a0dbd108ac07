// bogp_point.hip -- C ABI of the one-point / B-point consumption path (kernels_point.hip): bogp_point_eval,
// bogp_point_eval_batch, bogp_gradient_batch, bogp_polish, and of its multi-objective finish (kernels_point_ehvi.hip):
// bogp_point_eval_ehvi, bogp_polish_ehvi, and of its feasibility-weighted finish (kernels_point_constrained.hip):
// bogp_point_eval_constrained, bogp_polish_constrained, and of the product of the two (kernels_point_ehvi_constrained.hip):
// bogp_point_eval_ehvi_constrained, bogp_polish_ehvi_constrained.  See include/bogp.h for the contracts.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bogp_handle.h"

using namespace bogp;

namespace {

struct PointPlan {
  int NC, npass, Npp, nRB, Nr32, rec_stride, rb, nsplit;
};

PointPlan plan_of(const bogp_handle* h, int B, int q, bool want_dacq) {
  PointPlan p;
  point_tri_geometry(h->N, h->d, B, &p.rb, &p.nsplit);
  p.NC = point_columns_per_pass(h->d);
  p.npass = point_passes(h->d);
  p.Npp = h->ldr;                         // rows of the right-hand sides (zero beyond N)
  p.nRB = (h->N + p.rb - 1) / p.rb;       // row blocks of V (rows beyond N are identity padding: C = rhs = 0)
  p.Nr32 = (h->N + 31) / 32 * 32;         // <= Np: gamma / w are zero padded up to there
  p.rec_stride = 2 + q + 2 * h->d + (want_dacq ? q * h->d : 0);
  return p;
}

int check_common(bogp_handle* h, const char* who, int q, const int* acq_id, const double* acq_par) {
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model", who);
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP || h->kernel == BOGP_KERNEL_MATERN_NU)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the cubic correlation has no input-derivative (corr_dx leaves it undefined in the reference, gpr.py:655-658)", who);
  if (h->p > 1 && h->trend != BOGP_TREND_LINEAR)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the quadratic trend has no Jacobian in the reference either (trend.py:138-139)", who);
  if (h->n_t > 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: one target (several: bogp_predict + bogp_gradient per target)", who);
  if (h->d > BOGP_POINT_MAX_D) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: at most %d input dimensions", who, BOGP_POINT_MAX_D);
  if (q < 0 || q > BOGP_MAX_Q || (q > 0 && !acq_id)) FAIL(h, BOGP_ERR_INVALID, "%s: 0 <= q <= %d with non-null acq_id", who, BOGP_MAX_Q);
  for (int i = 0; i < q; ++i) {
    if (acq_id[i] < 0 || acq_id[i] > 3) FAIL(h, BOGP_ERR_INVALID, "unknown acquisition id %d", acq_id[i]);
    const bool zero_ok = acq_id[i] == BOGP_ACQ_EPSILON_PI;
    if (acq_id[i] != BOGP_ACQ_EI && (!acq_par || !(acq_par[i] > 0 || (zero_ok && acq_par[i] == 0))))
      FAIL(h, BOGP_ERR_INVALID, "acquisition parameter %d must be > 0 (the reference asserts alpha/epsilon/t > 0)", i);
  }
  return BOGP_OK;
}

// arrival tickets: a new block is zeroed
int ensure_tickets(bogp_handle* h, DevBuf<unsigned int>& c, size_t n) {
  if (c.cap >= n && c) return BOGP_OK;
  const int e = c.ensure(h, n);
  if (e) return e;
  HIPCHK(h, hipMemsetAsync(c, 0, n * sizeof(unsigned int), h->stream));
  return BOGP_OK;
}
int ensure_counters(bogp_handle* h, size_t n) { return ensure_tickets(h, h->dpt_counter, n); }

// What one evaluation computes at each of its points, whichever entry asks: q criteria and -- want_dacq -- their input gradients behind
// k_point_finish, or the finish of an m-target model in its place (at most one of eh / cn / ec; they hold what that family alone knows:
// cells and targets, or criteria and bounds, or cells and bounds).  The record then keeps k_point_finish's layout for q criteria, which EHVI fills like ONE.
struct PointCall {
  int q;
  const int* acq_id;
  const double* acq_par;  // null: zeros
  double plugin;
  int minimize;
  bool want_dacq;
  const PointEhviArgs* eh;
  const PointConstrainedArgs* cn;
  const PointEhviConstrainedArgs* ec;
  size_t mom_stride;  // doubles per point of the m-target finishes' second block, written behind the B records; 0: not wanted
};

// the EHVI request: a record sized like one criterion's with its gradient (the id itself is not evaluated)
PointCall ehvi_call(const PointEhviArgs* eh, size_t mom_stride) {
  static const int one_id = BOGP_ACQ_EI;
  return PointCall{1, &one_id, nullptr, 0.0, 0, true, eh, nullptr, nullptr, mom_stride};
}
// ... and the constrained-EHVI request, sized the same way
PointCall ehvi_constrained_call(const PointEhviConstrainedArgs* ec, size_t mom_stride) {
  static const int one_id = BOGP_ACQ_EI;
  return PointCall{1, &one_id, nullptr, 0.0, 0, true, nullptr, nullptr, ec, mom_stride};
}

// the criterion block of PointTriArgs, for k_point_finish and its MFMA flavour alike
void fill_criteria(const bogp_handle* h, const PointPlan& pl, const PointCall& c, unsigned long long* done_flag, unsigned long long done_seq,
                   PointTriArgs* a) {
  a->rec_stride = pl.rec_stride; a->q = c.q; a->want_dacq = c.want_dacq ? 1 : 0; a->estimate_trend = h->estimate_trend;
  a->minimize = c.minimize;
  for (int i = 0; i < c.q; ++i) { a->acq_id[i] = c.acq_id[i]; a->acq_par[i] = c.acq_par ? c.acq_par[i] : 0.0; }
  a->plugin = c.plugin; a->beta = h->beta; a->G = h->G; a->ftft = h->ftft; a->sigma2 = h->sigma2;
  a->done_flag = done_flag; a->done_seq = done_seq;
}

// the arguments of an m-target finish: `a` arrives with its family's own fields and leaves with those PointEhviArgs,
// PointConstrainedArgs and PointEhviConstrainedArgs share (the ones point_multi_sums reads, the second block and the done word)
template <class Args>
Args multi_finish_args(const bogp_handle* h, const PointPlan& pl, Args a, int B, size_t mom_stride, double* out, unsigned long long* done_flag,
                       unsigned long long done_seq) {
  a.part = h->dpt_part; a.rhs = h->dpt_rhs; a.gamma = h->dgamma_base; a.ld_gamma = h->Np; a.out = out;
  a.mom = mom_stride ? out + (size_t)B * pl.rec_stride : nullptr; a.mom_stride = (int)mom_stride;
  a.N = h->N; a.Npp = pl.Npp; a.nRB = pl.nRB; a.npass = pl.npass; a.d = h->d; a.rec_stride = pl.rec_stride;
  a.estimate_trend = h->estimate_trend; a.beta = h->beta; a.G = h->G; a.ftft = h->ftft;
  for (int t = 0; t < a.m; ++t) a.sigma2[t] = h->sigma2_t[t];
  a.done_flag = done_flag; a.done_seq = done_seq;
  return a;
}

// queue k_point_rhs + k_point_tri and the finish of `c` for B points; the records land in `out` (device or device-mapped host memory)
int queue_point_eval(bogp_handle* h, const PointPlan& pl, const PointCall& c, const double* dXb, const double* x_host, int B, double* out,
                     unsigned long long* done_flag = nullptr, unsigned long long done_seq = 0) {
  hipStream_t st = h->stream;
  int e;
  // Enough right-hand sides: C = V rhs is the candidate sweep's triangular product -- FP64 MFMA through k_contract16's
  // cross-product epilogue against the packed V of the commit (kernels_point.hip, "MFMA flavour") instead of k_point_tri's
  // FP64-VALU loop.  "Enough" = the (64-column tile, 256-column group of V) workgroups fill the GPU's 512 slots one and a half
  // times: a workgroup of the last group walks all N rows whatever B is (220 us at N = 2048), so below that the VALU path's
  // finer split is faster -- C3: 128 points 515 us (VALU) vs 582 (MFMA); C5: 32 points 6.1 ms vs 3.0, 128 points 24.7 vs 11.0
  // (profiles/r03_point_call_latency.txt).  BOGP_POINT_MFMA_MIN = that workgroup count (default 768; 0 = never).
  const int ncp = point_mfma_columns(h->d);
  const char* e_min = getenv("BOGP_POINT_MFMA_MIN");  // read per call: the tests run both flavours in one process
  const long long mfma_min = e_min ? atoll(e_min) : 768LL;
  if (!c.eh && !c.cn && !c.ec && dXb && ncp > 0 && h->dVp && h->p == 1 && mfma_min > 0 && (((long long)B * ncp + 63) / 64) * ((h->Np + 255) / 256) >= mfma_min) {
    const int Np = h->Np, nJ = (Np + 255) / 256;
    const long long Mc = ((long long)B * ncp + 63) / 64 * 64;
    if ((e = h->drT[0].ensure(h, (size_t)Np * Mc))) return e;
    if ((e = h->dpt_part.ensure(h, (size_t)B * (nJ + 1) * 2 * ncp))) return e;
    PointRhsArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.X = h->dX; ra.theta = h->dtheta; ra.Xb = dXb; ra.N = h->N; ra.d = h->d;
    HIPCHK(h, launch_point_rhs_T(h->kernel, ra, ncp, h->drT[0], Mc, Np, B, st));
    HIPCHK(h, launch_point_gw(ncp, h->drT[0], Mc, h->dgamma, h->dw, pl.Nr32, B, nJ, h->dpt_part, st));
    ContractArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.rT = h->drT[0]; ka.Vp = h->dVp; ka.ss_part = h->dpt_part; ka.Mc = Mc; ka.nMt = (int)(Mc / 64); ka.nJ = nJ;
    ka.NJ16 = Np / 16; ka.NKP = Np / 8; ka.cross_B = B;
    HIPCHK(h, launch_contract_cross(ka, ncp, st));
    PointTriArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.part = h->dpt_part; fa.out = out; fa.nRB = nJ; fa.npass = 1; fa.d = h->d;
    fill_criteria(h, pl, c, done_flag, done_seq, &fa);
    HIPCHK(h, launch_point_finish_mfma(fa, ncp, B, st));
    return BOGP_OK;
  }
  if ((e = h->dpt_rhs.ensure(h, (size_t)B * pl.npass * pl.Npp * pl.NC))) return e;
  if ((e = h->dpt_part.ensure(h, (size_t)B * pl.npass * (pl.nRB + 1) * 2 * pl.NC))) return e;
  const size_t nslots = (size_t)B * pl.npass * (pl.nRB + 1);
  if ((e = ensure_counters(h, (size_t)std::max(B, 64) + 1))) return e;
  if (pl.nsplit > 1) {
    if ((e = h->dpt_split.ensure(h, nslots * pl.nsplit * pl.rb * pl.NC))) return e;
    if ((e = ensure_tickets(h, h->dpt_splitc, nslots))) return e;
  }
  PointRhsArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.X = h->dX; ra.theta = h->dtheta; ra.Xb = dXb; ra.rhs = h->dpt_rhs;
  ra.N = h->N; ra.d = h->d; ra.Npp = pl.Npp; ra.npass = pl.npass;
  if (!dXb) memcpy(ra.x, x_host, (size_t)h->d * sizeof(double));
  HIPCHK(h, launch_point_rhs(h->kernel, ra, B, st));
  const double* trend_rec = nullptr;
  if (h->p > 1) {  // linear basis: (Ft^T L^-1) [r | dr/dx] and the trend's share of mu, MSE and their gradients (kernels_point.hip)
    if ((e = h->dpt_tw.ensure(h, (size_t)B * pl.npass * h->p * pl.NC))) return e;
    if ((e = h->dpt_trec.ensure(h, (size_t)B * (2 + 2 * h->d)))) return e;
    HIPCHK(h, launch_point_trend(ra, h->dWp, h->Np, h->p, h->dbetav, h->dSinv, h->estimate_trend, h->dpt_tw, h->dpt_trec, B, st));
    trend_rec = h->dpt_trec;
  }
  PointTriArgs ta;
  memset(&ta, 0, sizeof(ta));
  ta.V = h->dV; ta.gamma = h->dgamma; ta.wvec = h->dw; ta.rhs = h->dpt_rhs; ta.part = h->dpt_part;
  ta.counter = h->dpt_counter; ta.out = out;
  ta.split_scratch = h->dpt_split; ta.split_counter = h->dpt_splitc; ta.rb = pl.rb; ta.nsplit = pl.nsplit;
  ta.ld = h->ldr; ta.Npp = pl.Npp; ta.Nr32 = pl.Nr32; ta.nRB = pl.nRB; ta.npass = pl.npass; ta.d = h->d;
  fill_criteria(h, pl, c, done_flag, done_seq, &ta);
  ta.trend_rec = trend_rec;
  HIPCHK(h, launch_point_tri(ta, B, st, !c.eh && !c.cn && !c.ec));  // an m-target finish takes k_point_finish's place
  if (c.eh) HIPCHK(h, launch_point_ehvi_finish(multi_finish_args(h, pl, *c.eh, B, c.mom_stride, out, done_flag, done_seq), B, st));
  if (c.cn) HIPCHK(h, launch_point_constrained_finish(multi_finish_args(h, pl, *c.cn, B, c.mom_stride, out, done_flag, done_seq), B, st));
  if (c.ec) HIPCHK(h, launch_point_ehvi_constrained_finish(multi_finish_args(h, pl, *c.ec, B, c.mom_stride, out, done_flag, done_seq), B, st));
  return BOGP_OK;
}

// the lock-step polish of B starts with the evaluation of `call` (one criterion and its gradient: q = 1) queued every iteration:
// the loop of bogp_polish, bogp_polish_ehvi, bogp_polish_constrained and bogp_polish_ehvi_constrained
int polish_loop(bogp_handle* h, const char* who, const PointCall& call, const double* X0, int B, const double* lo, const double* hi,
                int max_evals, double pgtol, double factr, double* Xout, double* fout, int* n_evals) {
  int e;
  if (!X0 || !lo || !hi || !Xout || !fout || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null pointer or B <= 0", who);
  const int d = h->d;
  if (max_evals <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: max_evals must be positive", who);
  double wmin = INFINITY;
  for (int k = 0; k < d; ++k) {
    if (!(hi[k] >= lo[k])) FAIL(h, BOGP_ERR_INVALID, "%s: lo[%d] > hi[%d]", who, k, k);
    if (hi[k] > lo[k]) wmin = std::min(wmin, hi[k] - lo[k]);
  }
  if (!std::isfinite(wmin)) wmin = 1.0;
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const PointPlan pl = plan_of(h, B, 1, true);
  const size_t ss = polish_state_doubles(d);
  if ((e = h->dpt_Xb.ensure(h, (size_t)B * d))) return e;
  if ((e = h->dpt_out.ensure(h, (size_t)B * pl.rec_stride))) return e;
  if ((e = h->dpt_state.ensure(h, (size_t)B * ss))) return e;
  if ((e = h->dpt_box.ensure(h, (size_t)2 * d))) return e;
  if ((e = ensure_counters(h, (size_t)std::max(B, 64) + 1))) return e;
  if ((e = h->hpin.ensure(h, std::max<size_t>((size_t)B * (d + 2) + 16, 1024)))) return e;
  unsigned int* dn_done = h->dpt_counter + (h->dpt_counter.cap - 1);
  // starting points clipped into the box (scipy's L-BFGS-B projects x0 the same way)
  std::vector<double> xs((size_t)B * d), box(2 * (size_t)d), st0((size_t)B * ss, 0.0);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < d; ++k) xs[(size_t)b * d + k] = std::min(std::max(X0[(size_t)b * d + k], lo[k]), hi[k]);
  for (int k = 0; k < d; ++k) { box[k] = lo[k]; box[d + k] = hi[k]; }
  for (int b = 0; b < B; ++b) { st0[(size_t)b * ss + 1] = 1.0; st0[(size_t)b * ss + 7] = 1.0; }  // alpha = 1, first = 1
  HIPCHK(h, hipMemcpyAsync(h->dpt_Xb, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(h->dpt_box, box.data(), box.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(h->dpt_state, st0.data(), st0.size() * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(dn_done, 0, sizeof(unsigned int), st));
  PolishArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.state = h->dpt_state; pa.rec = h->dpt_out; pa.Xt = h->dpt_Xb; pa.lo = h->dpt_box; pa.hi = h->dpt_box + d; pa.n_done = dn_done;
  pa.d = d; pa.q = 1; pa.rec_stride = pl.rec_stride; pa.state_stride = (int)ss; pa.max_evals = max_evals;
  pa.pgtol = pgtol; pa.factr_eps = factr * 2.220446049250313e-16; pa.first_step = 0.05 * wmin;
  unsigned int* hdone = (unsigned int*)h->hpin.ptr;
  // every iteration = one batched evaluation of the B trial points + one optimiser step, all queued; the host looks at the
  // count of finished starts every 8 iterations (one 4-byte read-back) to stop early
  int it = 0;
  while (it < max_evals) {
    const int burst = std::min(8, max_evals - it);
    for (int s = 0; s < burst; ++s, ++it) {
      if ((e = queue_point_eval(h, pl, call, h->dpt_Xb, nullptr, B, h->dpt_out))) return e;
      HIPCHK(h, launch_polish_step(pa, B, st));
    }
    HIPCHK(h, hipMemcpyAsync(hdone, dn_done, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (*hdone >= (unsigned int)B) break;
  }
  std::vector<double> fin((size_t)B * ss);
  HIPCHK(h, hipMemcpyAsync(fin.data(), h->dpt_state, fin.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  for (int b = 0; b < B; ++b) {
    const double* s = &fin[(size_t)b * ss];
    fout[b] = s[0];
    if (n_evals) n_evals[b] = (int)s[6];
    memcpy(Xout + (size_t)b * d, s + 8, (size_t)d * sizeof(double));
  }
  return BOGP_OK;
}

// the committed model of an m-target finish: what check_ehvi and check_constrained refuse in the same words, behind their own forest
// and "no committed model" lines
int check_multi_model(bogp_handle* h, const char* who) {
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP || h->kernel == BOGP_KERNEL_MATERN_NU)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the correlation has no input-derivative (corr_dx leaves it undefined in the reference, gpr.py:655-658)", who);
  if (h->p != 1) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: several targets take the constant trend only (gpr.py:787)", who);
  if (h->d > BOGP_POINT_MAX_D) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: at most %d input dimensions", who, BOGP_POINT_MAX_D);
  return BOGP_OK;
}

// what bogp_point_eval_ehvi and bogp_polish_ehvi refuse alike (the cells are checked by ehvi_cells_resident)
int check_ehvi(bogp_handle* h, const char* who, int m) {
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest, which has no input gradient", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model", who);
  if (int e = check_multi_model(h, who)) return e;
  if (m != h->n_t) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d but the committed model has %d targets", who, m, h->n_t);
  if (m < 2 || m > BOGP_MAX_TARGETS) FAIL(h, BOGP_ERR_INVALID, "%s: m = %d outside [2, %d]", who, m, BOGP_MAX_TARGETS);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  return BOGP_OK;
}

// the cells on the device (bogp_sweep_ehvi's rules).  A call whose (m, C, bytes) equal the cells this path left there skips the
// checks and the upload: the BFGS loop makes thousands of one-point calls over the same cells.
int ehvi_cells_resident(bogp_handle* h, const char* who, int m, int C, const double* lower, const double* upper) {
  if (C < 1 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "%s: C = %d cells outside [1, %d]", who, C, BOGP_MAX_EHVI_CELLS);
  if (!lower || !upper) FAIL(h, BOGP_ERR_INVALID, "%s: lower and upper must be non-null", who);
  const size_t nb = (size_t)C * m;
  if (h->dehvi_cells && h->ehvi_host_m == m && h->ehvi_host_C == C && h->h_ehvi_cells.size() == 2 * nb &&
      memcmp(h->h_ehvi_cells.data(), lower, nb * sizeof(double)) == 0 && memcmp(h->h_ehvi_cells.data() + nb, upper, nb * sizeof(double)) == 0)
    return BOGP_OK;
  int e;
  if ((e = check_ehvi_cells(h, who, nb, lower, upper))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  if ((e = stage_ehvi_cells(h, lower, upper, nb, h->stream))) return e;
  h->h_ehvi_cells.assign(lower, lower + nb);
  h->h_ehvi_cells.insert(h->h_ehvi_cells.end(), upper, upper + nb);
  h->ehvi_host_m = m;
  h->ehvi_host_C = C;
  return BOGP_OK;
}

// stage the B rows of Xb, queue the evaluation of `call` and wait for it: afterwards the B records lie at h->hpin, the second blocks
// (call.mom_stride doubles a point) behind them
int point_eval_wait(bogp_handle* h, const PointPlan& pl, const PointCall& call, const double* Xb, int B) {
  hipStream_t st = h->stream;
  const int d = h->d;
  const size_t nrec = (size_t)B * (pl.rec_stride + call.mom_stride);
  int e;
  // the finishing workgroups write straight into pinned host memory: one stream synchronisation, no copy command
  if ((e = h->hpin.ensure(h, std::max<size_t>(nrec + 8, 1024)))) return e;
  const double* dXb = nullptr;
  if (B > 1 || d > BOGP_POINT_ARG_D) {
    if ((e = h->dpt_Xb.ensure(h, (size_t)B * d))) return e;
    HIPCHK(h, hipMemcpyAsync(h->dpt_Xb, Xb, (size_t)B * d * sizeof(double), hipMemcpyHostToDevice, st));
    dXb = h->dpt_Xb;
  }
  // One point (the BFGS loop's call): completion is read off a sequence word the finishing workgroup stores behind the record
  // (pinned memory, system-scope release) -- polling it costs less than a stream synchronisation (profiles/r03_point_call_latency.txt);
  // bounded: after ~2 ms of polling the ordinary synchronisation takes over.
  if (B == 1) {
    volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(h->hpin + nrec);
    const unsigned long long seq = ++h->pt_seq;
    unsigned long long* dflag = reinterpret_cast<unsigned long long*>(h->hpin.dev + nrec);
    if ((e = queue_point_eval(h, pl, call, dXb, Xb, B, h->hpin.dev, dflag, seq))) return e;
    bool seen = false;
    for (int spin = 0; spin < 400000; ++spin) {
      if (*flag == seq) { seen = true; break; }
      __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!seen) HIPCHK(h, hipStreamSynchronize(st));
  } else {
    if ((e = queue_point_eval(h, pl, call, dXb, Xb, B, h->hpin.dev))) return e;
    HIPCHK(h, hipStreamSynchronize(st));
  }
  return BOGP_OK;
}

// The B rows of Xb through point_eval_wait in chunks whose right-hand sides (8 ld NC bytes per point and pass) stay below 256 MB, and
// never more than 4096 points; unpack(row of Xb, its record, its second block) copies a point's results out of the pinned buffer.
template <class Unpack>
int point_eval_chunks(bogp_handle* h, const PointCall& call, const double* Xb, int B, Unpack unpack) {
  const int d = h->d;
  const size_t per_point = (size_t)point_passes(d) * h->ldr * point_columns_per_pass(d) * sizeof(double);
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>(4096, ((size_t)256 << 20) / per_point));
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = std::min(chunk, B - b0);
    const PointPlan pl = plan_of(h, nb, call.q, call.want_dacq);
    const int e = point_eval_wait(h, pl, call, Xb + (size_t)b0 * d, nb);
    if (e) return e;
    const double* mom = h->hpin + (size_t)nb * pl.rec_stride;
    for (int b = 0; b < nb; ++b) unpack((size_t)b0 + b, h->hpin + (size_t)b * pl.rec_stride, mom + (size_t)b * call.mom_stride);
  }
  return BOGP_OK;
}

}  // namespace

namespace bogp {

void ehvi_cells_forget(bogp_handle* h) {
  h->h_ehvi_cells.clear();
  h->ehvi_host_m = h->ehvi_host_C = 0;
}

int check_ehvi_cells(bogp_handle* h, const char* who, size_t nb, const double* lower, const double* upper) {
  for (size_t i = 0; i < nb; ++i) {
    if (!std::isfinite(lower[i])) FAIL(h, BOGP_ERR_INVALID, "%s: lower bound %zu is not finite", who, i);
    if (std::isnan(upper[i])) FAIL(h, BOGP_ERR_INVALID, "%s: upper bound %zu is NaN", who, i);
    if (!(upper[i] >= lower[i])) FAIL(h, BOGP_ERR_INVALID, "%s: upper bound %zu (%g) is below its lower bound (%g)", who, i, upper[i], lower[i]);
  }
  return BOGP_OK;
}

int stage_ehvi_cells(bogp_handle* h, const double* lower, const double* upper, size_t nb, hipStream_t st) {
  ehvi_cells_forget(h);  // (bogp_point_eval_ehvi keeps a host copy of what it left in this buffer)
  if (nb == 0) return BOGP_OK;
  if (int e = h->dehvi_cells.ensure(h, 2 * nb)) return e;
  // (the cells are the kernel's arguments: copied in stream order, before the kernels that read them)
  HIPCHK(h, hipMemcpyAsync(h->dehvi_cells, lower, nb * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(h->dehvi_cells + nb, upper, nb * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipStreamSynchronize(st));  // the caller's arrays are not needed past this call
  return BOGP_OK;
}

int point_eval_host(bogp_handle* h, const char* who, const double* Xb, int B, int q, const int* acq_id, const double* acq_par,
                    double plugin, int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq, double* dacq) {
  int e = check_common(h, who, q, acq_id, acq_par);
  if (e) return e;
  if (!Xb || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null points or B <= 0", who);
  if (q > 0 && !acq && !dacq) FAIL(h, BOGP_ERR_INVALID, "%s: q > 0 needs acq or dacq", who);
  HIPCHK(h, hipSetDevice(h->device));
  const int d = h->d;
  const bool want_dacq = dacq != nullptr && q > 0;
  const PointCall call{q, acq_id, acq_par, plugin, minimize, want_dacq, nullptr, nullptr, nullptr, 0};
  return point_eval_chunks(h, call, Xb, B, [=](size_t b, const double* o, const double*) {
    if (mu) mu[b] = o[0];
    if (mse) mse[b] = o[1];
    if (acq) memcpy(acq + b * q, o + 2, (size_t)q * sizeof(double));
    if (dmu) memcpy(dmu + b * d, o + 2 + q, (size_t)d * sizeof(double));
    if (dmse) memcpy(dmse + b * d, o + 2 + q + d, (size_t)d * sizeof(double));
    if (want_dacq) memcpy(dacq + b * q * d, o + 2 + q + 2 * d, (size_t)q * d * sizeof(double));
  });
}

}  // namespace bogp

extern "C" int bogp_point_eval(bogp_handle* h, const double* x, int q, const int* acq_id, const double* acq_par, double plugin,
                               int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq) {
  if (!h) return BOGP_ERR_INVALID;
  if (!x || !mu || !mse || !dmu || !dmse) FAIL(h, BOGP_ERR_INVALID, "bogp_point_eval: null pointer");
  if (q > 0 && !acq) FAIL(h, BOGP_ERR_INVALID, "bogp_point_eval: q > 0 with a null acq");
  return point_eval_host(h, "bogp_point_eval", x, 1, q, acq_id, acq_par, plugin, minimize, mu, mse, dmu, dmse, acq, nullptr);
}

extern "C" int bogp_point_eval_batch(bogp_handle* h, const double* Xb, int B, int q, const int* acq_id, const double* acq_par,
                                     double plugin, int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq,
                                     double* dacq) {
  if (!h) return BOGP_ERR_INVALID;
  return point_eval_host(h, "bogp_point_eval_batch", Xb, B, q, acq_id, acq_par, plugin, minimize, mu, mse, dmu, dmse, acq, dacq);
}

extern "C" int bogp_gradient_batch(bogp_handle* h, const double* Xb, int B, double* dmu, double* dmse) {
  if (!h) return BOGP_ERR_INVALID;
  if (!Xb || !dmu || !dmse || B <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_gradient_batch: null pointer or B <= 0");
  return point_eval_host(h, "bogp_gradient_batch", Xb, B, 0, nullptr, nullptr, 0.0, 1, nullptr, nullptr, dmu, dmse, nullptr, nullptr);
}

extern "C" int bogp_polish(bogp_handle* h, const double* X0, int B, const double* lo, const double* hi, int acq_id, double acq_par,
                           double plugin, int minimize, int max_evals, double pgtol, double factr, double* Xout, double* fout,
                           int* n_evals) {
  if (!h) return BOGP_ERR_INVALID;
  int e = check_common(h, "bogp_polish", 1, &acq_id, &acq_par);
  if (e) return e;
  const PointCall call{1, &acq_id, &acq_par, plugin, minimize, true, nullptr, nullptr, nullptr, 0};
  return polish_loop(h, "bogp_polish", call, X0, B, lo, hi, max_evals, pgtol, factr, Xout, fout, n_evals);
}

// ---- EHVI and its input gradient at B points of the committed m-target model (kernels_point_ehvi.hip) --------------------------
extern "C" int bogp_point_eval_ehvi(bogp_handle* h, const double* Xb, int B, int m, int C, const double* lower, const double* upper,
                                    double* ehvi, double* dehvi, double* mu, double* mse, double* dmu, double* dmse) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_point_eval_ehvi";
  int e = check_ehvi(h, who, m);
  if (e) return e;
  if (!Xb || !ehvi || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null points, null ehvi or B <= 0", who);
  if ((e = ehvi_cells_resident(h, who, m, C, lower, upper))) return e;
  HIPCHK(h, hipSetDevice(h->device));
  const int d = h->d;
  PointEhviArgs eh;
  memset(&eh, 0, sizeof(eh));
  eh.m = m; eh.C = C; eh.lower = h->dehvi_cells; eh.upper = h->dehvi_cells + (size_t)C * m;
  const bool want_mom = mu || mse || dmu || dmse;
  const size_t md = (size_t)m * d;
  return point_eval_chunks(h, ehvi_call(&eh, want_mom ? 2 * m + 2 * md : 0), Xb, B, [=](size_t b, const double* o, const double* mom) {
    ehvi[b] = o[2];
    if (dehvi) memcpy(dehvi + b * d, o + 3 + 2 * d, (size_t)d * sizeof(double));
    if (!want_mom) return;
    if (mu) memcpy(mu + b * m, mom, (size_t)m * sizeof(double));
    if (mse) memcpy(mse + b * m, mom + m, (size_t)m * sizeof(double));
    if (dmu) memcpy(dmu + b * md, mom + 2 * m, md * sizeof(double));
    if (dmse) memcpy(dmse + b * md, mom + 2 * m + md, md * sizeof(double));
  });
}

extern "C" int bogp_polish_ehvi(bogp_handle* h, const double* X0, int B, const double* lo, const double* hi, int m, int C,
                                const double* lower, const double* upper, int max_evals, double pgtol, double factr, double* Xout,
                                double* fout, int* n_evals) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_polish_ehvi";
  int e = check_ehvi(h, who, m);
  if (e) return e;
  if (!X0 || !lo || !hi || !Xout || !fout || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null pointer or B <= 0", who);
  if ((e = ehvi_cells_resident(h, who, m, C, lower, upper))) return e;
  PointEhviArgs eh;
  memset(&eh, 0, sizeof(eh));
  eh.m = m; eh.C = C; eh.lower = h->dehvi_cells; eh.upper = h->dehvi_cells + (size_t)C * m;
  return polish_loop(h, who, ehvi_call(&eh, 0), X0, B, lo, hi, max_evals, pgtol, factr, Xout, fout, n_evals);
}

// ---- feasibility-weighted criteria and their input gradients at B points of the committed m-target model (kernels_point_constrained.hip) ----
// what bogp_point_eval_constrained and bogp_polish_constrained refuse alike: the model, then what bogp_sweep_constrained refuses too
static int check_constrained(bogp_handle* h, const char* who, int q, const int* acq_id, const double* acq_par, int n_con, const double* lo,
                             const double* hi) {
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest; modelled constraints take a multi-target Gaussian process", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (int e = check_multi_model(h, who)) return e;
  return check_constrained_request(h, who, q, acq_id, acq_par, n_con, lo, hi);
}

static void fill_constrained(const bogp_handle* h, PointConstrainedArgs* cn, int q, const int* acq_id, const double* acq_par, double plugin,
                             int minimize, int n_con, const double* lo, const double* hi) {
  memset(cn, 0, sizeof(*cn));
  cn->m = h->n_t; cn->q = q; cn->plugin = plugin; cn->minimize = minimize;
  for (int c = 0; c < q; ++c) { cn->acq_id[c] = acq_id[c]; cn->acq_par[c] = acq_par ? acq_par[c] : 0.0; }
  for (int j = 0; j < n_con; ++j) { cn->lo[j + 1] = lo[j]; cn->hi[j + 1] = hi[j]; }
}

extern "C" int bogp_point_eval_constrained(bogp_handle* h, const double* Xb, int B, int q, const int* acq_id, const double* acq_par, double plugin,
                                           int minimize, int n_con, const double* lo, const double* hi, double* acq, double* dacq, double* pof,
                                           double* dpof, double* mu, double* mse, double* dmu, double* dmse) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_point_eval_constrained";
  int e = check_constrained(h, who, q, acq_id, acq_par, n_con, lo, hi);
  if (e) return e;
  if (!Xb || !acq || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null points, null acq or B <= 0", who);
  HIPCHK(h, hipSetDevice(h->device));
  const int d = h->d, m = h->n_t;
  PointConstrainedArgs cn;
  fill_constrained(h, &cn, q, acq_id, acq_par, plugin, minimize, n_con, lo, hi);
  const bool want_mom = pof || dpof || mu || mse || dmu || dmse;
  const size_t md = (size_t)m * d;
  const PointCall call{q, cn.acq_id, cn.acq_par, plugin, minimize, true, nullptr, &cn, nullptr, want_mom ? 1 + d + 2 * m + 2 * md : 0};
  return point_eval_chunks(h, call, Xb, B, [=](size_t b, const double* o, const double* mom) {
    memcpy(acq + b * q, o + 2, (size_t)q * sizeof(double));
    if (dacq) memcpy(dacq + b * q * d, o + 2 + q + 2 * d, (size_t)q * d * sizeof(double));
    if (!want_mom) return;
    if (pof) pof[b] = mom[0];
    if (dpof) memcpy(dpof + b * d, mom + 1, (size_t)d * sizeof(double));
    mom += 1 + d;
    if (mu) memcpy(mu + b * m, mom, (size_t)m * sizeof(double));
    if (mse) memcpy(mse + b * m, mom + m, (size_t)m * sizeof(double));
    if (dmu) memcpy(dmu + b * md, mom + 2 * m, md * sizeof(double));
    if (dmse) memcpy(dmse + b * md, mom + 2 * m + md, md * sizeof(double));
  });
}

extern "C" int bogp_polish_constrained(bogp_handle* h, const double* X0, int B, const double* box_lo, const double* box_hi, int acq_id,
                                       double acq_par, double plugin, int minimize, int n_con, const double* lo, const double* hi, int max_evals,
                                       double pgtol, double factr, double* Xout, double* fout, int* n_evals) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_polish_constrained";
  int e = check_constrained(h, who, 1, &acq_id, &acq_par, n_con, lo, hi);
  if (e) return e;
  PointConstrainedArgs cn;
  fill_constrained(h, &cn, 1, &acq_id, &acq_par, plugin, minimize, n_con, lo, hi);
  const PointCall call{1, cn.acq_id, cn.acq_par, plugin, minimize, true, nullptr, &cn, nullptr, 0};
  return polish_loop(h, who, call, X0, B, box_lo, box_hi, max_evals, pgtol, factr, Xout, fout, n_evals);
}

// ---- feasibility-weighted EHVI and its input gradient at B points of the committed (m_obj + n_con)-target model (kernels_point_ehvi_constrained.hip) ----
// what bogp_point_eval_ehvi_constrained and bogp_polish_ehvi_constrained refuse alike, in bogp_sweep_ehvi_constrained's words where it
// refuses the same; then the cells on the device (ehvi_cells_resident with m = m_obj: a repeated call skips check and upload) and the request
static int ehvi_constrained_request(bogp_handle* h, const char* who, int m_obj, int C, const double* lower, const double* upper, int n_con,
                                    const double* lo, const double* hi, PointEhviConstrainedArgs* ec) {
  if (h->forest_T > 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "%s: the handle holds a forest; modelled constraints take a multi-target Gaussian process", who);
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "%s: no committed model: call bogp_commit first", who);
  if (int e = check_multi_model(h, who)) return e;
  const int m = h->n_t;
  if (m_obj < 2) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj = %d objectives; EHVI needs at least 2", who, m_obj);
  if (n_con < 1) FAIL(h, BOGP_ERR_INVALID, "%s: n_con = %d constraints; without one this is the EHVI call", who, n_con);
  if (m > BOGP_MAX_TARGETS || m_obj + n_con != m) FAIL(h, BOGP_ERR_INVALID, "%s: m_obj + n_con = %d + %d but the committed model has %d targets (at most %d)", who, m_obj, n_con, m, BOGP_MAX_TARGETS);
  if (C < 0 || C > BOGP_MAX_EHVI_CELLS) FAIL(h, BOGP_ERR_INVALID, "%s: C = %d cells outside [0, %d]", who, C, BOGP_MAX_EHVI_CELLS);
  if (!lo || !hi) FAIL(h, BOGP_ERR_INVALID, "%s: lo and hi must be non-null", who);
  if ((int)h->sigma2_t.size() < m) FAIL(h, BOGP_ERR_INVALID, "%s: the commit holds %d target variances", who, (int)h->sigma2_t.size());
  for (int j = 0; j < n_con; ++j) {
    if (std::isnan(lo[j]) || std::isnan(hi[j])) FAIL(h, BOGP_ERR_INVALID, "%s: a bound of constraint %d is NaN", who, j);
    if (hi[j] < lo[j]) FAIL(h, BOGP_ERR_INVALID, "%s: the upper bound of constraint %d (%g) is below its lower bound (%g)", who, j, hi[j], lo[j]);
  }
  if (C > 0)
    if (int e = ehvi_cells_resident(h, who, m_obj, C, lower, upper)) return e;
  memset(ec, 0, sizeof(*ec));
  ec->m = m; ec->m_obj = m_obj; ec->C = C;
  if (C > 0) { ec->lower = h->dehvi_cells; ec->upper = h->dehvi_cells + (size_t)C * m_obj; }
  for (int j = 0; j < n_con; ++j) { ec->lo[j] = lo[j]; ec->hi[j] = hi[j]; }
  return BOGP_OK;
}

extern "C" int bogp_point_eval_ehvi_constrained(bogp_handle* h, const double* Xb, int B, int m_obj, int C, const double* lower, const double* upper,
                                                int n_con, const double* lo, const double* hi, double* val, double* dval, double* pof, double* dpof,
                                                double* ehvi, double* dehvi, double* mu, double* mse, double* dmu, double* dmse) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_point_eval_ehvi_constrained";
  if (!Xb || !val || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null points, null val or B <= 0", who);
  PointEhviConstrainedArgs ec;
  int e = ehvi_constrained_request(h, who, m_obj, C, lower, upper, n_con, lo, hi, &ec);
  if (e) return e;
  HIPCHK(h, hipSetDevice(h->device));
  const int d = h->d, m = h->n_t;
  const bool want_mom = pof || dpof || ehvi || dehvi || mu || mse || dmu || dmse;
  const size_t md = (size_t)m * d;
  return point_eval_chunks(h, ehvi_constrained_call(&ec, want_mom ? 2 + 2 * d + 2 * m + 2 * md : 0), Xb, B,
                           [=](size_t b, const double* o, const double* mom) {
    val[b] = o[2];
    if (dval) memcpy(dval + b * d, o + 3 + 2 * d, (size_t)d * sizeof(double));
    if (!want_mom) return;
    if (pof) pof[b] = mom[0];
    if (dpof) memcpy(dpof + b * d, mom + 1, (size_t)d * sizeof(double));
    if (ehvi) ehvi[b] = mom[1 + d];
    if (dehvi) memcpy(dehvi + b * d, mom + 2 + d, (size_t)d * sizeof(double));
    mom += 2 + 2 * d;
    if (mu) memcpy(mu + b * m, mom, (size_t)m * sizeof(double));
    if (mse) memcpy(mse + b * m, mom + m, (size_t)m * sizeof(double));
    if (dmu) memcpy(dmu + b * md, mom + 2 * m, md * sizeof(double));
    if (dmse) memcpy(dmse + b * md, mom + 2 * m + md, md * sizeof(double));
  });
}

extern "C" int bogp_polish_ehvi_constrained(bogp_handle* h, const double* X0, int B, const double* box_lo, const double* box_hi, int m_obj, int C,
                                            const double* lower, const double* upper, int n_con, const double* lo, const double* hi, int max_evals,
                                            double pgtol, double factr, double* Xout, double* fout, int* n_evals) {
  if (!h) return BOGP_ERR_INVALID;
  const char* who = "bogp_polish_ehvi_constrained";
  if (!X0 || !box_lo || !box_hi || !Xout || !fout || B <= 0) FAIL(h, BOGP_ERR_INVALID, "%s: null pointer or B <= 0", who);
  PointEhviConstrainedArgs ec;
  int e = ehvi_constrained_request(h, who, m_obj, C, lower, upper, n_con, lo, hi, &ec);
  if (e) return e;
  return polish_loop(h, who, ehvi_constrained_call(&ec, 0), X0, B, box_lo, box_hi, max_evals, pgtol, factr, Xout, fout, n_evals);
}
