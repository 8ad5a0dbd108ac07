// bogp_api_sweep.hip -- the C ABI of libbogp.so (include/bogp.h), part 3 of 3: candidate sets (upload, lazy upload, device generators),
// the posterior / acquisition sweep, top-k, the one-point gradient / Hessian calls, timing and the debug / self-test exports.
// Part 1 = bogp_api.hip, part 2 = bogp_api_fit.hip.
// run_sweep dispatches a SweepRequest to sweep_small_batch (M <= 32), sweep_one_launch (Np <= 512, everything fused), sweep_chunks (producer
// -> contraction -> criteria per chunk; sweep_pruned_chunk, sweep_trend_chunk) or sweep_onepass (the one-pass pruned flow).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_device.h"
#include "bogp_handle.h"
#include "bogp_internal.h"
#include "bogp_fit.h"

using namespace bogp;

// ------------------------------------------------------------------------------------------------------
// candidates
// ------------------------------------------------------------------------------------------------------
// The winners a sweep left on the device (dbest_* / dtopk_*) refer to rows of the candidate set they were computed on: any
// change of that set -- and a sweep of the other flavour, which overwrites dbest_* -- makes them unusable for
// bogp_exchange_* (stale or out-of-range rows would be packed otherwise).
void bogp::invalidate_sweep_results(bogp_handle* h) { h->last_q = h->last_topk_q = h->last_topk_k = 0; }

// ---- lazy upload: the copy of chunk c + 1 runs beside the kernels of chunk c --------------------------------------------------------
// rows [lazy_done, upto) onto the copy stream (a copy from pageable memory blocks the HOST while the runtime stages it, not the
// device: the kernels queued before it keep running), the event re-recorded behind it
static int lazy_copy_to(bogp_handle* h, int64_t upto) {
  if (!h->hXs_lazy) return BOGP_OK;
  upto = std::min<int64_t>(upto, h->M);
  if (upto <= h->lazy_done) return BOGP_OK;
  const size_t d = (size_t)h->d;
  HIPCHK(h, hipMemcpyAsync(h->dXs_owned + (size_t)h->lazy_done * d, h->hXs_lazy + (size_t)h->lazy_done * d,
                           (size_t)(upto - h->lazy_done) * d * sizeof(double), hipMemcpyHostToDevice, h->stream_copy));
  HIPCHK(h, hipEventRecord(h->ev_copy[0], h->stream_copy));
  h->lazy_done = upto;
  return BOGP_OK;
}
// `st` waits for every copy enqueued so far
static int lazy_wait(bogp_handle* h, hipStream_t st) {
  if (!h->hXs_lazy || h->lazy_done == 0) return BOGP_OK;
  HIPCHK(h, hipStreamWaitEvent(st, h->ev_copy[0], 0));
  return BOGP_OK;
}
// everything copied and visible to the main stream; the host rows are not needed any more
static int lazy_finish(bogp_handle* h) {
  if (!h->hXs_lazy) return BOGP_OK;
  int e = lazy_copy_to(h, h->M);
  if (e) return e;
  HIPCHK(h, hipStreamSynchronize(h->stream_copy));
  h->hXs_lazy = nullptr;
  return BOGP_OK;
}
static int lazy_drop(bogp_handle* h) {  // new candidates arrive: pending copies of the old ones must not land later
  if (h->hXs_lazy) {
    HIPCHK(h, hipStreamSynchronize(h->stream_copy));
    h->hXs_lazy = nullptr;
  }
  return BOGP_OK;
}

extern "C" int bogp_candidates_upload_lazy(bogp_handle* h, const double* Xs, int64_t M) {
  if (!h) return BOGP_ERR_INVALID;
  invalidate_sweep_results(h);
  if (!Xs || M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_upload_lazy: Xs must be non-null and M > 0");
  if (!has_dim(h)) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_upload_lazy: call bogp_set_train first (d is unknown)");
  HIPCHK(h, hipSetDevice(h->device));
  int e = lazy_drop(h);
  if (e) return e;
  if (!h->stream_copy) HIPCHK(h, hipStreamCreateWithFlags(&h->stream_copy, hipStreamNonBlocking));
  if (!h->ev_copy.at(0)) FAIL(h, BOGP_ERR_HIP, "hipEventCreate failed");
  if ((e = h->dXs_owned.ensure(h, (size_t)M * h->d))) return e;
  // (the buffer may have been re-allocated, and the last sweep may still read the old candidates: the copies start behind it)
  HIPCHK(h, hipEventRecord(h->ev_copy[0], h->stream));
  HIPCHK(h, hipStreamWaitEvent(h->stream_copy, h->ev_copy[0], 0));
  h->dXs = h->dXs_owned;
  h->M = M;
  h->hXs_lazy = Xs;
  h->lazy_done = 0;
  // the first 8 MB go now: they are what the first chunk of the next sweep waits for
  return lazy_copy_to(h, std::max<int64_t>(1, ((int64_t)8 << 20) / (int64_t)(h->d * sizeof(double))));
}

extern "C" int bogp_candidates_upload(bogp_handle* h, const double* Xs, int64_t M) {
  if (!h) return BOGP_ERR_INVALID;
  invalidate_sweep_results(h);
  if (!has_dim(h)) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_upload: call bogp_set_train first (d is unknown)");
  if (!Xs || M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_upload: Xs must be non-null and M > 0");
  HIPCHK(h, hipSetDevice(h->device));
  int e = lazy_drop(h);
  if (e) return e;
  if ((e = h->dXs_owned.ensure(h, (size_t)M * h->d))) return e;
  HIPCHK(h, hipMemcpyAsync(h->dXs_owned, Xs, (size_t)M * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->dXs = h->dXs_owned;
  h->M = M;
  return BOGP_OK;
}

// shared front end of the three on-device generators: validates the box, sizes the candidate buffer, stages lo / hi
static int generate_prepare(bogp_handle* h, const char* who, const double* lo, const double* hi, int64_t M, int64_t first) {
  invalidate_sweep_results(h);
  if (!has_dim(h)) FAIL(h, BOGP_ERR_INVALID, "%s: call bogp_set_train first (d is unknown)", who);
  if (!lo || !hi || M <= 0 || first < 0) FAIL(h, BOGP_ERR_INVALID, "%s: bounds must be non-null, M > 0, first row/index >= 0", who);
  const int d = h->d;
  for (int k = 0; k < d; ++k)
    if (!(std::isfinite(lo[k]) && std::isfinite(hi[k]) && lo[k] <= hi[k])) FAIL(h, BOGP_ERR_INVALID, "%s: bad bounds in dimension %d", who, k);
  HIPCHK(h, hipSetDevice(h->device));
  int e = lazy_drop(h);
  if (e) return e;
  if ((e = h->dXs_owned.ensure(h, (size_t)M * d))) return e;
  if ((e = h->dbounds.ensure(h, (size_t)2 * d))) return e;
  HIPCHK(h, hipMemcpyAsync(h->dbounds, lo, d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->dbounds + d, hi, d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return BOGP_OK;
}

extern "C" int bogp_candidates_set_transform(bogp_handle* h, const int* scale, const int* precision, const double* lo,
                                             const double* hi) {
  if (!h) return BOGP_ERR_INVALID;
  if (!has_dim(h)) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_set_transform: call bogp_set_train first (d is unknown)");
  HIPCHK(h, hipSetDevice(h->device));
  if (!scale && !precision) {  // back to plain designs
    h->h_xform.clear();
    return BOGP_OK;
  }
  const int d = h->d;
  std::vector<double> spec((size_t)4 * d);
  bool any = false;
  for (int k = 0; k < d; ++k) {
    const int sc = scale ? scale[k] : BOGP_SCALE_LINEAR, pr = precision ? precision[k] : -1;
    if (sc < BOGP_SCALE_LINEAR || sc > BOGP_SCALE_BILOG) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_set_transform: unknown scale id %d in dimension %d", sc, k);
    if (pr > 15) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_set_transform: precision %d in dimension %d (at most 15 decimals)", pr, k);
    if (pr >= 0 && (!lo || !hi || !(lo[k] <= hi[k]))) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_set_transform: rounding needs the variable's bounds (dimension %d)", k);
    spec[4 * k] = sc; spec[4 * k + 1] = pr < 0 ? -1 : pr;
    spec[4 * k + 2] = lo ? lo[k] : 0.0; spec[4 * k + 3] = hi ? hi[k] : 0.0;
    any = any || sc != BOGP_SCALE_LINEAR || pr >= 0;
  }
  if (!any) {
    h->h_xform.clear();
    return BOGP_OK;
  }
  if (int rc = h->dxform.ensure(h, (size_t)4 * BOGP_MAX_DIM)) return rc;
  h->h_xform = spec;
  HIPCHK(h, hipMemcpy(h->dxform, spec.data(), spec.size() * sizeof(double), hipMemcpyHostToDevice));
  return BOGP_OK;
}

static int generate_finish(bogp_handle* h, int64_t M) {
  if (!h->h_xform.empty() && (int)h->h_xform.size() == 4 * h->d)
    HIPCHK(h, launch_candidates_transform(h->dXs_owned, M * h->d, h->d, h->dxform, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));  // lo / hi (and sv) are caller memory
  h->dXs = h->dXs_owned;
  h->M = M;
  return BOGP_OK;
}

extern "C" int bogp_candidates_generate(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                                        int64_t first_row) {
  if (!h) return BOGP_ERR_INVALID;
  int e = generate_prepare(h, "bogp_candidates_generate", lo, hi, M, first_row);
  if (e) return e;
  const int d = h->d;
  HIPCHK(h, launch_generate_uniform(h->dXs_owned, M * d, d, h->dbounds, h->dbounds + d, seed, (uint64_t)first_row * (uint64_t)d, h->stream));
  return generate_finish(h, M);
}

extern "C" int bogp_candidates_generate_lhs(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                                            int64_t first_row, int64_t n_strata) {
  if (!h) return BOGP_ERR_INVALID;
  int e = generate_prepare(h, "bogp_candidates_generate_lhs", lo, hi, M, first_row);
  if (e) return e;
  if (n_strata < first_row + M) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_generate_lhs: rows [%lld, %lld) exceed the %lld strata", (long long)first_row, (long long)(first_row + M), (long long)n_strata);
  const int d = h->d;
  HIPCHK(h, launch_generate_lhs(h->dXs_owned, M * d, d, h->dbounds, h->dbounds + d, seed, (uint64_t)first_row * (uint64_t)d, (uint64_t)n_strata, h->stream));
  return generate_finish(h, M);
}

// largest design the maximin criterion accepts: M^2 d / 2 pair terms per trial design (2^18 points, d = 20: ~0.1 s each)
static constexpr int64_t BOGP_MAXIMIN_MAX_POINTS = (int64_t)1 << 18;

extern "C" int bogp_candidates_min_pdist2(bogp_handle* h, double* min_sq) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_min_pdist2: no candidates");
  if (!min_sq) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_min_pdist2: null output");
  if (h->M > BOGP_MAXIMIN_MAX_POINTS) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_candidates_min_pdist2: %lld points exceed the %lld-point limit of the O(M^2 d) pair sweep", (long long)h->M, (long long)BOGP_MAXIMIN_MAX_POINTS);
  HIPCHK(h, hipSetDevice(h->device));
  {
    const int e = lazy_finish(h);
    if (e) return e;
  }
  unsigned long long* dout = (unsigned long long*)h->dscal.ptr;
  HIPCHK(h, launch_min_pdist2(h->dXs, (int)h->M, h->d, dout, h->stream));
  unsigned long long bits = 0;
  HIPCHK(h, hipMemcpyAsync(&bits, dout, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (bits == ~0ull) {
    *min_sq = INFINITY;  // fewer than two points
  } else {
    memcpy(min_sq, &bits, sizeof(double));
  }
  return BOGP_OK;
}

extern "C" int bogp_candidates_generate_lhs_maximin(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                                                    int iterations, double* best_min_dist, int* best_iteration) {
  if (!h) return BOGP_ERR_INVALID;
  if (iterations < 1 || iterations > 64) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_generate_lhs_maximin: iterations = %d outside [1, 64]", iterations);
  if (M > BOGP_MAXIMIN_MAX_POINTS) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_candidates_generate_lhs_maximin: %lld points exceed the %lld-point limit of the O(M^2 d) pair sweep", (long long)M, (long long)BOGP_MAXIMIN_MAX_POINTS);
  int e = generate_prepare(h, "bogp_candidates_generate_lhs_maximin", lo, hi, M, 0);
  if (e) return e;
  const int d = h->d;
  // trial designs live in the unit cube, un-transformed (pyDOE measures the design before the caller scales it)
  if ((e = h->dbatch.ensure(h, (size_t)2 * d))) return e;
  std::vector<double> unit((size_t)2 * d, 0.0);
  for (int k = 0; k < d; ++k) unit[d + k] = 1.0;
  HIPCHK(h, hipMemcpyAsync(h->dbatch, unit.data(), (size_t)2 * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
  unsigned long long* dout = (unsigned long long*)h->dscal.ptr;
  double best = -1.0;
  int best_it = 0;
  for (int it = 0; it < iterations; ++it) {
    const uint64_t s_it = seed + 0x9E3779B97F4A7C15ull * (uint64_t)it;
    HIPCHK(h, launch_generate_lhs(h->dXs_owned, M * d, d, h->dbatch, h->dbatch + d, s_it, 0, (uint64_t)M, h->stream));
    HIPCHK(h, launch_min_pdist2(h->dXs_owned, (int)M, d, dout, h->stream));
    unsigned long long bits = 0;
    HIPCHK(h, hipMemcpyAsync(&bits, dout, sizeof(bits), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double msq = INFINITY;
    if (bits != ~0ull) memcpy(&msq, &bits, sizeof(double));
    const double dist = std::sqrt(msq);  // pyDOE compares the distances: `if maxdist < np.min(d)` keeps the EARLIER design on ties
    if (best < dist) {
      best = dist;
      best_it = it;
    }
  }
  const uint64_t s_best = seed + 0x9E3779B97F4A7C15ull * (uint64_t)best_it;
  HIPCHK(h, launch_generate_lhs(h->dXs_owned, M * d, d, h->dbounds, h->dbounds + d, s_best, 0, (uint64_t)M, h->stream));
  if (best_min_dist) *best_min_dist = best;
  if (best_iteration) *best_iteration = best_it;
  return generate_finish(h, M);
}

extern "C" int bogp_candidates_generate_sobol(bogp_handle* h, const double* lo, const double* hi, int64_t M,
                                              int64_t first_index, const uint64_t* sv, int bits) {
  if (!h) return BOGP_ERR_INVALID;
  int e = generate_prepare(h, "bogp_candidates_generate_sobol", lo, hi, M, first_index);
  if (e) return e;
  if (!sv || bits < 1 || bits > 53) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_generate_sobol: direction numbers must be non-null with 1 <= bits <= 53");
  if (((uint64_t)(first_index + M - 1) >> bits) != 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_generate_sobol: index %lld needs more than %d bits", (long long)(first_index + M - 1), bits);
  const int d = h->d;
  if ((e = h->dsobol.ensure(h, (size_t)d * bits))) return e;
  HIPCHK(h, hipMemcpyAsync(h->dsobol, sv, (size_t)d * bits * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, launch_generate_sobol(h->dXs_owned, M * d, d, h->dbounds, h->dbounds + d, (const uint64_t*)h->dsobol.ptr, bits,
                                  (uint64_t)first_index * (uint64_t)d, h->stream));
  return generate_finish(h, M);
}

extern "C" int bogp_candidates_read(bogp_handle* h, const int64_t* rows, int n, double* out) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_read: no candidates");
  if (!rows || !out || n < 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_read: null pointer");
  HIPCHK(h, hipSetDevice(h->device));
  {
    const int e = lazy_finish(h);
    if (e) return e;
  }
  const int d = h->d;
  for (int i = 0; i < n; ++i)
    if (rows[i] < 0 || rows[i] >= h->M) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_read: row %lld outside [0, %lld)", (long long)rows[i], (long long)h->M);
  for (int i = 0; i < n;) {  // one copy per run of consecutive rows
    int j = i + 1;
    while (j < n && rows[j] == rows[j - 1] + 1) ++j;
    HIPCHK(h, hipMemcpyAsync(out + (size_t)i * d, h->dXs + (size_t)rows[i] * d, (size_t)(j - i) * d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    i = j;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return BOGP_OK;
}

extern "C" int bogp_candidates_bind(bogp_handle* h, const void* d_Xs, int64_t M) {
  if (!h) return BOGP_ERR_INVALID;
  if (!d_Xs || M <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_candidates_bind: pointer must be non-null and M > 0");
  invalidate_sweep_results(h);
  {
    const int e = lazy_drop(h);
    if (e) return e;
  }
  h->dXs = (const double*)d_Xs;
  h->M = M;
  return BOGP_OK;
}

// ------------------------------------------------------------------------------------------------------
// posterior + acquisition sweep
// ------------------------------------------------------------------------------------------------------
// What bogp_last_timing reports, from the spans a call leaves on h->timer (SpanTimer, bogp_handle.h): corr_ms = the producer spans,
// contract_ms = the contraction spans, acquisition_ms = the criteria spans -- or, where a whole-sweep span exists, that span less the
// other two sums (the criteria spans are then not read).  A chunk has five marks: 0 / 1 around its producer (producer stream), 2, 3, 4 on
// the main stream; p0 / p1 are the two marks around the pilot's contraction.
//
//   path                  | producer                     | contraction                  | criteria
//   ----------------------+------------------------------+------------------------------+-----------------------------------------------
//   small batch           | -                            | -                            | -                               (n_chunks = 0)
//   one launch            | -                            | k_sweep_small                | -
//   chunks                | (0,1)                        | (2,3)                        | (3,4)
//   pruned chunks         | (0,1)                        | (2,3); the pilot's (p0,p1)   | (1,2) bound / scan / gather, (3,4); in the pilot's
//                         |                              |                              | chunk (1,p0) and (p1,2) in place of (1,2)
//   one pass              | every producer and FP32-sums | every contraction launch;    | whole sweep less the two: the small kernels and
//                         | launch; a fall-back's (0,1)  | a fall-back's (2,3)          | the host's waits
//   forest calls          | -                            | -                            | k_forest / k_forest_ehvi         (n_chunks = 1)
//
// The believer batches (bogp_api_believer.hip) leave pass 0 here as "chunks" -- its criteria span is k_acquisition, k_ehvi or
// k_constrained / k_ehvi_constrained -- and the passes behind it on h->bel_timer, which bogp_believer_last / _ehvi_last / _constrained_last /
// _ehvi_constrained_last report (the last three read the B_CRITERION sum, h->bel_criterion_ms):
//
//   kind                  | spans
//   ----------------------+------------------------------------------------------------------------------------------------------
//   B_SOLVE               | one per believed point: upload, r(p), the two solves with V, the read-back
//   B_PRODUCER, B_PASS    | per chunk of a candidate pass: the producer (first believed point only when one chunk holds every row), k_believer
//   B_CRITERION           | one per pass of a multi-target family: k_believer_ehvi, k_believer_constrained or k_believer_ehvi_constrained over all rows

// The spans of the last sweep are read lazily (bogp_last_timing, or the next sweep): reading them needs the events
// to have completed, and an un-synchronised sweep (bogp_sweep without host outputs) must not wait for them.
static void collect_timing(bogp_handle* h) {
  if (!h->timing_pending) return;
  h->timing_pending = false;
  (void)hipSetDevice(h->device);
  SpanTimer& t = h->timer;
  h->t_corr_ms = t.sum(T_PRODUCER);
  h->t_contract_ms = t.sum(T_CONTRACT);
  const bool whole = std::any_of(t.spans.begin(), t.spans.end(), [](const SpanTimer::Span& s) { return s.kind == T_WHOLE; });
  h->t_acq_ms = whole ? t.sum(T_WHOLE) - h->t_corr_ms - h->t_contract_ms : t.sum(T_CRITERIA);
}


int bogp::candidates_ready(bogp_handle* h) { return lazy_finish(h); }
void bogp::clear_sweep_timing(bogp_handle* h) {
  collect_timing(h);
  h->t_corr_ms = h->t_contract_ms = h->t_acq_ms = 0;
  h->n_chunks = 0;
}

// ---- what the sweep shares with the believer and the Thompson passes (bogp_handle.h) -------------------------------------------------
int bogp::sweep_geometry(bogp_handle* h, int rows, SweepGeometry* g) {
  int64_t chunk_bytes = (int64_t)1 << 30;
  if (const char* env = getenv("BOGP_CHUNK_MB")) chunk_bytes = (int64_t)std::max(1, atoi(env)) << 20;
  g->Mc = sweep_chunk_rows(rows, h->M, chunk_bytes);
  if (g->Mc < 0) FAIL(h, BOGP_ERR_UNSUPPORTED, "a chunk of more than %lld candidates is beyond the kernels' 32-bit row offsets: lower BOGP_CHUNK_MB", (long long)SWEEP_MAX_CHUNK_ROWS);
  g->nchunk = (h->M + g->Mc - 1) / g->Mc;
  g->S = sweep_slices(h->Np);
  return BOGP_OK;
}

CorrArgs bogp::corr_chunk_args(const bogp_handle* h, const SweepGeometry& g, int64_t m0, int b) {
  CorrArgs ca;
  ca.Xs = h->dXs; ca.M = h->M; ca.m0 = m0; ca.Mc = g.Mc; ca.d = h->d; ca.Np = h->Np; ca.nblk_per_split = SWEEP_NBLK_PER_SPLIT;
  ca.sqrt_theta = h->dsqrt_theta; ca.XthT = h->dXthT; ca.xnorm = h->dXnorm; ca.gamma = h->dgamma; ca.wvec = h->dw;
  ca.rT = h->drT[b]; ca.mu_part = h->dmu_part[b]; ca.w_part = h->dw_part[b];
  return ca;
}

int bogp::ensure_sweep_outputs(bogp_handle* h, int q, int64_t nblk, size_t n_out, bool want_acq_out) {
  int e;
  if (q > 0) {
    if ((e = h->dblk_val.ensure(h, (size_t)q * nblk))) return e;
    if ((e = h->dblk_idx.ensure(h, (size_t)q * nblk))) return e;
    if ((e = h->dbest_val.ensure(h, BOGP_MAX_Q)) || (e = h->dbest_idx.ensure(h, BOGP_MAX_Q))) return e;
  }
  if (n_out > 0 && ((e = h->dmu_out.ensure(h, n_out)) || (e = h->dmse_out.ensure(h, n_out)))) return e;
  if (want_acq_out && (e = h->dacq_out.ensure(h, (size_t)q * h->M))) return e;
  return BOGP_OK;
}

int bogp::rank_stored_values(bogp_handle* h, const double* vals, int64_t M, int q, int k, hipStream_t st) {
  // rank 0 is the argmax over the stored values; ranks 1 .. k-1 repeat it with the winners so far masked out -- all q criteria per
  // launch, the winners kept on the device: 2 k queued launches (launch_topk)
  const int64_t nblk = (M + 255) / 256;
  int e;
  if ((e = h->dblk_val.ensure(h, (size_t)q * (nblk + 1)))) return e;
  if ((e = h->dblk_idx.ensure(h, (size_t)q * (nblk + 1)))) return e;
  if ((e = h->dtopk_val.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return e;
  if ((e = h->dtopk_idx.ensure(h, (size_t)BOGP_MAX_Q * BOGP_MAX_TOPK))) return e;
  HIPCHK(h, launch_topk(vals, M, q, k, h->dblk_val, h->dblk_idx, h->dtopk_val, h->dtopk_idx, st));
  return BOGP_OK;
}

void bogp::pad_short_ranks(double* best_val, int64_t* best_idx, int n) {
  for (int i = 0; i < n; ++i)
    if (best_idx[i] == INT64_MAX) {  // fewer candidates than k: pad with (-inf, -1)
      best_val[i] = -INFINITY;
      best_idx[i] = -1;
    }
}

int bogp::fetch_winners(bogp_handle* h, int q, int k, const double* vals, double* best_val, int64_t* best_idx, hipStream_t st) {
  if (k == 1) {  // the sweep's own argmax
    HIPCHK(h, hipMemcpyAsync(best_val, h->dbest_val, (size_t)q * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(best_idx, h->dbest_idx, (size_t)q * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  } else {  // ranks 0 .. k-1 over the stored values, as bogp_sweep_topk ranks them (dtopk_*: what bogp_exchange_topk packs)
    if (int e = rank_stored_values(h, vals, h->M, q, k, st)) return e;
    HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)q * k * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)q * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  pad_short_ranks(best_val, best_idx, q * k);
  return BOGP_OK;
}

void bogp::multi_target_model(const bogp_handle* h, MultiTargetChunk& a) {
  a.gamma = h->dgamma_base; a.ld_gamma = h->Np; a.N = h->N; a.m = h->n_t;
  for (int t = 0; t < a.m; ++t) a.sigma2[t] = h->sigma2_t[t];
}

int bogp::check_criteria(bogp_handle* h, int q, const int* acq_id, const double* acq_par) {
  for (int i = 0; i < q; ++i) {
    if (acq_id[i] < 0 || acq_id[i] > 3) FAIL(h, BOGP_ERR_INVALID, "unknown acquisition id %d", acq_id[i]);
    const bool zero_ok = acq_id[i] == BOGP_ACQ_EPSILON_PI;  // epsilon = 0 is plain PI
    if (acq_id[i] != BOGP_ACQ_EI && (!acq_par || !(acq_par[i] > 0 || (zero_ok && acq_par[i] == 0))))
      FAIL(h, BOGP_ERR_INVALID, "acquisition parameter %d must be > 0 (the reference asserts alpha/epsilon/t > 0)", i);
  }
  return BOGP_OK;
}

#ifndef BOGP_PRUNE_PILOT
#define BOGP_PRUNE_PILOT 4096  // (1024 / 8192 measured with `make EXTRA=-DBOGP_PRUNE_PILOT=...`: profiles/prune_sweep.txt)
#endif
constexpr int64_t PRUNE_PILOT = BOGP_PRUNE_PILOT;  // rows of chunk 0 evaluated exactly to seed the thresholds; a multiple of 256
static_assert(PRUNE_PILOT % 256 == 0 && PRUNE_PILOT > 0 && PRUNE_PILOT <= 8192, "pilot rows");

template <class Args>  // AcqArgs, SmallArgs, PruneBoundArgs
static void set_criteria(Args& a, int q, const int* id, const double* par) { a.q = q; for (int i = 0; i < q; ++i) { a.acq_id[i] = id[i]; a.acq_par[i] = par ? par[i] : 0.0; } }

// what the chunked paths share: built once by run_sweep
struct SweepCtx {
  SweepRequest rq;
  SweepGeometry g;
  int64_t M, nblk_total;  // (256-row block records; per-chunk block counts are rounded up)
  int Nrows, nJ, nJ_main, NJ16, pv;
  bool vx_model, vx, overlap, prune, onepass, bound32;
  hipStream_t st, stP;
  // pruned sweep: rows of the survivor buffer, segment geometry of the one-pass flow, the carved work space (sweep_workspace)
  int64_t Ms, seg_rows, seg_stride, Rmax, sidx_cap, prune_nbk;
  long long* pctl;
  int64_t *poffsets, *pmap, *psidx, *psidx1;
  int *psel, *pblk_count;
  unsigned char *pflags, *pflags1;
  double *pxc, *dss_surv;
  double *pxc1, *pmu32, *pwd32, *pna32;  // FP32 stage: the candidate rows of S1; the per-row sums and squared norms of a segment
  int64_t blk_offset, prune_pending;  // block records written so far; upper bound of the survivors waiting in the buffer (their count stays on the device)
};

// the model's and the request's half of k_acquisition's arguments; the caller adds the arrays and the geometry of its launch
static AcqArgs acq_model_args(const bogp_handle* h, const SweepRequest& rq, int S, int nJ, int64_t nblk_total) {
  AcqArgs aa;
  memset(&aa, 0, sizeof(aa));
  aa.S = S; aa.nJ = nJ; aa.beta = h->beta; aa.G = h->G; aa.estimate_trend = h->estimate_trend; aa.sigma2 = h->sigma2;
  set_criteria(aa, rq.q, rq.acq_id, rq.acq_par);
  aa.plugin = rq.plugin; aa.minimize = rq.minimize; aa.M = h->M;
  aa.blk_val = h->dblk_val; aa.blk_idx = h->dblk_idx; aa.nblk_total = nblk_total;
  aa.mu_out = rq.want_out ? h->dmu_out : nullptr; aa.mse_out = rq.want_out ? h->dmse_out : nullptr; aa.acq_out = rq.want_acq_out ? h->dacq_out : nullptr;
  return aa;
}

// ... and of k_prune_bound's; the caller adds the region (partial sums, stride, rows)
static PruneBoundArgs prune_bound_args(const bogp_handle* h, const SweepCtx& cx) {
  PruneBoundArgs pb;
  memset(&pb, 0, sizeof(pb));
  pb.S = cx.g.S; pb.beta = h->beta; pb.G = h->G; pb.sigma2 = h->sigma2; pb.plugin = cx.rq.plugin; pb.estimate_trend = h->estimate_trend;
  pb.minimize = cx.rq.minimize;
  set_criteria(pb, cx.rq.q, cx.rq.acq_id, cx.rq.acq_par);
  pb.best_val = h->dbest_val; pb.flags = cx.pflags; pb.blk_count = cx.pblk_count;
  return pb;
}

// Small batches (the reference's one-point-per-call usage through L-BFGS-B): the tiled contraction would leave one
// workgroup walking all N columns alone (~0.3 ms at N = 2048).  For M <= 32 the posterior is instead
// r -> rt = V r (k_gemm64 with M right-hand sides) -> column reductions, feeding the same acquisition kernel.
static int sweep_small_batch(bogp_handle* h, const SweepRequest& rq) {
  hipStream_t st = h->stream;
  const int64_t M = h->M;
  int e, B = (int)M, N = h->N;
  if ((e = h->dbatch.ensure(h, (size_t)3 * N * B + 3 * (size_t)B))) return e;
  double *dr = h->dbatch, *ds2 = dr + (size_t)N * B, *drt = ds2 + (size_t)N * B;
  double* dred = drt + (size_t)N * B;  // mu[B], wd[B], ss[B]
  if ((e = ensure_sweep_outputs(h, rq.q, 2, rq.want_out ? (size_t)M : 0, rq.want_acq_out))) return e;
  HIPCHK(h, launch_batch_corr(h->kernel, h->dX, N, h->d, h->dtheta, h->dXs, B, dr, ds2, st));
  HIPCHK(h, launch_gemm(0, 0, N, B, N, 1.0, h->dV, h->ldr, dr, N, 0.0, drt, N, st, 1));  // rt = V r, V lower with a zero upper triangle
  HIPCHK(h, launch_col_reduce(dr, drt, N, B, h->dgamma, h->dw, dred, dred + B, dred + 2 * B, st));
  AcqArgs aa = acq_model_args(h, rq, 1, 1, 1);
  aa.mu_part = dred; aa.w_part = dred + B; aa.ss_part = dred + 2 * B; aa.Mc = B; aa.mcount = B; aa.m0 = 0;
  HIPCHK(h, launch_acquisition(aa, st));
  if (rq.q > 0) HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, 1, 1, rq.q, h->dbest_val, h->dbest_idx, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->t_corr_ms = h->t_contract_ms = h->t_acq_ms = 0;
  h->n_chunks = 0; h->timing_pending = false; h->prune_used = false;
  h->contracted_rows = rq.need_var ? M : 0;
  return BOGP_OK;
}

// Small training sets (Np <= 512, d <= 60, constant trend): the whole sweep is ONE launch of k_sweep_small -- producer,
// triangular contraction, posterior, criteria and argmax fused, r never leaves LDS (kernels_small.hip).
static int sweep_one_launch(bogp_handle* h, const SweepRequest& rq) {
  hipStream_t st = h->stream;
  const int Np = h->Np;
  const int64_t M = h->M, nblk = std::max<int64_t>(sweep_small_blocks(M, h->n_cu), (M + 15) / 16);
  int e;
  if ((e = ensure_sweep_outputs(h, rq.q, nblk, rq.want_out ? (size_t)M : 0, rq.want_acq_out))) return e;
  if (!h->dcounter) {
    if ((e = h->dcounter.ensure(h, 1))) return e;
    HIPCHK(h, hipMemsetAsync(h->dcounter, 0, sizeof(unsigned int), st));
  }
  SmallArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.Xs = h->dXs; sa.sqrt_theta = h->dsqrt_theta; sa.XthT = h->dXthT; sa.gamma = h->dgamma; sa.wvec = h->dw; sa.Vp = h->dVp;
  sa.M = M; sa.d = h->d; sa.Np = Np; sa.NJ16 = Np / 16; sa.NKP = Np / 8; sa.need_var = rq.need_var ? 1 : 0;
  sa.beta = h->beta; sa.G = h->G; sa.sigma2 = h->sigma2; sa.plugin = rq.plugin;
  sa.estimate_trend = h->estimate_trend; sa.minimize = rq.minimize;
  set_criteria(sa, rq.q, rq.acq_id, rq.acq_par);
  sa.mu_out = rq.want_out ? h->dmu_out : nullptr; sa.mse_out = rq.want_out ? h->dmse_out : nullptr;
  sa.acq_out = rq.want_acq_out ? h->dacq_out : nullptr;
  sa.blk_val = h->dblk_val; sa.blk_idx = h->dblk_idx; sa.nblk = nblk; sa.counter = h->dcounter;
  sa.best_val = h->dbest_val; sa.best_idx = h->dbest_idx;
  const bool stamps = getenv("BOGP_SMALL_STAMPS") && atoi(getenv("BOGP_SMALL_STAMPS"));
  if (stamps) {  // measurement aid: per-phase wave-cycles of this launch, printed on stderr
    if ((e = h->dbatch.ensure(h, (size_t)8))) return e;
    HIPCHK(h, hipMemsetAsync(h->dbatch, 0, 8 * sizeof(double), st));
    sa.stamps = (long long*)h->dbatch.ptr;
  }
  if ((e = timed_span(h, h->timer, st, T_CONTRACT, [&] { return launch_sweep_small(h->kernel, sa, h->n_cu, st); }))) return e;  // one kernel: reported as the contraction's time
  h->n_chunks = 1; h->timing_pending = true; h->prune_used = false;
  h->contracted_rows = rq.need_var ? M : 0;
  if (rq.sync || stamps) HIPCHK(h, hipStreamSynchronize(st));
  if (stamps) {
    collect_timing(h);
    long long sv[5] = {0, 0, 0, 0, 0};
    HIPCHK(h, hipMemcpy(sv, h->dbatch, sizeof(sv), hipMemcpyDeviceToHost));
    const double nw = (double)std::max<long long>(1, sv[4]);
    fprintf(stderr, "k_sweep_small M=%lld: %.3f ms; per wave: produce %.0f, contract %.0f, wait-at-barrier %.0f, epilogue %.0f cycles (%lld waves)\n",
            (long long)M, h->t_contract_ms, sv[0] / nw, sv[1] / nw, sv[2] / nw, sv[3] / nw, sv[4]);
  }
  return BOGP_OK;
}

// The pruned sweep's sizes and work space (kernels_prune.hip): control words | block offsets | index map | selected rows |
// block counts | flags | one pass: survivor indices of a segment | candidate rows of a round; the survivor buffer = the second chunk
// buffer of the two-stream mode.  One pass: the rows behind the pilot are bounded a SEGMENT at a time -- as many
// whole chunks as keep the two partial-sum arrays within 256 MiB -- and only survivors get columns.  Then the buffers every chunked path needs.
static int sweep_workspace(bogp_handle* h, SweepCtx& cx) {
  const int64_t Mc = cx.g.Mc, Mpad = ((cx.M + 63) / 64) * 64;
  const int S = cx.g.S, nbuf = cx.overlap ? 2 : 1;
  int e;
  cx.Ms = cx.prune ? Mc : 0;  // rows of the survivor buffer: one chunk's, i.e. four chunks' worst case (half a chunk measured: profiles/prune_sweep.txt)
  cx.seg_rows = cx.onepass ? std::max<int64_t>(1, (((int64_t)256 << 20) / (int64_t)(2 * S * sizeof(double))) / Mc) * Mc : 0;
  cx.seg_stride = std::min<int64_t>(cx.seg_rows, Mpad);  // row stride of a segment's partial sums
  cx.Rmax = std::max<int64_t>(Mc, cx.seg_stride);        // rows one bounding launch may cover
  cx.sidx_cap = cx.seg_stride / 4 + 1;                   // survivor indices kept: a fuller segment falls back
  cx.prune_nbk = cx.Rmax / 256 + 1;
  if (cx.prune) {
    const size_t w_off = PRUNE_CTL_WORDS, w_map = w_off + (size_t)cx.prune_nbk + 1, w_sel = w_map + (size_t)cx.Ms, w_cnt = w_sel + (size_t)(Mc / 4) / 2 + 1,
                 w_flag = w_cnt + (size_t)cx.prune_nbk / 2 + 1, w_sidx = w_flag + (size_t)cx.Rmax / 8 + 1, w_xc = w_sidx + (cx.onepass ? (size_t)cx.sidx_cap : 0),
                 w_xc1 = w_xc + (cx.onepass ? (size_t)cx.Ms * h->d : 0),
                 // FP32 stage: S1's indices and candidate rows, both capped like S's; the segment's flags, sums and norms
                 w_sidx1 = w_xc1 + (cx.bound32 ? (size_t)cx.sidx_cap * h->d : 0), w_flag1 = w_sidx1 + (cx.bound32 ? (size_t)cx.sidx_cap : 0),
                 w_row32 = w_flag1 + (cx.bound32 ? (size_t)cx.Rmax / 8 + 1 : 0), w_end = w_row32 + (cx.bound32 ? (size_t)3 * cx.Rmax : 0);
    if ((e = h->dprune.ensure(h, w_end))) return e;
    cx.pctl = h->dprune; cx.poffsets = (int64_t*)(h->dprune + w_off); cx.pmap = (int64_t*)(h->dprune + w_map); cx.psel = (int*)(h->dprune + w_sel);
    cx.pblk_count = (int*)(h->dprune + w_cnt); cx.pflags = (unsigned char*)(h->dprune + w_flag);
    cx.psidx = (int64_t*)(h->dprune + w_sidx); cx.pxc = (double*)(h->dprune + w_xc);
    cx.pxc1 = (double*)(h->dprune + w_xc1); cx.psidx1 = (int64_t*)(h->dprune + w_sidx1); cx.pflags1 = (unsigned char*)(h->dprune + w_flag1);
    if (cx.bound32) { h->b32_ws_row32 = w_row32; h->b32_ws_flag1 = w_flag1; h->b32_ws_rmax = (size_t)cx.Rmax; }
    cx.pmu32 = (double*)(h->dprune + w_row32); cx.pwd32 = cx.pmu32 + cx.Rmax; cx.pna32 = cx.pwd32 + cx.Rmax;
    if ((e = h->drT[1].ensure(h, (size_t)cx.Nrows * cx.Ms))) return e;
    if ((e = h->dmu_part[1].ensure(h, (size_t)S * cx.Ms))) return e;
    if ((e = h->dw_part[1].ensure(h, (size_t)S * cx.Ms))) return e;
  }
  for (int b = 0; b < nbuf; ++b) {
    // (one pass: the chunk buffer is allocated only if a per-chunk path runs after all; the partial sums are a segment's)
    if (!cx.onepass && (e = h->drT[b].ensure(h, (size_t)cx.Nrows * Mc))) return e;
    if ((e = h->dmu_part[b].ensure(h, (size_t)S * (cx.onepass ? cx.Rmax : Mc)))) return e;
    if ((e = h->dw_part[b].ensure(h, (size_t)S * (cx.onepass ? cx.Rmax : Mc)))) return e;
  }
  if ((e = h->dss_part.ensure(h, (size_t)cx.nJ * (Mc + cx.Ms)))) return e;  // (+ the survivor buffer's sums)
  cx.dss_surv = h->dss_part + (size_t)cx.nJ * Mc;
  if (h->p > 1) {
    const size_t n_tiles = (size_t)Mc * ((h->p + 127) / 128 * 128);  // whole 128-column tiles (k_mm128)
    if (!cx.vx_model && ((e = h->dTt.ensure(h, n_tiles)) || (e = h->dCS.ensure(h, n_tiles)))) return e;
    if ((e = h->duu.ensure(h, (size_t)Mc))) return e;
    if ((e = h->dmtrend.ensure(h, (size_t)Mc))) return e;
  }
  if (cx.pv > 0)
    for (int b = 0; b < nbuf; ++b)
      if ((e = h->dtpart[b].ensure(h, (size_t)S * cx.pv * Mc))) return e;
  return BOGP_OK;
}

// Polynomial trend of one chunk: mean f(x*) . beta, and under universal kriging u = G^-T (Ft^T L^-1 r - f(x*)) (gpr.py:496-498):
// T = r W (Mc x p, a tile product on the chunk that k_contract has just read), c = T - f(x*), u^T u = c^T (Ft^T Ft)^-1 c.
// The two products run on k_mm128 (128 x 128 tiles, kernels_chol.hip) when the chunk is whole tiles -- the default
// chunk sizes are; rows past Mc_eff of the last tile are computed on stale chunk data and never read -- and on the
// generic k_gemm64 otherwise.  Leaves mtrend / uu in `aa`.
static int sweep_trend_chunk(bogp_handle* h, const SweepCtx& cx, int b, int64_t m0, int64_t mcount, int64_t Mc_eff, AcqArgs& aa) {
  hipStream_t st = cx.st;
  const int64_t Mc = cx.g.Mc;
  const int Np = h->Np, d = h->d, pt = h->p, pp = (pt + 127) / 128 * 128;
  if (cx.vx) {
    // (mtrend was written by k_trend_rows beside the chunk's extra rows; |u|^2 comes out of the contraction)
  } else if (cx.pv > 0) {  // (T = W^T r was accumulated by the producer itself)
    HIPCHK(h, launch_trend_small(h->trend, h->dXs, m0, mcount, d, Mc, h->dbetav, h->dtpart[b], cx.g.S, cx.pv, pt, h->dSinv, h->dmtrend, h->duu, st));
    aa.uu = h->duu;
  } else {
    const bool tiles128 = Mc % 128 == 0, products = h->estimate_trend && !cx.vx_model;
    const int TI = (int)((Mc_eff + 127) / 128);
    const double one = 1.0, zero = 0.0;
    if (products) {
      if (tiles128)
        HIPCHK(h, launch_mm128_gen(h->drT[b], (int)Mc, h->dWpT, pp, h->dTt, (int)Mc, TI, pp / 128, Np, st));
      else
        HIPCHK(h, launch_gemm(0, 0, (int)Mc_eff, pt, Np, one, h->drT[b], (int)Mc, h->dWp, Np, zero, h->dTt, (int)Mc, st, 0, &h->gsplit));
    }
    HIPCHK(h, launch_trend_terms(h->trend, h->dXs, m0, mcount, d, Mc, h->dbetav, products ? h->dTt : nullptr, h->dmtrend, st));
    if (products) {
      if (tiles128)
        HIPCHK(h, launch_mm128_gen(h->dTt, (int)Mc, h->dSinvP, pp, h->dCS, (int)Mc, TI, pp / 128, pp, st));
      else
        HIPCHK(h, launch_gemm(0, 0, (int)Mc_eff, pt, pt, one, h->dTt, (int)Mc, h->dSinv, pt, zero, h->dCS, (int)Mc, st, 0, &h->gsplit));
      HIPCHK(h, launch_rowdot(h->dTt, h->dCS, Mc, mcount, pt, h->duu, st));
      aa.uu = h->duu;
    }
  }
  aa.mtrend = h->dmtrend;
  aa.estimate_trend = 0;  // the scalar w_part path is for the constant basis
  return BOGP_OK;
}

// One chunk of the per-chunk pruned flow, behind its producer: in chunk 0 the pilot (unless `skip` rows of it are done already), then
// bound -> scan + decision -> compaction -> gather, the contractions of both outcomes, criteria and the running best.  `model`: the
// criteria kernel's arguments less the arrays; `ka`: the chunk's contraction; `e1`: the mark behind the chunk's producer.
static int sweep_pruned_chunk(bogp_handle* h, SweepCtx& cx, const AcqArgs& model, const ContractArgs& ka, int64_t c, int64_t c_end, int64_t m0, int64_t mcount, int64_t skip, int e1) {
  hipStream_t st = cx.st;
  long long* const pctl = cx.pctl;
  const int64_t Mc = cx.g.Mc, Ms = cx.Ms, nblk_total = cx.nblk_total;
  const int q = cx.rq.q;
  SpanTimer& tm = h->timer;
  int e, p0 = -1, p1 = -1, e2 = 0, e3 = 0, e4 = 0;
  int64_t i0 = 0;  // first row of the chunk's region: behind the pilot in chunk 0
  if (skip > 0) i0 = skip;
  else if (c == 0) {  // pilot: the first rows through the contraction and the criteria as ever -> the first thresholds
    const int64_t P = std::min<int64_t>(PRUNE_PILOT, mcount);
    HIPCHK(h, launch_prune_init(pctl, h->dbest_val, h->dbest_idx, q, P, st));
    if ((e = tm.mark(h, st, &p0))) return e;
    ContractArgs kp = ka;
    kp.nMt = (int)((P + 63) / 64);
    HIPCHK(h, launch_contract(kp, st, h->contract_tile));
    if ((e = tm.mark(h, st, &p1))) return e;
    AcqArgs ap = model;
    ap.mu_part = h->dmu_part[0]; ap.w_part = h->dw_part[0]; ap.ss_part = h->dss_part; ap.Mc = Mc; ap.mcount = P; ap.m0 = 0;
    HIPCHK(h, launch_acquisition(ap, st));
    HIPCHK(h, launch_prune_update(h->dblk_val, h->dblk_idx, nblk_total, nullptr, P, q, h->dbest_val, h->dbest_idx, st));
    i0 = P;  // (a multiple of 256 unless the chunk ends with it)
  }
  const int64_t rcount = mcount - i0;
  if (rcount > 0) {  // bound -> scan + decision -> compaction -> gather
    PruneBoundArgs pb = prune_bound_args(h, cx);
    pb.mu_part = h->dmu_part[0] + i0; pb.w_part = h->dw_part[0] + i0; pb.Mc = Mc; pb.rcount = rcount;
    HIPCHK(h, launch_prune_bound(pb, st));
    HIPCHK(h, launch_prune_scan(cx.pblk_count, (rcount + 255) / 256, cx.poffsets, rcount, Ms, pctl, st));
    PruneGatherArgs pg;
    pg.ctl = pctl; pg.flags = cx.pflags; pg.offsets = cx.poffsets; pg.rcount = rcount; pg.m0 = m0 + i0; pg.Mc = Mc; pg.Ms = Ms; pg.S = cx.g.S;
    pg.Np = h->Np; pg.rT = h->drT[0] + i0; pg.mu_part = h->dmu_part[0] + i0; pg.w_part = h->dw_part[0] + i0;
    pg.rTs = h->drT[1]; pg.mu_s = h->dmu_part[1]; pg.w_s = h->dw_part[1]; pg.sel = cx.psel; pg.map = cx.pmap;
    HIPCHK(h, launch_prune_gather(pg, st));
    cx.prune_pending += rcount / 4;
  }
  // the buffer goes through the contraction behind the last chunk, and whenever the next chunk's quarter might not fit
  const bool flush = cx.prune_pending > 0 && (c + 1 == c_end || cx.prune_pending + Mc / 4 > Ms);
  if ((e = tm.mark(h, st, &e2))) return e;
  if (p0 < 0) {
    tm.span(T_CRITERIA, e1, e2);
  } else {  // (the pilot's contraction ran in between)
    tm.span(T_CRITERIA, e1, p0); tm.span(T_CONTRACT, p0, p1); tm.span(T_CRITERIA, p1, e2);
  }
  // in place or gathered is decided on the device: both contractions are queued, workgroups past the live count return at once
  if (rcount > 0) {
    ContractArgs ki = ka;
    ki.rT = h->drT[0] + i0; ki.ss_part = h->dss_part + i0; ki.nMt = (int)((rcount + 63) / 64); ki.live = pctl + 1;
    HIPCHK(h, launch_contract(ki, st, h->contract_tile));
  }
  if (flush) {
    ContractArgs kf = ka;
    kf.rT = h->drT[1]; kf.ss_part = cx.dss_surv; kf.Mc = Ms; kf.nMt = (int)(Ms / 64); kf.live = pctl + 0;
    HIPCHK(h, launch_contract(kf, st, h->contract_tile));
  }
  if ((e = tm.mark(h, st, &e3))) return e;
  if (rcount > 0) {
    AcqArgs ai = model;
    ai.mu_part = h->dmu_part[0] + i0; ai.w_part = h->dw_part[0] + i0; ai.ss_part = h->dss_part + i0; ai.Mc = Mc; ai.mcount = rcount;
    ai.m0 = m0 + i0; ai.live = pctl + 1;
    HIPCHK(h, launch_acquisition(ai, st));
    HIPCHK(h, launch_prune_update(h->dblk_val, h->dblk_idx, nblk_total, pctl + 1, 0, q, h->dbest_val, h->dbest_idx, st));
  }
  if (flush) {
    AcqArgs af = model;
    af.mu_part = h->dmu_part[1]; af.w_part = h->dw_part[1]; af.ss_part = cx.dss_surv; af.Mc = Ms; af.mcount = Ms; af.m0 = 0;
    af.live = pctl + 0; af.map = cx.pmap;
    HIPCHK(h, launch_acquisition(af, st));
    HIPCHK(h, launch_prune_update(h->dblk_val, h->dblk_idx, nblk_total, pctl + 0, 0, q, h->dbest_val, h->dbest_idx, st));
    HIPCHK(h, launch_prune_flushed(pctl, st));
    cx.prune_pending = 0;
  }
  if ((e = tm.mark(h, st, &e4))) return e;
  tm.span(T_CONTRACT, e2, e3); tm.span(T_CRITERIA, e3, e4);
  return BOGP_OK;
}

// What the chunk loop fills for a multi-target tail kernel (the model's half came with the request: multi_target_model): the arrays of
// the chunk at m0 on chunk buffer b, its geometry and the trend's scalars
static void multi_target_chunk(const bogp_handle* h, const SweepCtx& cx, int b, int64_t m0, int64_t mcount, MultiTargetChunk& a) {
  a.rT = h->drT[b]; a.ss_part = h->dss_part; a.w_part = h->dw_part[b]; a.S = cx.g.S; a.nJ = cx.nJ_main; a.Mc = cx.g.Mc;
  a.mcount = mcount; a.m0 = m0; a.beta = h->beta; a.G = h->G; a.estimate_trend = h->estimate_trend;
}

// Chunks [c_begin, c_end): producer -> contraction -> criteria (or the pruned flow).  pilot_done (a pruned sweep that began on the
// one-pass flow): thresholds, control words and the pilot rows' winners are in place -- chunk 0 starts behind the pilot.
// Two-stream mode (cx.overlap): the producer of chunk c + 1 runs on stP beside the contraction of chunk c, what it writes double buffered.
static int sweep_chunks(bogp_handle* h, SweepCtx& cx, int64_t c_begin, int64_t c_end, bool pilot_done) {
  const SweepRequest& rq = cx.rq;
  hipStream_t st = cx.st, stP = cx.stP;
  const int64_t M = cx.M, Mc = cx.g.Mc;
  const int Np = h->Np, S = cx.g.S;
  const bool overlap = cx.overlap, vx = cx.vx;
  const AcqArgs model = acq_model_args(h, rq, S, cx.nJ_main, cx.nblk_total);
  SpanTimer& tm = h->timer;
  int done[2] = {-1, -1};  // two-stream mode: chunk c leaves its last mark in [c & 1], where chunk c + 2 finds it
  for (int64_t c = c_begin; c < c_end; ++c) {
    const int b = overlap ? (int)(c & 1) : 0;
    int e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0;
    const int64_t m0 = c * Mc;
    const int64_t mcount = std::min<int64_t>(Mc, M - m0);
    const int64_t Mc_eff = ((mcount + 63) / 64) * 64;  // rows actually launched; array stride stays Mc
    CorrArgs ca = corr_chunk_args(h, cx.g, m0, b);
    if (cx.pv > 0) {
      ca.pv = cx.pv; ca.Wrow = h->dWpT; ca.wld = (h->p + 127) / 128 * 128; ca.t_part = h->dtpart[b];
    }
    ContractArgs ka;
    ka.rT = h->drT[b]; ka.Vp = vx ? h->dVpx : h->dVp; ka.ss_part = h->dss_part; ka.Mc = Mc; ka.nMt = (int)(Mc_eff / 64); ka.nJ = cx.nJ;
    ka.NJ16 = cx.NJ16; ka.NKP = cx.Nrows / 8;
    // producer: may reuse buffer b only after chunk c-2 (its previous user) is completely done
    if (overlap && c >= 2) HIPCHK(h, hipStreamWaitEvent(stP, tm.event(done[c & 1]), 0));
    // trend-rows models: k_trend_rows (below, on the producer stream) writes h->dmtrend, which is NOT double buffered -- chunk c - 1's
    // k_acquisition on the main stream must have read it first (without this wait chunk c - 1 could get chunk c's means)
    if (overlap && vx && c >= 1) HIPCHK(h, hipStreamWaitEvent(stP, tm.event(done[(c - 1) & 1]), 0));
    int e;  // lazily uploaded candidates: this chunk's rows must have arrived (chunk 0: copied here; later ones: below)
    if ((e = lazy_copy_to(h, m0 + mcount)) || (e = lazy_wait(h, stP)) || (stP != st && (e = lazy_wait(h, st)))) return e;
    if ((e = tm.mark(h, stP, &e0))) return e;
    const int64_t skip = pilot_done && c == 0 ? std::min<int64_t>(PRUNE_PILOT, mcount) : 0;  // (a multiple of 64)
    if (skip > 0) {
      ca.m0 += skip; ca.rT += skip; ca.mu_part += skip; ca.w_part += skip;
    }
    if (Mc_eff > skip) HIPCHK(h, launch_corr_chunk(h->kernel, ca, (int)((Mc_eff - skip) / 64), S, stP));
    if (vx) {  // rows Np .. Ne - 1 = 0 (their columns of the factor are zero: any FINITE value would do), rows Ne .. = -f(x*), then zeros
      if (h->vx_Ne > Np) HIPCHK(h, hipMemsetAsync(h->drT[b] + (size_t)Np * Mc, 0, (size_t)(h->vx_Ne - Np) * Mc * sizeof(double), stP));
      HIPCHK(h, launch_trend_rows(h->trend, h->dXs, m0, mcount, Mc_eff, h->d, Mc, h->dbetav, h->drT[b] + (size_t)h->vx_Ne * Mc, h->p,
                                  h->vx_Nt - h->vx_Ne, h->dmtrend, stP));
    }
    if ((e = tm.mark(h, stP, &e1))) return e;
    tm.span(T_PRODUCER, e0, e1);
    if (overlap) HIPCHK(h, hipStreamWaitEvent(st, tm.event(e1), 0));
    if (cx.prune) {
      if ((e = sweep_pruned_chunk(h, cx, model, ka, c, c_end, m0, mcount, skip, e1))) return e;
    } else {
      if ((e = tm.mark(h, st, &e2))) return e;
      // predict(X) without eval_MSE (gpr.py:486-491 returns before the triangular solve): the N^2 contraction is skipped
      // and k_acquisition sums zero variance groups (its MSE output is not read)
      if (rq.need_var) HIPCHK(h, launch_contract(ka, st, h->contract_tile));
      if ((e = tm.mark(h, st, &e3))) return e;
      AcqArgs aa = model;
      aa.mu_part = h->dmu_part[b]; aa.w_part = h->dw_part[b]; aa.ss_part = h->dss_part; aa.nJ = rq.need_var ? cx.nJ_main : 0; aa.Mc = Mc;
      aa.nJ_plus = vx ? cx.nJ - cx.nJ_main : 0;
      aa.mcount = mcount; aa.m0 = m0; aa.blk_offset = cx.blk_offset;
      if (h->p > 1 && (e = sweep_trend_chunk(h, cx, b, m0, mcount, Mc_eff, aa))) return e;
      if (rq.eh) {  // the m-target posterior + EHVI of this chunk in place of the q single-target criteria (kernels_ehvi.hip)
        EhviArgs ea = *rq.eh;
        multi_target_chunk(h, cx, b, m0, mcount, ea);
        ea.ehvi_out = h->dacq_out; ea.mu_out = rq.want_out ? h->dmu_out : nullptr; ea.mse_out = rq.want_out ? h->dmse_out : nullptr;
        ea.blk_val = h->dblk_val; ea.blk_idx = h->dblk_idx; ea.blk_offset = cx.blk_offset;
        HIPCHK(h, launch_ehvi(ea, st));
      } else if (rq.cn) {  // ... or the q feasibility-weighted criteria of the m-target posterior (kernels_constrained.hip)
        ConstrainedArgs cn = *rq.cn;
        multi_target_chunk(h, cx, b, m0, mcount, cn);
        cn.acq_out = h->dacq_out; cn.M = M; cn.mu_out = rq.want_out ? h->dmu_out : nullptr; cn.mse_out = rq.want_out ? h->dmse_out : nullptr;
        cn.blk_val = h->dblk_val; cn.blk_idx = h->dblk_idx; cn.blk_offset = cx.blk_offset; cn.nblk_total = cx.nblk_total;
        HIPCHK(h, launch_constrained(cn, st));
      } else if (rq.ec) {  // ... or EHVI of its objectives weighted by its constraints' feasibility (kernels_ehvi_constrained.hip)
        ConstrainedEhviArgs ec = *rq.ec;  // (its own field order: it does not hold MultiTargetChunk, bogp_internal.h)
        ec.rT = h->drT[b]; ec.ss_part = h->dss_part; ec.w_part = h->dw_part[b]; ec.S = S; ec.nJ = cx.nJ_main; ec.Mc = Mc;
        ec.mcount = mcount; ec.m0 = m0; ec.beta = h->beta; ec.G = h->G; ec.estimate_trend = h->estimate_trend;
        ec.val_out = h->dacq_out; ec.mu_out = rq.want_out ? h->dmu_out : nullptr; ec.mse_out = rq.want_out ? h->dmse_out : nullptr;
        ec.blk_val = h->dblk_val; ec.blk_idx = h->dblk_idx; ec.blk_offset = cx.blk_offset;
        HIPCHK(h, launch_ehvi_constrained(ec, st));
      } else {
        HIPCHK(h, launch_acquisition(aa, st));
      }
      if ((e = tm.mark(h, st, &e4))) return e;
      tm.span(T_CONTRACT, e2, e3); tm.span(T_CRITERIA, e3, e4);
      done[c & 1] = e4;
    }
    cx.blk_offset += (mcount + 255) / 256;
    if ((e = lazy_copy_to(h, m0 + mcount + Mc))) return e;  // the next chunk's rows travel while this chunk's kernels (queued above) run
  }
  return BOGP_OK;
}

// One pass: pilot -> pilot estimate -> per segment: producer without the store, bound, scan, survivor indices ->
// rounds.  Two fall-backs to sweep_chunks: the whole sweep where the pilot's own rows show that little can be pruned, one segment where
// too many of its rows survive.  The host waits twice per decision (survivors_of).
static int sweep_onepass(bogp_handle* h, SweepCtx& cx) {
  hipStream_t st = cx.st;
  const int64_t M = cx.M, Mc = cx.g.Mc, Ms = cx.Ms, nchunk = cx.g.nchunk, nblk_total = cx.nblk_total;
  const int S = cx.g.S, q = cx.rq.q, kernel = h->kernel;
  long long* const pctl = cx.pctl;
  const int64_t P = std::min<int64_t>(PRUNE_PILOT, Mc);  // (nchunk > 1: chunk 0 is a whole chunk)
  long long* const hcount = reinterpret_cast<long long*>(h->hfit + 3504);  // pinned: the one count the host waits for
  int e, w0 = 0, w1 = 0;  // (the marks around the whole sweep)
  // scan of the bound's block counts (and, index_from >= 0, the survivors' global indices in order); the host waits for the count
  // (`through`: the flagged rows are rows of that list -- S out of S1 -- and their entries of it are what is kept)
  auto survivors_of = [&](int64_t rows, int64_t index_from, long long* out, const unsigned char* flags, int64_t* sidx, const int64_t* through) -> int {
    HIPCHK(h, launch_prune_scan(cx.pblk_count, (rows + 255) / 256, cx.poffsets, rows, -1, pctl, st));
    if (index_from >= 0) HIPCHK(h, launch_prune_index(flags, cx.poffsets, rows, index_from, cx.sidx_cap, sidx, st, through));
    HIPCHK(h, hipMemcpyAsync(hcount, pctl + PRUNE_CTL_TOTAL, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    *out = *hcount;
    return BOGP_OK;
  };
  const CorrArgs cc = corr_chunk_args(h, cx.g, 0, 1);  // the survivor buffer's producer (Ms = Mc): the pilot, then every round
  ContractArgs kc;                                     // ... and its contraction
  kc.rT = h->drT[1]; kc.Vp = h->dVp; kc.ss_part = cx.dss_surv; kc.Mc = Ms; kc.nJ = cx.nJ; kc.NJ16 = cx.NJ16; kc.NKP = cx.Nrows / 8;
  AcqArgs aa = acq_model_args(h, cx.rq, S, cx.nJ_main, nblk_total);
  aa.mu_part = h->dmu_part[1]; aa.w_part = h->dw_part[1]; aa.ss_part = cx.dss_surv; aa.Mc = Ms; aa.m0 = 0;
  PruneBoundArgs pb = prune_bound_args(h, cx);
  Bound32Model md32{h->dX32, h->dvec32, h->dvec32 + h->Np, h->dvec32 + 2 * (size_t)h->Np, h->stats32[0], h->stats32[1], h->stats32[2]};
  int contract_launches = 0;
  // rows [0, cnt) of the survivor buffer (already produced) -> contraction, criteria (global indices through `map`, or m0 = 0), running best
  auto evaluate = [&](int64_t cnt, const int64_t* map) -> int {
    kc.nMt = (int)((cnt + 63) / 64);
    if (int e2 = timed_span(h, h->timer, st, T_CONTRACT, [&] { return launch_contract(kc, st, h->contract_tile); })) return e2;
    ++contract_launches;
    aa.mcount = cnt; aa.map = map;
    HIPCHK(h, launch_acquisition(aa, st));
    HIPCHK(h, launch_prune_update(h->dblk_val, h->dblk_idx, nblk_total, nullptr, cnt, q, h->dbest_val, h->dbest_idx, st));
    return BOGP_OK;
  };
  // a per-chunk path after all: chunks [c0, c1) behind the pilot, with the chunk buffer they need
  auto fall_back = [&](int64_t c0, int64_t c1, int path) -> int {
    int e2;
    if ((e2 = h->drT[0].ensure(h, (size_t)cx.Nrows * Mc))) return e2;
    if ((e2 = sweep_chunks(h, cx, c0, c1, true))) return e2;
    contract_launches += (int)(c1 - c0);
    h->prune_path = path;
    return BOGP_OK;
  };
  if ((e = h->timer.mark(h, st, &w0))) return e;
  HIPCHK(h, launch_prune_init(pctl, h->dbest_val, h->dbest_idx, q, P, st));
  if ((e = timed_span(h, h->timer, st, T_PRODUCER, [&] { return launch_corr_chunk(kernel, cc, (int)(P / 64), S, st); }))) return e;
  if ((e = evaluate(P, nullptr))) return e;
  // pilot estimate: the pilot's own rows against the thresholds they set -- what share of such rows the bound lets through
  long long pilot_surv = 0;
  pb.mu_part = h->dmu_part[1]; pb.w_part = h->dw_part[1]; pb.Mc = Ms; pb.rcount = P;
  HIPCHK(h, launch_prune_bound(pb, st));
  if ((e = survivors_of(P, -1, &pilot_surv, cx.pflags, cx.psidx, nullptr))) return e;
  if (prune_decide(P, pilot_surv, 1, 0) == BOGP_PRUNE_PATH_CHUNKS) {
    if ((e = fall_back(0, nchunk, BOGP_PRUNE_PATH_CHUNKS))) return e;
  } else {
    h->prune_path = BOGP_PRUNE_PATH_ONEPASS;
    for (int64_t s0 = 0; s0 < M; s0 += cx.seg_rows) {
      const int64_t sb = std::max<int64_t>(P, s0), se = std::min<int64_t>(M, s0 + cx.seg_rows), rows = se - sb;
      if (rows <= 0) continue;
      CorrArgs cs = cc;  // the segment's partial sums, nothing else
      cs.m0 = sb; cs.Mc = cx.seg_stride; cs.rT = nullptr; cs.store = false; cs.mu_part = h->dmu_part[0]; cs.w_part = h->dw_part[0];
      pb.mu_part = h->dmu_part[0]; pb.w_part = h->dw_part[0]; pb.Mc = cx.seg_stride;
      long long surv = 0, s1 = -1;
      if (cx.bound32) {
        // stage 1: every row from FP32 sums, flagged unless its margins rule it out -> S1, a superset of the survivors
        Bound32Args ba;
        ba.Xs = h->dXs; ba.M = M; ba.m0 = sb; ba.rcount = rows; ba.d = h->d; ba.Np = h->Np; ba.sqrt_theta = h->dsqrt_theta;
        ba.estimate_trend = pb.estimate_trend;
        ba.md = md32; ba.mu = cx.pmu32; ba.wd = cx.pwd32; ba.na = cx.pna32;
        if ((e = timed_span(h, h->timer, st, T_PRODUCER, [&] { return launch_bound32_sums(kernel, ba, st); }))) return e;
        PruneBoundArgs p1 = pb;
        p1.mu_part = cx.pmu32; p1.w_part = cx.pwd32; p1.S = 1; p1.Mc = rows; p1.rcount = rows; p1.flags = cx.pflags1;
        HIPCHK(h, launch_bound32_flags(p1, kernel, h->d, cx.pwd32, cx.pna32, md32, st));
        if ((e = survivors_of(rows, sb, &s1, cx.pflags1, cx.psidx1, nullptr))) return e;
        h->b32_rows += rows; h->b32_kept += s1; h->b32_last_rows = rows;
        if (4 * s1 > rows) {  // the exact pass over the whole segment after all: the FP32 pass was wasted
          ++h->b32_fallbacks;
          s1 = -1;
        }
      }
      if (s1 < 0) {
        if ((e = timed_span(h, h->timer, st, T_PRODUCER, [&] { return launch_corr_chunk(kernel, cs, (int)((rows + 63) / 64), S, st); }))) return e;
        pb.rcount = rows;
        HIPCHK(h, launch_prune_bound(pb, st));
        if ((e = survivors_of(rows, sb, &surv, cx.pflags, cx.psidx, nullptr))) return e;
      } else if (s1 > 0) {
        // stage 2: the exact sums of S1's rows alone (a row's sums do not depend on its neighbours), the exact bound, S in the original order
        HIPCHK(h, launch_prune_rows(h->dXs, cx.psidx1, s1, h->d, cx.pxc1, st));
        cs.Xs = cx.pxc1; cs.M = s1; cs.m0 = 0;
        if ((e = timed_span(h, h->timer, st, T_PRODUCER, [&] { return launch_corr_chunk(kernel, cs, (int)((s1 + 63) / 64), S, st); }))) return e;
        pb.rcount = s1;
        HIPCHK(h, launch_prune_bound(pb, st));
        if ((e = survivors_of(s1, 0, &surv, cx.pflags, cx.psidx, cx.psidx1))) return e;
      }
      if (prune_decide(P, pilot_surv, rows, surv) == BOGP_PRUNE_PATH_ONEPASS_FALLBACK) {  // (needs ordered candidates: the pilot saw few such rows)
        if ((e = fall_back(sb / Mc, (se + Mc - 1) / Mc, BOGP_PRUNE_PATH_ONEPASS_FALLBACK))) return e;
        continue;
      }
      for (int64_t k0 = 0; k0 < surv; k0 += Ms) {  // rounds of at most one survivor buffer, in the survivors' order
        const int64_t cnt = std::min<int64_t>(Ms, surv - k0);
        HIPCHK(h, launch_prune_rows(h->dXs, cx.psidx + k0, cnt, h->d, cx.pxc, st));
        CorrArgs cr = cc;
        cr.Xs = cx.pxc; cr.M = cnt;
        if ((e = timed_span(h, h->timer, st, T_PRODUCER, [&] { return launch_corr_chunk(kernel, cr, (int)((cnt + 63) / 64), S, st); }))) return e;
        if ((e = evaluate(cnt, cx.psidx + k0))) return e;
        ++h->prune_rounds;
      }
      h->prune_survivors += surv;
    }
  }
  if ((e = h->timer.mark(h, st, &w1))) return e;
  h->timer.span(T_WHOLE, w0, w1);
  h->n_chunks = contract_launches;
  return BOGP_OK;
}

int bogp::run_sweep(bogp_handle* h, const SweepRequest& rq) {
  collect_timing(h);  // the events are about to be re-recorded
  h->timer.begin();
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "no committed model: call bogp_commit first");
  if (!h->dXs || h->M <= 0) FAIL(h, BOGP_ERR_INVALID, "no candidates: call bogp_candidates_upload/bind first");
  if (rq.q < 0 || rq.q > BOGP_MAX_Q) FAIL(h, BOGP_ERR_INVALID, "q = %d outside [0, %d]", rq.q, BOGP_MAX_Q);
  HIPCHK(h, hipSetDevice(h->device));
  const int Np = h->Np, q = rq.q;
  const int64_t M = h->M;
  h->prune_path = BOGP_PRUNE_PATH_NONE; h->prune_survivors = 0; h->prune_rounds = 0;
  h->b32_rows = h->b32_kept = h->b32_last_rows = 0; h->b32_fallbacks = 0;
  int e;
  // the two single-target shortcuts (the multi-target requests -- bogp_sweep_ehvi: eh non-null, bogp_sweep_constrained: cn non-null,
  // bogp_sweep_ehvi_constrained: ec non-null -- take neither: they always run the chunked path below); nothing to overlap a lazy upload
  // with: the whole upload first (one launch reads every candidate)
  const bool multi = rq.eh || rq.cn || rq.ec;
  const bool small_batch = !multi && M <= 32 && h->p == 1;
  if (small_batch || (!multi && h->p == 1 && sweep_small_supported(Np, h->d, h->kernel))) {
    if ((e = lazy_finish(h))) return e;
    return small_batch ? sweep_small_batch(h, rq) : sweep_one_launch(h, rq);
  }
  SweepCtx cx{};
  cx.rq = rq; cx.M = M; cx.st = h->stream;
  // trend-rows path (k_pack_Vx): the chunk carries Nt - Np extra rows (the hole up to a whole column group, then -f(x*)), the contraction
  // runs over the extended factor
  cx.vx_model = h->vx_Nt > 0 && h->p >= trend_rows_min() && h->estimate_trend;  // the committed model takes the trend-rows path ...
  cx.vx = cx.vx_model && rq.need_var;                                            // ... and this call needs the variance
  cx.Nrows = cx.vx ? h->vx_Nt : Np;
  if ((e = sweep_geometry(h, cx.Nrows, &cx.g))) return e;
  const int64_t nchunk = cx.g.nchunk;
  if (nchunk == 1 && (e = lazy_finish(h))) return e;  // (as above)
  const int cols = contract_cols_per_group();
  cx.NJ16 = cx.Nrows / 16;
  cx.nJ_main = (Np + cols - 1) / cols;                             // column groups of V: |L^-1 r|^2
  cx.nJ = cx.vx ? (cx.Nrows + cols - 1) / cols : cx.nJ_main;       // ... + the groups of the trend rows: |u|^2
  cx.nblk_total = (M + 255) / 256 + nchunk;
  // a polynomial basis of at most 32 columns under universal kriging: T = W^T r is accumulated by the producer itself
  // (k_corr_chunk<K, PV>) and finished by ONE per-candidate launch (k_trend_small); (the tile products it replaces: git 3357059)
  // (a mean-only call of a trend-rows model keeps the producer the full call uses -- pv = 0 -- so that mu comes out bit-identical)
  cx.pv = (!cx.vx_model && h->p > 1 && h->estimate_trend) ? corr_trend_columns(h->p) : 0;
  // Optional two-stream mode (BOGP_OVERLAP=1): the correlation producer of chunk c+1 (FP64 VALU) runs beside the
  // contraction of chunk c (FP64 MFMA), everything the producer writes double buffered.  Measured on MI355X (r01,
  // C3): the kernels do overlap (contract 75.9 -> 81.9 ms, corr 6.8 -> 11.7 ms) but the step time is unchanged
  // (83.3 -> 83.0 ms): the DP pipe is the shared resource.  Off by default: it costs a second 1-GiB chunk buffer.
  cx.overlap = nchunk > 1 && getenv("BOGP_OVERLAP") && atoi(getenv("BOGP_OVERLAP")) == 1;
  cx.stP = cx.overlap ? h->stream2 : cx.st;
  // Pruned sweep (kernels_prune.hip): only the winners leave this call, so a row whose criteria cannot reach the best
  // values found so far even with ss = 0 skips the contraction.  Everything else -- value outputs, polynomial bases, EHVI, modelled constraints -- runs as ever.
  cx.prune = h->prune_mode != 0 && rq.need_var && q > 0 && !rq.want_out && !rq.want_acq_out && !multi && h->p == 1 && !cx.vx_model && !cx.overlap;
  // one pass: every candidate resident and a producer that exists without its store
  cx.onepass = cx.prune && h->prune_mode == 1 && nchunk > 1 && !h->hXs_lazy && corr_chunk_without_store(h->kernel, 0, h->dXnorm != nullptr);
  // ... bounded in FP32 first where the kernel's profile has a bounded slope
  cx.bound32 = cx.onepass && h->prune_bound32 != 0 && bound32_supported(h->kernel, h->d);
  if (cx.bound32 && (h->b32_gen != h->commit_gen || h->b32_target != h->target) && (e = bound32_prepare(h))) return e;  // (another target since the commit)
  if ((e = sweep_workspace(h, cx))) return e;
  if ((e = ensure_sweep_outputs(h, q, cx.nblk_total, rq.want_out ? (size_t)M * rq.targets() : 0, rq.want_acq_out))) return e;
  if (cx.overlap) {  // the producer stream must see everything queued on the main stream so far (commit, uploads)
    int b0 = 0;
    if ((e = h->timer.mark(h, cx.st, &b0))) return e;
    HIPCHK(h, hipStreamWaitEvent(cx.stP, h->timer.event(b0), 0));
  }
  if (!cx.onepass) {
    if ((e = sweep_chunks(h, cx, 0, nchunk, false))) return e;
    if (cx.prune) h->prune_path = BOGP_PRUNE_PATH_CHUNKS;
    h->n_chunks = (int)nchunk;
  } else if ((e = sweep_onepass(h, cx))) {
    return e;
  }
  // every row is on its way; once the copy stream is idle the caller's buffer is no longer needed
  if ((e = lazy_finish(h))) return e;
  // (a pruned sweep kept its running best in dbest_* all along)
  if (q > 0 && !cx.prune) HIPCHK(h, launch_argmax_final(h->dblk_val, h->dblk_idx, cx.blk_offset, cx.nblk_total, q, h->dbest_val, h->dbest_idx, cx.st));
  h->timing_pending = true; h->prune_used = cx.prune;
  h->contracted_rows = rq.need_var ? M : 0;
  if (rq.sync || cx.overlap) HIPCHK(h, hipStreamSynchronize(cx.st));
  if (cx.overlap) HIPCHK(h, hipStreamSynchronize(cx.stP));
  return BOGP_OK;
}

extern "C" int bogp_predict(bogp_handle* h, double* mu, double* mse) {
  if (!h) return BOGP_ERR_INVALID;
  if (!mu) FAIL(h, BOGP_ERR_INVALID, "bogp_predict: mu must be non-null");
  SweepRequest rq;
  rq.want_out = true; rq.need_var = mse != nullptr;
  if (int rc = run_sweep(h, rq)) return rc;
  HIPCHK(h, hipMemcpy(mu, h->dmu_out, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost));
  if (mse) HIPCHK(h, hipMemcpy(mse, h->dmse_out, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}

extern "C" int bogp_sweep(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                          double* best_val, int64_t* best_idx, double* acq_out) {
  if (!h) return BOGP_ERR_INVALID;
  if (q <= 0 || !acq_id || (!best_val != !best_idx)) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep: q > 0, non-null acq_id, and best_val / best_idx both given or both NULL");
  const bool local = best_val != nullptr;  // NULL outputs: the winners stay on the device for bogp_exchange_argmax
  if (!local && acq_out) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep: acq_out needs best_val / best_idx");
  int rc;
  if ((rc = check_criteria(h, q, acq_id, acq_par))) return rc;
  invalidate_sweep_results(h);
  SweepRequest rq;
  rq.q = q; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin; rq.minimize = minimize; rq.want_acq_out = acq_out != nullptr; rq.sync = local;
  if ((rc = run_sweep(h, rq))) return rc;
  h->last_q = q;  // dbest_val / dbest_idx hold this sweep's winners for bogp_exchange_argmax
  if (!local) return BOGP_OK;  // queued, not waited for: the exchange that follows is ordered behind it on the stream
  HIPCHK(h, hipMemcpy(best_val, h->dbest_val, q * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(best_idx, h->dbest_idx, q * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (acq_out) HIPCHK(h, hipMemcpy(acq_out, h->dacq_out, (size_t)q * h->M * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}

extern "C" int bogp_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                               int k, double* best_val, int64_t* best_idx) {
  if (!h) return BOGP_ERR_INVALID;
  if (k <= 0 || k > BOGP_MAX_TOPK) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_topk: k = %d outside [1, %d]", k, BOGP_MAX_TOPK);
  if (q <= 0 || !acq_id || !best_val || !best_idx) FAIL(h, BOGP_ERR_INVALID, "bogp_sweep_topk: q > 0 and non-null acq_id/best_val/best_idx required");
  int rc;
  if ((rc = check_criteria(h, q, acq_id, acq_par))) return rc;
  invalidate_sweep_results(h);  // run_sweep below overwrites dbest_* as well
  SweepRequest rq;  // (want_acq_out: keeps the q x M values on the device)
  rq.q = q; rq.acq_id = acq_id; rq.acq_par = acq_par; rq.plugin = plugin; rq.minimize = minimize; rq.want_acq_out = true;
  if ((rc = run_sweep(h, rq))) return rc;
  // the k ranks of every criterion (rank 0 repeats the sweep's own argmax) and ONE read-back of q x k (value, index) pairs
  hipStream_t st = h->stream;
  if ((rc = rank_stored_values(h, h->dacq_out, h->M, q, k, st))) return rc;
  HIPCHK(h, hipMemcpyAsync(best_val, h->dtopk_val, (size_t)q * k * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(best_idx, h->dtopk_idx, (size_t)q * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->last_topk_q = q;
  h->last_topk_k = k;
  pad_short_ranks(best_val, best_idx, q * k);
  return BOGP_OK;
}

extern "C" int bogp_last_timing(bogp_handle* h, double* corr_ms, double* contract_ms, double* acquisition_ms, int* n_chunks) {
  if (!h) return BOGP_ERR_INVALID;
  collect_timing(h);
  if (corr_ms) *corr_ms = h->t_corr_ms;
  if (contract_ms) *contract_ms = h->t_contract_ms;
  if (acquisition_ms) *acquisition_ms = h->t_acq_ms;
  if (n_chunks) *n_chunks = h->n_chunks;
  return BOGP_OK;
}

extern "C" int bogp_set_prune(bogp_handle* h, int on) {
  if (!h) return BOGP_ERR_INVALID;
  if (on < 0 || on > 2) FAIL(h, BOGP_ERR_INVALID, "bogp_set_prune: %d is none of 0 (off), 1 (automatic), 2 (per-chunk path)", on);
  h->prune_mode = on;
  return BOGP_OK;
}

// FP32 copies of the committed model for the bounding stage (kernels_bound32.hip): at commit, and for another target on demand
int bogp::bound32_prepare(bogp_handle* h) {
  if (!h->committed || h->p != 1 || !h->dXnorm || !bound32_supported(h->kernel, h->d)) return BOGP_OK;
  const int d = h->d, Np = h->Np;
  hipStream_t st = h->stream;
  int e;
  if ((e = h->dX32.ensure(h, (size_t)4 * ((d + 3) / 4) * Np)) || (e = h->dvec32.ensure(h, (size_t)3 * Np))) return e;
  if ((e = h->dstats32.ensure(h, 3))) return e;
  HIPCHK(h, launch_bound32_prepare(h->kernel, h->dXthT, h->dXnorm, h->dgamma, h->dw, d, Np, h->dX32, h->dvec32, h->dstats32, st));
  HIPCHK(h, hipMemcpyAsync(h->stats32, h->dstats32, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->b32_gen = h->commit_gen; h->b32_target = h->target;
  return BOGP_OK;
}

extern "C" int bogp_set_prune_bound32(bogp_handle* h, int on) {
  if (!h) return BOGP_ERR_INVALID;
  if (on != 0 && on != 1) FAIL(h, BOGP_ERR_INVALID, "bogp_set_prune_bound32: %d is neither 0 (off) nor 1 (on)", on);
  h->prune_bound32 = on;
  return BOGP_OK;
}

extern "C" int bogp_last_bound32(bogp_handle* h, int64_t* rows, int64_t* kept, int* fallbacks) {
  if (!h) return BOGP_ERR_INVALID;
  if (rows) *rows = h->b32_rows;
  if (kept) *kept = h->b32_kept;
  if (fallbacks) *fallbacks = h->b32_fallbacks;
  return BOGP_OK;
}

extern "C" int bogp_debug_bound32(bogp_handle* h, int64_t cap, double* mu32, double* e_mu, double* wd32, double* e_w, unsigned char* flags, int64_t* rows) {
  if (!h) return BOGP_ERR_INVALID;
  if (!rows) FAIL(h, BOGP_ERR_INVALID, "bogp_debug_bound32: null row count");
  *rows = h->b32_last_rows;
  const int64_t n = h->b32_last_rows;
  if (n == 0 || !(mu32 || e_mu || wd32 || e_w || flags)) return BOGP_OK;
  if (cap < n) FAIL(h, BOGP_ERR_INVALID, "bogp_debug_bound32: %lld rows, room for %lld", (long long)n, (long long)cap);
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the work space as sweep_workspace carved it for the last sweep: the three per-row arrays end it, the flags sit in front of them
  const int64_t Rmax = (int64_t)(h->b32_ws_rmax);
  const double* base = (const double*)(h->dprune + h->b32_ws_row32);
  std::vector<double> na((size_t)n);
  HIPCHK(h, hipMemcpy(na.data(), base + 2 * Rmax, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (mu32) HIPCHK(h, hipMemcpy(mu32, base, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (wd32) HIPCHK(h, hipMemcpy(wd32, base + Rmax, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  if (flags) HIPCHK(h, hipMemcpy(flags, h->dprune + h->b32_ws_flag1, (size_t)n, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; ++i) {
    double a = 0, b = 0;
    bound32_margin(h->kernel, h->d, na[(size_t)i], h->stats32[2], h->stats32[0], h->stats32[1], &a, &b);
    if (e_mu) e_mu[i] = a;
    if (e_w) e_w[i] = b;
  }
  return BOGP_OK;
}

// host evaluations of the FP32 stage's margin and interval bound (csrc/bogp_device.h): no device, no handle; tests/test_bound32_host.py
extern "C" int bogp_bound32_margin(int kernel, int d, double na, double nb_max, double gamma_l1, double w_l1, double* e_mu, double* e_w) {
  if (!e_mu || !e_w) return BOGP_ERR_INVALID;
  bound32_margin(kernel, d, na, nb_max, gamma_l1, w_l1, e_mu, e_w);
  return BOGP_OK;
}
extern "C" double bogp_acq_upper_bound_interval(int acq_id, double acq_par, double y_hat, double e, double sd_ub, double plugin, double sigma2) {
  return acq_upper_bound_interval(acq_id, acq_par, y_hat, e, sd_ub, plugin, sigma2);
}

extern "C" int bogp_last_prune_path(bogp_handle* h, int* path, int64_t* survivors, int* rounds) {
  if (!h) return BOGP_ERR_INVALID;
  if (path) *path = h->prune_path;
  if (survivors) *survivors = h->prune_survivors;
  if (rounds) *rounds = h->prune_rounds;
  return BOGP_OK;
}

extern "C" int bogp_prune_decide(int64_t pilot_rows, int64_t pilot_survivors, int64_t segment_rows, int64_t segment_survivors) {
  return prune_decide(pilot_rows, pilot_survivors, segment_rows, segment_survivors);
}
extern "C" int64_t bogp_sweep_chunk_rows(int64_t rows, int64_t M, int64_t chunk_bytes) { return sweep_chunk_rows(rows, M, chunk_bytes); }

extern "C" int bogp_last_contracted_rows(bogp_handle* h, int64_t* rows) {
  if (!h) return BOGP_ERR_INVALID;
  if (!rows) FAIL(h, BOGP_ERR_INVALID, "bogp_last_contracted_rows: null output");
  *rows = h->contracted_rows;
  if (h->prune_used && h->dprune) {  // the count of a pruned sweep never left the device: wait for the sweep, read it
    HIPCHK(h, hipSetDevice(h->device));
    long long n = 0;
    HIPCHK(h, hipMemcpyAsync(&n, h->dprune + PRUNE_CTL_CONTRACTED, sizeof(n), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *rows = (int64_t)n + h->prune_survivors;  // (+ the rows the one-pass rounds contracted: the host knows those)
  }
  return BOGP_OK;
}

extern "C" int bogp_set_contract_tile(bogp_handle* h, int rows) {
  if (!h) return BOGP_ERR_INVALID;
  if (rows != 0 && rows != 16 && rows != 32 && rows != 64) FAIL(h, BOGP_ERR_INVALID, "bogp_set_contract_tile: %d is none of 0 (automatic), 16, 32, 64", rows);
  h->contract_tile.forced = rows;
  return BOGP_OK;
}
extern "C" int bogp_last_contract_tile(bogp_handle* h, int* rows) {
  if (!h) return BOGP_ERR_INVALID;
  if (!rows) FAIL(h, BOGP_ERR_INVALID, "bogp_last_contract_tile: null output");
  *rows = h->contract_tile.last;
  return BOGP_OK;
}
extern "C" int bogp_contract_tile_rows(int64_t row_tiles64, int nJ, int n_cu, int live) { return contract_tile_rows(row_tiles64, nJ, n_cu, live != 0); }

// host evaluations of the pruned sweep's bound and test (csrc/bogp_device.h): no device, no handle; tests/test_prune_bounds_host.py
extern "C" double bogp_acq_upper_bound(int acq_id, double acq_par, double y_hat, double sd_ub, double plugin, double sigma2) {
  return acq_upper_bound(acq_id, acq_par, y_hat, sd_ub, plugin, sigma2);
}
extern "C" int bogp_prune_below(double bound, double threshold) { return prune_below(bound, threshold) ? 1 : 0; }

extern "C" double bogp_flops_per_candidate(const bogp_handle* h) {
  if (!h || !h->committed) return 0.0;
  const double N = h->N, d = h->d, p = h->estimate_trend ? 1 : 0;
  return N * N + N * (3 * d + 5 + 2 * p);
}

// ------------------------------------------------------------------------------------------------------
// gradient of the posterior at one point (gpr.py:537-576)
// ------------------------------------------------------------------------------------------------------
extern "C" int bogp_gradient(bogp_handle* h, const double* x, double* dmu, double* dmse) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "bogp_gradient: no committed model");
  if (h->kernel == BOGP_KERNEL_CUBIC || h->kernel == BOGP_KERNEL_GENEXP || h->kernel == BOGP_KERNEL_MATERN_NU) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_gradient: the cubic correlation has no input-derivative (corr_dx leaves it undefined in the reference, gpr.py:655-658)");
  if (!x || !dmu || !dmse) FAIL(h, BOGP_ERR_INVALID, "bogp_gradient: null pointer");
  const int N = h->N, d = h->d;
  hipStream_t st = h->stream;
  HIPCHK(h, hipSetDevice(h->device));
  const int pt = h->p;
  if (pt == 1)  // constant basis: k_point_rhs + k_point_tri, no library call (kernels_point.hip)
    return point_eval_host(h, "bogp_gradient", x, 1, 0, nullptr, nullptr, 0.0, 1, nullptr, nullptr, dmu, dmse, nullptr, nullptr);
  if (pt > 1 && h->trend == BOGP_TREND_QUADRATIC)
    FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_gradient: the quadratic trend has no Jacobian in the reference either (trend.py:138-139)");
  int e = h->dgrad_partial.ensure(h, (size_t)N * (d + 3) + 4 * d + 8 + (size_t)pt * (d + 1));
  if (e) return e;
  double* dr = h->dgrad_partial;            // N
  double* drdx = dr + N;                    // d x N (column k = dr/dx_k); [r | dr/dx] is one N x (d+1) column-major matrix
  double* dz = drdx + (size_t)N * d;        // N
  double* dx = dz + N;                      // d
  double* dout = dx + d;                    // 3 d
  double* dtw = dout + 3 * d + 8;           // p x (d+1): W^T [r | dr/dx]
  double* dvr = dtw + (size_t)pt * (d + 1);  // N: V r
  HIPCHK(h, hipMemcpyAsync(dx, x, d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_point_corr(h->kernel, h->dX, N, d, h->dtheta, dx, dr, drdx, st));
  // z = L^-T L^-1 r = V^T (V r) with the explicit V = L^-1 kept from the commit: two triangular matrix-vector
  // products (bandwidth bound, ~50 us at N = 2048) instead of two dependent triangular solves (~350 us each)
  HIPCHK(h, launch_gemm(0, 0, N, 1, N, 1.0, h->dV, h->ldr, dr, N, 0.0, dvr, N, st, 1));  // V r
  HIPCHK(h, launch_gemm(1, 0, N, 1, N, 1.0, h->dV, h->ldr, dvr, N, 0.0, dz, N, st, 2));  // V^T (V r)
  const double one = 1.0, zero = 0.0;
  HIPCHK(h, launch_gemm(1, 0, d, 1, N, one, drdx, N, h->dgamma, N, zero, dout, d, st, 0, &h->gsplit));
  HIPCHK(h, launch_gemm(1, 0, d, 1, N, one, drdx, N, dz, N, zero, dout + d, d, st, 0, &h->gsplit));
  std::vector<double> out(3 * d, 0.0), tw;
  if (h->estimate_trend && pt > 1) {  // (Ft^T L^-1) [r | dr/dx] = W^T [r | dr/dx]   (gpr.py:570-571)
    HIPCHK(h, launch_gemm(1, 0, pt, d + 1, N, one, h->dWp, h->Np, dr, N, zero, dtw, pt, st, 0, &h->gsplit));
    tw.resize((size_t)pt * (d + 1));
    HIPCHK(h, hipMemcpyAsync(tw.data(), dtw, tw.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipMemcpyAsync(out.data(), dout, 2 * d * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  {  // linear basis (the constant one returned above): f = [1, x], Jacobian rows 1..d = identity (trend.py:104-112)
    std::vector<double> su;  // S u with u = Ft^T rt - f and S = (Ft^T Ft)^-1 (:570-573)
    if (h->estimate_trend) {
      std::vector<double> u(pt);
      for (int c = 0; c < pt; ++c) u[c] = tw[c] - (c == 0 ? 1.0 : x[c - 1]);
      su.assign(pt, 0.0);
      for (int c = 0; c < pt; ++c)
        for (int r = 0; r < pt; ++r) su[r] += h->h_Sinv[(size_t)c * pt + r] * u[c];  // S symmetric, column-major
    }
    for (int k = 0; k < d; ++k) {
      dmu[k] = h->h_betav[1 + k] + out[k];  // beta^T f_dx + gamma^T r_dx (:561)
      double m = -1.0 * out[d + k];
      if (h->estimate_trend) {
        double acc = 0.0;
        for (int c = 0; c < pt; ++c) acc += su[c] * (tw[(size_t)(1 + k) * pt + c] - (c == 1 + k ? 1.0 : 0.0));  // u_dx = Ft^T rt_dx - f_dx
        m += acc;
      }
      dmse[k] = 2.0 * h->sigma2 * m;
    }
  }
  return BOGP_OK;
}

// Hessian of the posterior mean at x (GaussianProcess.Hessian, gpr.py:578-598): f_dx2 . beta + r_dx2 . gamma.  The trend
// part is zero for the constant and linear bases (trend.py:88-91, 113-116; the quadratic one raises); the correlation part
// exists for the squared exponential only (corr_Hessian, :663-734, leaves H undefined for every other kernel).
extern "C" int bogp_hessian(bogp_handle* h, const double* x, double* H) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "bogp_hessian: no committed model");
  if (!x || !H) FAIL(h, BOGP_ERR_INVALID, "bogp_hessian: null pointer");
  if (h->kernel != BOGP_KERNEL_SE) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_hessian: squared exponential only (the reference's corr_Hessian defines no other kernel)");
  if (h->trend == BOGP_TREND_QUADRATIC) FAIL(h, BOGP_ERR_UNSUPPORTED, "bogp_hessian: the quadratic trend has no Hessian in the reference (trend.py:141-142)");
  const int N = h->N, d = h->d;
  hipStream_t st = h->stream;
  HIPCHK(h, hipSetDevice(h->device));
  int e = h->dgrad_partial.ensure(h, (size_t)N * (d + 1) + d + (size_t)d * d);
  if (e) return e;
  double* dr = h->dgrad_partial;
  double* drdx = dr + N;
  double* dx = drdx + (size_t)N * d;
  double* dH = dx + d;
  HIPCHK(h, hipMemcpyAsync(dx, x, d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_point_corr(h->kernel, h->dX, N, d, h->dtheta, dx, dr, drdx, st));
  HIPCHK(h, launch_point_hessian(h->dX, N, d, h->dtheta, dx, dr, drdx, h->dgamma, dH, st));
  HIPCHK(h, hipMemcpyAsync(H, dH, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return BOGP_OK;
}

// Correlation between the rows of X1 at the committed theta (GaussianProcess.prior_cov(X1, corr=True), gpr.py:318-353;
// its X2 argument cannot be used in the reference: `if X2` on an array raises).  R is n1 x n1, row-major.
extern "C" int bogp_prior_corr(bogp_handle* h, const double* X1, int n1, double* R) {
  if (!h) return BOGP_ERR_INVALID;
  if (!h->committed) FAIL(h, BOGP_ERR_INVALID, "bogp_prior_corr: no committed model");
  if (!X1 || !R || n1 <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_prior_corr: X1 / R must be non-null and n1 > 0");
  const int d = h->d;
  hipStream_t st = h->stream;
  HIPCHK(h, hipSetDevice(h->device));
  int e = h->dbatch.ensure(h, (size_t)n1 * d + 2 * (size_t)n1 * n1);
  if (e) return e;
  double* dX1 = h->dbatch;
  double* dr = dX1 + (size_t)n1 * d;
  double* ds2 = dr + (size_t)n1 * n1;
  HIPCHK(h, hipMemcpyAsync(dX1, X1, (size_t)n1 * d * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(h, launch_batch_corr(h->kernel, dX1, n1, d, h->dtheta, dX1, n1, dr, ds2, st));
  HIPCHK(h, hipMemcpyAsync(R, dr, (size_t)n1 * n1 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  return BOGP_OK;
}

// ------------------------------------------------------------------------------------------------------
// self test of kernels_gemm.hip on host buffers (include/bogp.h)
// ------------------------------------------------------------------------------------------------------
#ifdef NS_PROFILE
// (profiling builds only, `make EXTRA=-DNS_PROFILE`: the 64 scalars of the last polled read-back / of the device block, incl. the
// clock words a profiled kernel leaves -- tools/prof_nll_small_phases.py)
extern "C" int bogp_debug_fit_scalars(bogp_handle* h, double* out) {
  if (!h || !out) return BOGP_ERR_INVALID;
  memcpy(out, h->hfit + 2048, 64 * sizeof(double));
  return BOGP_OK;
}

extern "C" int bogp_debug_dscal(bogp_handle* h, double* out) {
  if (!h || !out) return BOGP_ERR_INVALID;
  HIPCHK(h, hipMemcpy(out, h->dscal, 64 * sizeof(double), hipMemcpyDeviceToHost));
  return BOGP_OK;
}
#endif

#ifdef ELIM_PROFILE
// (profiling builds only, `make EXTRA=-DELIM_PROFILE`: the wall-clock stamps the fused elimination step leaves -- tools/probes/elim_stamps.py)
namespace bogp { hipError_t debug_elim_stamps(unsigned long long* out); }
extern "C" int bogp_debug_elim_stamps(unsigned long long* out) { return bogp::debug_elim_stamps(out) == hipSuccess ? BOGP_OK : BOGP_ERR_HIP; }
#endif

#ifdef CONTRACT_D_TRACE
// (profiling builds only, -DCONTRACT_D_TRACE: the stamps the largest k_contract16d launch left -- tools/contract_d_trace.py)
namespace bogp { hipError_t debug_contract_trace(unsigned long long* out, size_t cap_words, size_t* used_words, int* dims); }
extern "C" int bogp_debug_contract_trace(unsigned long long* out, size_t cap_words, size_t* used_words, int* dims) {
  return bogp::debug_contract_trace(out, cap_words, used_words, dims) == hipSuccess ? BOGP_OK : BOGP_ERR_HIP;
}
#endif

extern "C" int bogp_selftest_gemm(bogp_handle* h, int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda,
                                  const double* B, int ldb, double beta, double* C, int ldc, int tri, int split) {
  if (!h) return BOGP_ERR_INVALID;
  if (!A || !B || !C || m <= 0 || n <= 0 || k <= 0) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_gemm: null pointer or empty shape");
  if (lda < (ta ? k : m) || ldb < (tb ? n : k) || ldc < m) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_gemm: leading dimension below the stored rows");
  if (tri && m != k) FAIL(h, BOGP_ERR_INVALID, "bogp_selftest_gemm: a triangular op(A) is square");
  HIPCHK(h, hipSetDevice(h->device));
  hipStream_t st = h->stream;
  const size_t na = (size_t)lda * (ta ? m : k), nb = (size_t)ldb * (tb ? k : n), nc = (size_t)ldc * n;
  DevBuf<double> dA, dB, dC;
  int rc = BOGP_OK;
  if (split && (rc = ensure_gsplit(h))) return rc;
  if (dA.ensure(h, na) || dB.ensure(h, nb) || dC.ensure(h, nc)) FAIL(h, BOGP_ERR_HIP, "bogp_selftest_gemm: hipMalloc failed");
  hipError_t e = hipMemcpyAsync(dA, A, na * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dB, B, nb * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dC, C, nc * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_gemm(ta, tb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, st, tri, split ? &h->gsplit : nullptr);
  if (e == hipSuccess) e = hipMemcpyAsync(C, dC, nc * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) FAIL(h, BOGP_ERR_HIP, "bogp_selftest_gemm: %s", hipGetErrorString(e));
  return BOGP_OK;
}
