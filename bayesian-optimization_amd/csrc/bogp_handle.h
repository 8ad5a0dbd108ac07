// bogp_handle.h -- the device state behind an opaque bogp_handle (include/bogp.h), the three types that own its device memory,
// pinned blocks and events (DevBuf, MappedBuf, EventPool), the span ledger of its event timing (SpanTimer), and the error plumbing shared
// by the translation units that implement the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bogp.h"
#include "bogp_internal.h"

struct bogp_handle;
namespace bogp {
void comm_release(bogp_handle* h);   // bogp_comm.hip: destroys an owned communicator
std::vector<bogp_handle*> nll_team(bogp_handle* h, int P);  // bogp_batch.hip: the handles a batch of one-evaluation calls is dealt over
// bogp_point.hip: posterior, input-gradients and q criteria of B points through k_point_rhs + k_point_tri.  `Xb` is a HOST
// array (B x d).  Outputs (host, any may be null): mu, mse (B), dmu, dmse (B x d), acq (B x q), dacq (B x q x d).
int point_eval_host(bogp_handle* h, const char* who, const double* Xb, int B, int q, const int* acq_id, const double* acq_par,
                    double plugin, int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq, double* dacq);
// bogp_api_sweep.hip: the posterior sweep over the current candidates (single-target criteria, or -- eh non-null -- the
// m-target EHVI of bogp_api_ehvi.hip, or -- cn non-null -- the feasibility-weighted criteria of bogp_api_constrained.hip, or -- ec
// non-null -- the feasibility-weighted EHVI of bogp_api_ehvi_constrained.hip, all on the chunked path), and the reset of the winners a
// sweep left on the device
struct SweepRequest {
  bool want_out = false, want_acq_out = false;  // mu / MSE of every candidate into dmu_out / dmse_out (EHVI: M x m moments); the q x M values into dacq_out
  bool need_var = true, sync = true;            // false: the contraction is skipped (predict without eval_MSE); false: queued, not waited for
  int q = 0, minimize = 1;
  const int* acq_id = nullptr;
  const double* acq_par = nullptr;  // (may stay null: EI takes no parameter)
  double plugin = 0.0;
  const EhviArgs* eh = nullptr;
  const ConstrainedArgs* cn = nullptr;  // (q, acq_id, acq_par, plugin, minimize above are the criteria it weights)
  const ConstrainedEhviArgs* ec = nullptr;  // bogp_sweep_ehvi_constrained: EHVI of the objectives times the constraints' feasibility
  int targets() const { return eh ? eh->m : cn ? cn->m : ec ? ec->m : 1; }  // moments per candidate in dmu_out / dmse_out
};
int run_sweep(bogp_handle* h, const SweepRequest& rq);
void invalidate_sweep_results(bogp_handle* h);
// bogp_api_sweep.hip, shared with the believer and the Thompson passes: the chunk geometry of a pass over columns of `rows` doubles (the ONE
// reader of BOGP_CHUNK_MB; fails where sweep_chunk_rows does), the producer's arguments for the chunk at m0 on chunk buffer b, the argmax /
// value arrays of a pass (nblk block records per criterion, n_out moments or 0), and the validation of q criteria
struct SweepGeometry { int64_t Mc, nchunk; int S; };  // candidates per chunk (a multiple of 64), chunks, slices of the training set
int sweep_geometry(bogp_handle* h, int rows, SweepGeometry* g);
CorrArgs corr_chunk_args(const bogp_handle* h, const SweepGeometry& g, int64_t m0, int b);
int ensure_sweep_outputs(bogp_handle* h, int q, int64_t nblk, size_t n_out, bool want_acq_out);
int check_criteria(bogp_handle* h, int q, const int* acq_id, const double* acq_par);
#pragma GCC visibility push(hidden)  // (the library's dynamic symbols stay the ones they were)
// bogp_api_sweep.hip, the ranked tail of every entry that returns k winners per criterion.  None of the three touches last_q /
// last_topk_q / last_topk_k: the caller records what bogp_exchange_argmax / bogp_exchange_topk may pack.
//   rank_stored_values: ranks 0 .. k-1 of the q criteria over vals[q][M] into dtopk_* (queued; the block records are sized here)
//   pad_short_ranks:    ranks beyond the number of candidates, which the device leaves as (-inf, INT64_MAX), become (-inf, -1)
//   fetch_winners:      k == 1: dbest_*, which the sweep left, else rank_stored_values over vals[q][h->M] and dtopk_*, copied to
//                       best_val / best_idx [q][k]; waits for st -- everything queued on it before is complete -- and pads
int rank_stored_values(bogp_handle* h, const double* vals, int64_t M, int q, int k, hipStream_t st);
void pad_short_ranks(double* best_val, int64_t* best_idx, int n);
int fetch_winners(bogp_handle* h, int q, int k, const double* vals, double* best_val, int64_t* best_idx, hipStream_t st);
// bogp_api_sweep.hip: the model's half of a multi-target tail kernel's arguments -- gamma, ld_gamma, N, m and sigma2[] of the commit
void multi_target_model(const bogp_handle* h, MultiTargetChunk& a);
// bogp_point.hip, what every entry that takes EHVI cells does alike.  check_ehvi_cells: the nb = C m bounds -- a finite lower, a
// non-NaN upper, upper >= lower (BOGP_ERR_INVALID; the cell count and the pointers are checked by each entry where its own order of
// refusals has them).  stage_ehvi_cells: the bounds into dehvi_cells ([lower nb | upper nb]) in stream order and waited for, so that
// the caller's arrays are not needed afterwards; whatever bogp_point_eval_ehvi left there is forgotten; nb == 0 copies nothing.
int check_ehvi_cells(bogp_handle* h, const char* who, size_t nb, const double* lower, const double* upper);
int stage_ehvi_cells(bogp_handle* h, const double* lower, const double* upper, size_t nb, hipStream_t st);
// bogp_api_constrained.hip: the n_con intervals of modelled constraints -- no NaN, hi >= lo (BOGP_ERR_INVALID)
int check_constraint_bounds(bogp_handle* h, const char* who, int n_con, const double* lo, const double* hi);
#pragma GCC visibility pop
// bogp_api_constrained.hip, shared with the point path: what every entry with modelled constraints refuses alike, from the target count
// through the criteria down to the bounds (all BOGP_ERR_INVALID; hidden: the library's dynamic symbols stay the ones they were)
__attribute__((visibility("hidden"))) int check_constrained_request(bogp_handle* h, const char* who, int q, const int* acq_id, const double* acq_par, int n_con, const double* lo,
                              const double* hi);
int bound32_prepare(bogp_handle* h);  // bogp_api_sweep.hip: the FP32 copies of the committed model's active target, where the stage serves it
// bogp_api_sweep.hip, for bogp_api_lift.hip: a pending lazy upload finished (every candidate row on the device); the
// sweep timing zeroed (a lifted sweep without a feasible row runs no posterior pass)
int candidates_ready(bogp_handle* h);
void clear_sweep_timing(bogp_handle* h);
// kinds of the spans on the handle's `timer` (what bogp_last_timing makes of them per path: the table above collect_timing, bogp_api_sweep.hip)
enum { T_PRODUCER, T_CONTRACT, T_CRITERIA, T_WHOLE };
// the candidate calls need the row width d: from bogp_set_train or from bogp_forest_set
bool has_dim(const bogp_handle* h);
// dehvi_cells was overwritten by a sweep: bogp_point_eval_ehvi must upload its cells again
void ehvi_cells_forget(bogp_handle* h);
}

// ------------------------------------------------------------------------------------------------------
// Ownership.  Every device allocation, mapped pinned block and event of a handle is a member of one of the three types below and is
// released by that member's destructor (bogp_destroy only synchronises, then deletes the handle).  A raw pointer in bogp_handle is a
// VIEW into one of them and is never freed.  Non-copyable; bogp_debug_live reads the process-wide counts.
// ------------------------------------------------------------------------------------------------------
namespace bogp {
struct LiveCounts { std::atomic<int64_t> allocations{0}, bytes{0}, events{0}; };
inline LiveCounts g_live;
inline void live_note(int64_t n, size_t bytes) { g_live.allocations += n; g_live.bytes += n * (int64_t)bytes; }

// one hipMalloc allocation of `cap` elements
template <typename T>
struct DevBuf {
  T* ptr = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { free(); }
  operator T*() const { return ptr; }
  // at least n elements: nothing if they are there; otherwise the old block is freed FIRST and exactly n are allocated (no copy, no
  // growth factor, never shrinks).  On failure the buffer is empty and the handle's error is set.
  int ensure(bogp_handle* h, size_t n);
  void free() {
    if (ptr) { (void)hipFree(ptr); live_note(-1, cap * sizeof(T)); }
    ptr = nullptr;
    cap = 0;
  }
};

// one hipHostMallocMapped block of `cap` doubles and its device address (hfit, hpin, hbatch)
struct MappedBuf {
  double *ptr = nullptr, *dev = nullptr;
  size_t cap = 0;
  MappedBuf() = default;
  MappedBuf(const MappedBuf&) = delete;
  MappedBuf& operator=(const MappedBuf&) = delete;
  ~MappedBuf() { free(); }
  operator double*() const { return ptr; }
  int ensure(bogp_handle* h, size_t n);  // as DevBuf::ensure; the handle's stream is synchronised before a block is replaced, a new block is zero-filled
  void free() {
    if (ptr) { (void)hipHostFree(ptr); live_note(-1, cap * sizeof(double)); }
    ptr = dev = nullptr;
    cap = 0;
  }
};

// events created on demand and kept for the handle's life
struct EventPool {
  std::vector<hipEvent_t> ev;
  unsigned flags;
  explicit EventPool(unsigned f = hipEventDefault) : flags(f) {}
  EventPool(const EventPool&) = delete;
  EventPool& operator=(const EventPool&) = delete;
  ~EventPool() {
    for (auto e : ev) (void)hipEventDestroy(e);
    g_live.events -= (int64_t)ev.size();
  }
  hipEvent_t at(size_t i) {  // event i, created with those before it where it does not exist yet; null on failure
    while (ev.size() <= i) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
      ev.push_back(e);
      ++g_live.events;
    }
    return ev[i];
  }
  hipEvent_t& operator[](size_t i) { return ev[i]; }  // an event that at() has created
};

// The event timing of one call: marks (events of the pool, recorded in the order they are taken) and spans (two marks that bracket work
// of one kind; adjacent spans may share a mark).  What a kind means is its user's business.
struct SpanTimer {
  struct Span { int kind, a, b; };
  EventPool pool;
  size_t next = 0;
  std::vector<Span> spans;
  void begin() { next = 0; spans.clear(); }             // a new call: the events are handed out from the first again
  int mark(bogp_handle* h, hipStream_t st, int* idx);  // the next event, created on demand and recorded on st; *idx = its index
  hipEvent_t event(int idx) { return pool[(size_t)idx]; }
  void span(int kind, int a, int b) { spans.push_back({kind, a, b}); }
  double sum(int kind) {  // ms over the spans of `kind`, each waited for
    double ms = 0;
    for (const Span& s : spans) {
      float t = 0;
      if (s.kind != kind) continue;
      (void)hipEventSynchronize(pool[(size_t)s.b]);
      (void)hipEventElapsedTime(&t, pool[(size_t)s.a], pool[(size_t)s.b]);
      ms += t;
    }
    return ms;
  }
};
template <class Launch>  // a launch between two marks of its own on tm: one span of `kind` (defined behind HIPCHK, below)
int timed_span(bogp_handle* h, SpanTimer& tm, hipStream_t st, int kind, Launch launch);
// what a Thompson entry leaves for its *_last reader (ms): producer, draw at X + solves, the family's kernel; candidate chunks
struct ThompsonLast { double corr_ms = 0, solve_ms = 0, paths_ms = 0; int chunks = 0; };
}  // namespace bogp

struct bogp_handle {
  // The views (raw pointers into a member below, never freed): dy, dyt, drho, dgamma (the active target's part of d*_base), dsqrt_theta
  // (dtheta), dinfo (dscal), dXs (dXs_owned), bws_rows (dbws), hfit_dev (hfit), gsplit's two pointers (dgsplit_*).  hXs_lazy is the caller's.
  int device = 0;
  int n_cu = 256;  // compute units of the device (launch planning of the fused small-N sweep)
  hipStream_t stream = nullptr;
  bogp::DevBuf<unsigned int> dchain_flags;  // 2 * (cap_ld / 64) words: hand-over flags of the resident diagonal chain (k_chol_chain)
  bogp::EventPool ev_chol{hipEventDisableTiming};  // [2] look-ahead of the large-matrix Cholesky (second stream)
  hipStream_t stream2 = nullptr;  // producer stream: k_corr_chunk of chunk c+1 runs beside k_contract of chunk c
  std::string err;

  // training set.  The buffers are sized for cap_ld rows / cap_d columns / cap_nt targets and re-used by every
  // bogp_set_train that fits (a BO loop grows N by one point per tell(): no free / malloc of the N x N buffers per iteration)
  int cap_ld = 0, cap_d = 0, cap_nt = 0;
  int N = 0, d = 0, Np = 0;
  int ldr = 0;  // leading dimension of dR / dV / dRinv: N rounded up to 64 (identity padding, kernels_chol.hip)
  bogp::DevBuf<double> dX;
  // multi-target y (gpr.py:463,490,502-505): the factorisation is shared, the vectors exist once per target.  The views dy / dyt /
  // drho / dgamma and `sigma2` below always point at the ACTIVE target (bogp_select_target) inside these slabs.
  int n_t = 1, target = 0;
  bogp::DevBuf<double> dy_base, dyt_base, drho_base, dgamma_base;  // N, N, N, Np (zero padded) per target
  double *dy = nullptr, *dyt = nullptr, *drho = nullptr, *dgamma = nullptr;  // views
  std::vector<double> sigma2_t, nv_t;  // committed, per target

  // factorisation workspace (column-major, ld = ldr)
  bogp::DevBuf<double> dR, dV, dU, dT, dRinv;  // L, L^-1, L^-T, scratch, R^-1
  bogp::DevBuf<double> dones;  // N ones (the constant trend basis)
  bogp::DevBuf<double> dgemv_scratch;  // segment partials of launch_gemv2
  std::vector<double> h_theta;  // [theta (d + 1) | sqrt_theta (d + 1)]: the block uploaded by factorize
  bogp::DevBuf<double> ddinv;  // ldr x 64: inverses of the diagonal blocks of the running factorisation (kernels_chol.hip)
  bogp::DevBuf<double> dft, dtmp;  // N each
  bogp::DevBuf<double> dw;         // Np (zero padded)
  bogp::DevBuf<double> dtheta;     // [theta (d + 1) | sqrt_theta (d + 1)]
  double* dsqrt_theta = nullptr;   // view: the second half of dtheta
  bogp::DevBuf<double> dscal;      // small scalar scratch
  int* dinfo = nullptr;            // view: doubles 62-63 of dscal
  bogp::DevBuf<double> dgrad_partial;
  bogp::DevBuf<double> dbatch;

  // how the last factorisation formed R from the correlations (k_build_R's arguments): what bogp_commit's refinement of
  // gamma recomputes R with
  bool R_div = false;
  double R_a = 1.0, R_b = 1.0, R_diag = 1.0;

  // committed state
  bool committed = false;
  int kernel = 0, mode = 0, estimate_trend = 0;
  double beta = 0, G = 0, sigma2 = 0, noise_var = 0, llf = 0, ftft = 0;
  bogp::DevBuf<double> dXthT;  // [d][Np]
  bogp::DevBuf<double> dXnorm;  // [Np] squared norms of the columns of XthT (k_corr_mfma)
  // trend-rows path (p > 32 columns under universal kriging, kernels_fit.hip: k_pack_Vx): the packed extended factor, its row offsets
  bogp::DevBuf<double2> dVpx;
  bogp::DevBuf<double> dAtx;  // W G^-1 (N x p)
  int vx_Ne = 0, vx_Nt = 0;  // 0: the committed model does not use the path
  bogp::DevBuf<double2> dVp;  // [Np/16][Np/8][64]

  // candidates
  const double* dXs = nullptr;  // view: dXs_owned once candidates are set
  bogp::DevBuf<double> dXs_owned;
  bogp::DevBuf<double> dbounds;
  bogp::DevBuf<double> dxform;  // per dimension [scale id, precision, lo, hi] of bogp_candidates_set_transform, or null
  std::vector<double> h_xform;
  bogp::DevBuf<double> dsobol;  // d x bits direction numbers (uint64 bit patterns)
  int64_t M = 0;
  // bogp_candidates_upload_lazy: host rows that are copied chunk by chunk on `stream_copy` WHILE the sweep contracts the chunk before
  // (run_sweep); lazy_done = rows whose copy has been enqueued, ev_copy = recorded behind the last enqueued copy
  const double* hXs_lazy = nullptr;
  int64_t lazy_done = 0;
  hipStream_t stream_copy = nullptr;
  bogp::EventPool ev_copy{hipEventDisableTiming};  // [1]

  // sweep scratch
  bogp::DevBuf<double> drT[2], dmu_part[2], dw_part[2];
  bogp::DevBuf<double> dss_part;
  bogp::ContractTile contract_tile;  // candidate tile of the direct contraction: bogp_set_contract_tile / bogp_last_contract_tile
  bogp::DevBuf<double> dblk_val, dmu_out, dmse_out, dacq_out, dbest_val;
  bogp::DevBuf<int64_t> dblk_idx, dbest_idx;
  bogp::DevBuf<unsigned int> dcounter;  // arrival ticket of k_sweep_small's last workgroup (zero between launches)
  // pruned sweep (kernels_prune.hip; bogp_set_prune): control words | block offsets | index map | selected rows | block counts | flags
  int prune_mode = 1;            // bogp_set_prune: 0 off, 1 automatic (one pass where it applies), 2 the per-chunk path
  int prune_path = 0;            // BOGP_PRUNE_PATH_* of the last sweep; survivors behind the pilot and rounds of its one-pass segments
  int64_t prune_survivors = 0;
  int prune_rounds = 0;
  bogp::DevBuf<long long> dprune;
  // FP32 bounding stage of the one-pass flow (kernels_bound32.hip; bogp_set_prune_bound32): FP32 copies of the committed
  // model -- [4 ceil(d / 4)][Np] scaled points | norms, gamma, w (Np each) | three statistics -- valid while b32_gen == commit_gen and
  // b32_target == target (rebuilt by bound32_prepare at commit and, for another target, by the sweep that needs them)
  int prune_bound32 = 1;
  bogp::DevBuf<float> dX32, dvec32;
  bogp::DevBuf<double> dstats32;
  double stats32[3] = {0, 0, 0};
  uint64_t commit_gen = 0, b32_gen = 0;
  int b32_target = -1;
  int64_t b32_rows = 0, b32_kept = 0;  // bogp_last_bound32: rows bounded in FP32, |S1| over the segments, segments that fell back
  int b32_fallbacks = 0;
  size_t b32_ws_row32 = 0, b32_ws_flag1 = 0, b32_ws_rmax = 0;  // where the last sweep's work space holds the segment's sums / flags (words of dprune)
  int64_t b32_last_rows = 0;           // rows of the last segment bounded in FP32: what bogp_debug_bound32 reads back
  bool prune_used = false;       // the last sweep pruned: its contracted-row count is on the device (dprune[4])
  int64_t contracted_rows = 0;   // ... otherwise it is this
  bogp::DevBuf<double> dtopk_val;  // [q][k] winners of bogp_sweep_topk (device-resident between its passes)
  bogp::DevBuf<int64_t> dtopk_idx;
  bogp::DevBuf<double> dehvi_cells;  // bogp_sweep_ehvi: [lower C x m | upper C x m]
  bogp::DevBuf<double> dpof_out;     // bogp_sweep_constrained: [M] probability of feasibility (pof_out requested)
  // host copy of the cells bogp_point_eval_ehvi / bogp_polish_ehvi left in dehvi_cells ([lower | upper], ehvi_host_C x ehvi_host_m): a call
  // with the same cells skips the upload.  Empty <=> unknown: every other writer of dehvi_cells clears it (ehvi_cells_forget)
  std::vector<double> h_ehvi_cells;
  int ehvi_host_m = 0, ehvi_host_C = 0;

  // lift of a reduced search space (bogp_api_lift.hip): lift_D > 0 <=> a lift is set, for a model of d = lift_r
  int lift_D = 0, lift_r = 0;
  bogp::DevBuf<double> dlift;       // [A (r x D) | mean | center | lo | hi]
  bogp::DevBuf<double> dlift_pen;   // [M] penalties of the last lifted sweep
  bogp::DevBuf<int> dlift_cnt;      // [ceil(M / 256)] feasible rows per workgroup
  bogp::DevBuf<int64_t> dlift_off;  // their exclusive scan, + M_f
  bogp::DevBuf<double> dlift_Z;     // [M_f][r] the feasible rows in their original order
  bogp::DevBuf<int64_t> dlift_map;  // [M_f] their original indices
  bogp::DevBuf<double> dlift_val;   // [q][M] merged values
  bogp::SpanTimer lift_timer;       // filter, merge (run_sweep, on the sweep's own timer, runs between them)
  int64_t lift_n_feasible = 0;
  double lift_filter_ms = 0, lift_merge_ms = 0;

  // Kriging-believer batches (bogp_api_believer.hip): shared by its four families and laid out anew by every call -- the table above
  // believer_run there states the four layouts
  bogp::DevBuf<double> dbel_s;      // the running variances sigma2_k s_B(x)
  bogp::DevBuf<double> dbel_C;      // [slots][M] c_k(x) of the believed points whose pivot passed the guard
  bogp::DevBuf<double> dbel_row;    // criterion values (PoF, k_believer's scratch) / MSE of the step evaluated last
  bogp::DevBuf<double> dbel_small;  // point, r(p), V r(p), R^-1 r(p), the believed rows and their mutual correlations
  bogp::SpanTimer bel_timer;        // solves, chunk producers, k_believer, the multi-target criterion kernel (run_sweep restarts the sweep's own)
  double bel_corr_ms = 0, bel_solve_ms = 0, bel_pass_ms = 0;  // of the last believer call of any family: producer, solves, k_believer
  int bel_passes = 0;                                          // candidate passes it ran after pass 0
  double bel_criterion_ms = 0;  // the criterion kernel of the last multi-target believer call (k_believer_ehvi / _constrained / _ehvi_constrained)

  // Thompson-sampling batches (bogp_api_thompson.hip)
  bogp::DevBuf<double> dth_small;  // omega | phase | W | coefficient block (-g, or gamma - g) | s, V s, R^-1 s of the call in flight
  bogp::SpanTimer th_timer;        // draw at X + solves, chunk producers, k_thompson / k_thompson_constrained
  bogp::ThompsonLast th_last, thc_last;  // of the last bogp_sweep_thompson / bogp_sweep_thompson_constrained, both on th_timer's spans

  // packed regression forest (bogp_api_forest.hip): the second model kind of a handle.  forest_T > 0 <=> a forest is set; it then
  // owns `d` (a handle carries a GP training set or a forest, never both)
  int forest_T = 0, forest_tree_words = 0, forest_depth = 0;
  int forest_m = 1;  // outputs a leaf holds: 1 (bogp_forest_set) or 2 .. BOGP_MAX_TARGETS (bogp_forest_set_multi)
  int64_t forest_nodes = 0, forest_leaves = 0;
  bogp::DevBuf<unsigned long long> dforest_words;
  bogp::DevBuf<bogp::ForestTree> dforest_tree;

  // polynomial trend bases with p > 1 columns (linear / quadratic; the constant basis keeps its scalar fast path)
  int trend = BOGP_TREND_CONSTANT, p = 1;  // committed
  double reml_logdet_ftf = 0.0;  // log det(F^T F) of the basis `reml_ftf_basis` (REML value, p > 1); -1: none cached
  int reml_ftf_basis = -1;
  int tr_built = -1, tr_p = 0, ldp = 0;    // basis currently held in dF / sizes of the buffers below
  std::vector<double> h_beta_fixed;        // bogp_set_trend_beta: simple-kriging coefficients
  // bogp_nll_batch above N = 2048 (r05): a second handle -- own stream, own factor buffers -- evaluates every other slot on a second host
  // thread, so that one evaluation's chain of small launches runs beside the other's rank-128 updates.  The host copy of the training set
  // (as bogp_set_train received it) is what the second handle is fed from; `train_gen` tells it when to take it again.
  std::vector<double> h_X, h_y;
  unsigned long train_gen = 0;
  std::vector<bogp_handle*> aux;       // helper handles (up to 2)
  std::vector<unsigned long> aux_gen;  // the train_gen each was last fed at
  bool aux_fail_valid = false;         // a helper could not be loaded (device memory) at train_gen == aux_fail_gen: not retried until the training set changes
  unsigned long aux_fail_gen = 0;
  std::vector<double> h_betav, h_Sinv;     // committed beta (p) and (Ft^T Ft)^-1 (p x p, column-major) for bogp_gradient
  bogp::DevBuf<double> dF, dFt, dQ1, dQ;  // N x p, column-major, ld = N
  bogp::DevBuf<double> dWp;               // Np x p: L^-T Ft, zero-padded rows
  // split-K scratch of the small products (kernels_gemm.hip), allocated with the trend buffers; gsplit = what launch_gemm takes: views of the two
  bogp::DevBuf<double> dgsplit_scratch;
  bogp::DevBuf<unsigned int> dgsplit_tickets;
  bogp::GemmSplit gsplit = {nullptr, 0, nullptr, 0};
  bogp::DevBuf<double> dWpT;    // pp x Np (pp = p rounded up to 128): W^T, zero rows in the padding -- column side of the k_mm128 trend product
  bogp::DevBuf<double> dSinvP;  // pp x pp: (Ft^T Ft)^-1, zero padded
  bogp::DevBuf<double> dA[2], dAV[2], dAU[2];  // ldp x ldp (CholeskyQR2)
  bogp::DevBuf<double> dAw, dAT;               // ldp x 64, ldp x ldp scratch
  bogp::DevBuf<double> dGinv, dSinv, dbetav, dqty;  // p x p, p x p, p, p
  bogp::DevBuf<int> dinfo2;
  bogp::DevBuf<double> dTt, dCS, duu, dmtrend;  // per sweep chunk: Mc x p, Mc x p, Mc, Mc
  bogp::DevBuf<double> dtpart[2];  // [S][pv][Mc] slice sums of W^T r from the fused producer (p <= 32)

  // cross-rank exchange (bogp_comm.hip): RCCL communicator (owned or borrowed), send / receive records on the device, and
  // what the last sweep left in dbest_* / dtopk_* for bogp_exchange_* to pack
  void* comm = nullptr;
  bool comm_owned = false;
  int comm_rank = 0, comm_world = 0;
  bogp::DevBuf<double> dxchg_send, dxchg_recv;
  int last_q = 0, last_topk_q = 0, last_topk_k = 0;

  // one-point / B-point evaluation and the lock-step polish (kernels_point.hip, bogp_point.hip)
  bogp::DevBuf<double> dpt_rhs, dpt_part, dpt_out, dpt_Xb, dpt_state, dpt_box;
  bogp::DevBuf<unsigned int> dpt_counter;  // [cap] arrival tickets (zero between launches) + 1 word: finished starts of the polish
  bogp::DevBuf<double> dpt_split;  // partial tiles of split row blocks (one-point latency mode of k_point_tri)
  bogp::DevBuf<double> dpt_tw, dpt_trec;  // linear trend in the one-point path: W^T [r | dr/dx] per point, the trend records
  bogp::DevBuf<unsigned int> dpt_splitc;
  // the likelihood's host traffic (r03): theta travels through a pinned staging block, the scalars / gradient sums come back through
  // a device-mapped pinned block that one gather kernel fills, completion read off a sequence word (bogp_api.hip: fit_readback)
  double* hfit_dev = nullptr;  // view: hfit's device address
  bogp::MappedBuf hfit;  // pinned: [0, 2048) theta staging | [2048, 2112) the 64 scalars | [2112, 2112 + 512) gradient sums | [3000] sequence word
  unsigned long long fit_seq = 0;
  bogp::DevBuf<unsigned int> dfin_ticket;  // k_grad_finish: which workgroup finished last
  bogp::MappedBuf hpin;  // pinned host buffer the finishing workgroup writes its records into (device-mapped)
  unsigned long long pt_seq = 0;  // sequence number of the last one-point call (completion word behind its record)
  // bogp_nll_batch (bogp_batch.hip): pinned device-mapped staging (parameter rows in, records out; the sequence word sits in the
  // block's last 8 doubles), the slot-completion ticket, and the P workspaces of the elimination path with their BatchSlot table
  bogp::MappedBuf hbatch;
  bogp::DevBuf<unsigned int> dbatch_ticket;
  unsigned long long batch_seq = 0;
  bogp::DevBuf<double> dbws;
  bogp::DevBuf<bogp::BatchSlot> dbslots;
  int bws_P = 0, bws_ld = 0, bws_d = 0, bws_N = 0;
  double* bws_rows = nullptr;  // view into dbws: [bws_P][bws_row] parameter rows on the device
  size_t bws_row = 0;

  // timing of the last sweep/predict
  bogp::SpanTimer timer;  // spans of the last sweep / predict / forest call (kinds and their meaning per path: collect_timing, bogp_api_sweep.hip)
  double t_corr_ms = 0, t_contract_ms = 0, t_acq_ms = 0;
  int n_chunks = 0;
  bool timing_pending = false;  // the spans have not been read into the three times yet
};

#define FAIL(h, code, ...)                              \
  do {                                                  \
    char _b[512];                                       \
    snprintf(_b, sizeof(_b), __VA_ARGS__);              \
    (h)->err = _b;                                      \
    return (code);                                      \
  } while (0)
#define HIPCHK(h, expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess) FAIL(h, BOGP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
template <typename T>
inline int bogp::DevBuf<T>::ensure(bogp_handle* h, size_t n) {
  if (cap >= n && ptr) return BOGP_OK;
  T** p = &ptr;  // (HIPCHK's message quotes its expression: the two below read as they did in the free-standing ensure(h, &ptr, &cap, n))
  if (*p) {
    HIPCHK(h, hipFree(*p));
    live_note(-1, cap * sizeof(T));
  }
  *p = nullptr;
  cap = 0;
  HIPCHK(h, hipMalloc((void**)p, n * sizeof(T)));
  cap = n;
  live_note(1, n * sizeof(T));
  return BOGP_OK;
}
inline int bogp::MappedBuf::ensure(bogp_handle* h, size_t n) {
  if (cap >= n && dev) return BOGP_OK;
  if (ptr) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipHostFree(ptr));
    live_note(-1, cap * sizeof(double));
    ptr = dev = nullptr;
    cap = 0;
  }
  HIPCHK(h, hipHostMalloc((void**)&ptr, n * sizeof(double), hipHostMallocMapped));
  cap = n;
  live_note(1, n * sizeof(double));
  HIPCHK(h, hipHostGetDevicePointer((void**)&dev, ptr, 0));
  memset(ptr, 0, n * sizeof(double));
  return BOGP_OK;
}
inline int bogp::SpanTimer::mark(bogp_handle* h, hipStream_t st, int* idx) {
  hipEvent_t e = pool.at(next);
  if (!e) FAIL(h, BOGP_ERR_HIP, "hipEventCreate failed");
  HIPCHK(h, hipEventRecord(e, st));
  *idx = (int)next++;
  return BOGP_OK;
}
template <class Launch>
inline int bogp::timed_span(bogp_handle* h, SpanTimer& tm, hipStream_t st, int kind, Launch launch) {
  int a = 0, b = 0, e;
  if ((e = tm.mark(h, st, &a))) return e;
  HIPCHK(h, launch());
  if ((e = tm.mark(h, st, &b))) return e;
  tm.span(kind, a, b);
  return BOGP_OK;
}
// (for the two local temporaries of bogp_selftest_profile, kernels_profile.hip; the handle's buffers free themselves)
template <typename T>
static inline void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}
