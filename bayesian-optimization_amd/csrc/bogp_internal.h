// bogp_internal.h -- host-side declarations shared by the translation units of libbogp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/bogp.h"

namespace bogp {

// ---- kernel argument blocks (passed by value) -------------------------------------------------------
struct CorrArgs {
  const double* Xs;          // candidates, M x d row-major (device)
  int64_t M;                 // total candidates
  int64_t m0;                // first candidate of this chunk
  int64_t Mc;                // chunk size padded to a multiple of 64
  int d;
  int Np;                    // training points padded to a multiple of 32
  int nblk_per_split;        // 32-blocks of n per workgroup (grid.y slices the training set)
  const double* sqrt_theta;  // d
  const double* XthT;        // [d][Np] theta-scaled training points, transposed
  const double* xnorm = nullptr;  // [Np] squared norms of the columns of XthT (k_corr_mfma); null: kernel A
  const double* gamma;       // Np (zero padded)
  const double* wvec;        // Np (zero padded): L^-T Ft, or zeros for simple kriging
  double* rT;                // [Np][Mc] correlation chunk, n-major
  bool store = true;         // false: r is not written and rT is not touched (may be null) -- only where corr_chunk_without_store()
  double* mu_part;           // [S][Mc]
  double* w_part;            // [S][Mc]
  // polynomial trend with few columns, fused into the producer (k_corr_chunk<K, PV>): pv = 0 (off) / 16 / 24 / 32 >= p
  int pv = 0;
  const double* Wrow = nullptr;  // [Np][wld] row-major W = L^-T Ft, zero padded columns
  int wld = 0;
  double* t_part = nullptr;      // [S][pv][Mc] slice sums of W^T r
};
// Leading dimension of the factor buffers for N training points: N rounded up to 64; to 128 above the elimination's limit (N > 3072), where the
// inverse, R^-1 and the Cholesky's wide panels work on 128 x 128 tiles (kernels_chol.hip, BIG_LD)
inline int train_ld(int N) { return N > 3072 ? ((N + 127) / 128) * 128 : ((N + 63) / 64) * 64; }
// Chunk geometry of every candidate pass (sweep, believer, Thompson).  The training set is sliced into groups of 8 x 32 rows per producer
// workgroup: S is a function of N only, so that the grouping of the partial sums of mu (hence every output bit) does not depend on the chunk size.
constexpr int SWEEP_NBLK_PER_SPLIT = 8;  // (4 / 16 measured: profiles/r05_corr_split_ab.txt)
inline int sweep_slices(int Np) { return (Np / 32 + SWEEP_NBLK_PER_SPLIT - 1) / SWEEP_NBLK_PER_SPLIT; }
// Candidates per chunk (exported as bogp_sweep_chunk_rows): what `chunk_bytes` hold of columns of `rows` doubles, in whole 64-row tiles,
// at least one tile and at most the M candidates padded to one.  The LDS-free kernels address the rows of a chunk through 32-bit lane
// byte offsets proportional to Mc, of which the largest is 8 (7 Mc + 30):
//   kernels_posterior.hip  k_contract16d      voffA1 = ((lane >> 4) * Mc + 2 * (lane & 15)) * 8 + 4 * Mc * 8
//   kernels_chol.hip       mm128_tile_direct  voffR1 = (lk * ldr + 2 * li) * 8 + 4 * ldr * 8, ldr = Mc in the trend product
//   corr_mfma_body.inc     k_corr_mfma        offR   = (lk * Mc + li) * 8, the smaller one
// with lane >> 4 = lk <= 3 and li <= 15.  8 (7 Mc + 30) < 2^32 holds up to Mc = 76 695 840, i.e. 76 695 808 in whole tiles; a larger
// chunk returns -1 and the callers fail.  The trend GEMM's own limit, Mc <= INT_MAX / 2, lies far above and is subsumed.
constexpr int64_t SWEEP_MAX_CHUNK_ROWS = ((((int64_t)1 << 29) - 31) / 7) / 64 * 64;
inline int64_t sweep_chunk_rows(int64_t rows, int64_t M, int64_t chunk_bytes) {
  const int64_t Mpad = (M + 63) / 64 * 64, fit = chunk_bytes / (rows * (int64_t)sizeof(double)) / 64 * 64;
  const int64_t Mc = fit < 64 ? 64 : fit < Mpad ? fit : Mpad;  // (Mpad >= 64)
  return Mc > SWEEP_MAX_CHUNK_ROWS ? -1 : Mc;
}
int corr_trend_columns(int p);  // the PV instantiation serving p trend columns, 0 if none does
bool corr_chunk_without_store(int kernel, int pv, bool have_xnorm);  // launch_corr_chunk has a producer without the store for this call

struct ContractArgs {
  const double* rT;   // [Np][Mc]
  const double2* Vp;  // packed L^-1: [NJ16][NKP][64] double2
  double* ss_part;    // [nJ][Mc]
  int64_t Mc;
  int nMt;   // Mc / 64
  int nJ;    // column groups
  int NJ16;  // Np / 16
  int NKP;   // Np / 8
  int64_t cross_B;  // launch_contract_cross: points (ss_part is then their record array, see k_contract16<NR, NCP>)
  const long long* live = nullptr;  // pruned sweep: device word holding the live row count (workgroups of tiles past it return at once), or null
};

// Candidates per workgroup of a direct contraction launch (exported as bogp_contract_tile_rows; DESIGN.md 5.2'''): 64 (k_contract16d) while the
// 64-row grid fills the chip, else 32, else 16 (k_contract16n).  tiles64 x nJ = the workgroups of the 64-row grid; the crossovers are workgroups of
// that grid per CU, in quarters so that the edges are exact in integers (measured: profiles/contract_rows.txt, section B).  The gated launches of the
// per-chunk pruned path (live) keep 64 rows.  The bits do not depend on the choice.
constexpr int CONTRACT_TILE64_MIN_WG_PER_4CU = 14;  // from 3.5 workgroups a CU: 64 rows              (profiles/contract_rows.txt, section B)
constexpr int CONTRACT_TILE32_MIN_WG_PER_4CU = 6;   // from 1.5 workgroups a CU: 32 rows, below: 16   (profiles/contract_rows.txt, section B)
inline int contract_tile_rows(int64_t tiles64, int nJ, int n_cu, bool live) {
  if (live) return 64;
  const int64_t wg4 = 4 * tiles64 * (int64_t)(nJ > 0 ? nJ : 1), cu = n_cu > 0 ? n_cu : 1;
  if (wg4 >= CONTRACT_TILE64_MIN_WG_PER_4CU * cu) return 64;
  if (wg4 >= CONTRACT_TILE32_MIN_WG_PER_4CU * cu) return 32;
  return 16;
}
struct ContractTile {
  int n_cu = 0;    // compute units of the handle's device
  int forced = 0;  // bogp_set_contract_tile: 0 automatic, 16 / 32 / 64
  int last = 64;   // bogp_last_contract_tile: tile rows of the last contraction launch
};

struct AcqArgs {
  const double* mu_part;  // [S][Mc]
  const double* w_part;   // [S][Mc]
  const double* ss_part;  // [nJ][Mc]
  int S, nJ;
  int nJ_plus = 0;        // trend-rows path (k_pack_Vx): column groups nJ .. nJ + nJ_plus - 1 of ss_part hold |u|^2 and are ADDED
  int64_t Mc;      // chunk stride of the partial arrays
  int64_t mcount;  // valid candidates in this chunk
  int64_t m0;      // global index of the chunk's first candidate
  double beta;     // trend coefficient (constant basis)
  const double* mtrend;  // [Mc] f(x*) . beta for polynomial bases (replaces beta), or null
  const double* uu;      // [Mc] u^T u for polynomial bases under universal kriging (replaces the w_part term), or null
  double G;        // QR factor of Ft (ordinary kriging), unused otherwise
  int estimate_trend;
  double sigma2;
  double* mu_out;   // [M] or null (global arrays, indexed by m0 + i)
  double* mse_out;  // [M] or null
  int q;
  int acq_id[64];
  double acq_par[64];
  double plugin;
  int minimize;
  double* acq_out;     // [q][M] or null
  int64_t M;           // row stride of acq_out
  double* blk_val;     // [q][nblk_total] per-block partial argmax
  int64_t* blk_idx;    // [q][nblk_total]
  int64_t blk_offset;  // first block slot of this chunk
  int64_t nblk_total;
  // pruned sweep (kernels_prune.hip): the valid row count on the device (replaces mcount; workgroups past it return at once), and the
  // global candidate index of every row of a gathered survivor buffer (replaces m0 + i); both null otherwise
  const long long* live;
  const int64_t* map;
};

// the pruned sweep (kernels_prune.hip): bound every row of a chunk region against the running best, compact the survivors in order,
// gather their columns into the survivor buffer, and merge the block records of an acquisition launch into the running best
constexpr int PRUNE_CTL_WORDS = 8;  // device control words: see kernels_prune.hip
constexpr int PRUNE_CTL_CONTRACTED = 4, PRUNE_CTL_TOTAL = 5;  // ... the two the host reads: rows contracted on the per-chunk path; survivors of the region bounded last
struct PruneBoundArgs {
  const double* mu_part;  // [S][Mc] (offset to the region's first row)
  const double* w_part;   // [S][Mc]
  int S;
  int64_t Mc;
  int64_t rcount;         // rows of the region
  double beta, G, sigma2, plugin;
  int estimate_trend, minimize, q;
  int acq_id[64];
  double acq_par[64];
  const double* best_val; // [q] running best per criterion (device): the thresholds
  unsigned char* flags;   // [rcount] 1 = survives
  int* blk_count;         // [ceil(rcount / 256)]
};
struct PruneGatherArgs {
  const long long* ctl;
  const unsigned char* flags;
  const int64_t* offsets;   // exclusive scan of blk_count
  int64_t rcount, m0;       // region rows; global index of the region's first row
  int64_t Mc, Ms;           // strides of the chunk arrays / of the survivor arrays
  int S, Np;
  const double *rT, *mu_part, *w_part;  // chunk arrays (offset to the region's first row)
  double *rTs, *mu_s, *w_s;             // survivor arrays
  int* sel;                 // [<= rcount / 4] region row of this region's k-th survivor
  int64_t* map;             // [Ms] global index of every buffered survivor
};
hipError_t launch_prune_init(long long* ctl, double* best_val, int64_t* best_idx, int q, int64_t pilot_rows, hipStream_t st);
hipError_t launch_prune_bound(const PruneBoundArgs& a, hipStream_t st);
hipError_t launch_prune_scan(const int* blk_count, int64_t nblk, int64_t* offsets, int64_t rcount, int64_t cap, long long* ctl, hipStream_t st);
hipError_t launch_prune_gather(const PruneGatherArgs& a, hipStream_t st);
// one pass: the global indices m0 + i of the flagged rows, in order, into sidx[0 .. cap); rows sidx[0 .. count) of Xs -> Xc (count x d)
hipError_t launch_prune_index(const unsigned char* flags, const int64_t* offsets, int64_t rcount, int64_t m0, int64_t cap, int64_t* sidx,
                              hipStream_t st, const int64_t* through = nullptr);  // through: sidx[k] = through[i] instead of m0 + i
hipError_t launch_prune_rows(const double* Xs, const int64_t* sidx, int64_t count, int d, double* Xc, hipStream_t st);

// The two host decisions of the one-pass pruned sweep (exported as bogp_prune_decide; the values are BOGP_PRUNE_PATH_* of include/bogp.h).
// A pilot of which more than an eighth survives its own thresholds sends the whole sweep to the per-chunk path (1); a segment of which
// more than a quarter survives falls back to it alone (3); otherwise the survivors are contracted in rounds (2).  Shares of exactly
// 1/8 and 1/4 stay on the one-pass side; products, not quotients, so that the edges are exact.
inline int prune_decide(int64_t pilot_rows, int64_t pilot_survivors, int64_t segment_rows, int64_t segment_survivors) {
  if (8 * pilot_survivors > pilot_rows) return 1;
  if (4 * segment_survivors > segment_rows) return 3;
  return 2;
}
// (value, index) records of the first ceil(rows / 256) blocks -> merged into best_val / best_idx; rows = *live if live, else count
hipError_t launch_prune_update(const double* blk_val, const int64_t* blk_idx, int64_t stride, const long long* live, int64_t count, int q,
                               double* best_val, int64_t* best_idx, hipStream_t st);
hipError_t launch_prune_flushed(long long* ctl, hipStream_t st);  // the buffer went through the contraction: count it, empty it

// The FP32 bounding stage of the one-pass pruned sweep (kernels_bound32.hip): the sums r . gamma and w . r of every
// row of a segment from FP32 correlations, the rows that cannot be ruled out within their margins flagged for the exact pass.
constexpr int BOUND32_MAX_D = 128;  // the FP32 candidate tile stays within the default 64 KB of dynamic LDS
inline bool bound32_supported(int kernel, int d) {
  return (kernel == BOGP_KERNEL_SE || kernel == BOGP_KERNEL_MATERN32 || kernel == BOGP_KERNEL_MATERN52) && d <= BOUND32_MAX_D;
}
struct Bound32Model {        // FP32 copies of the committed model (built at commit: bound32_prepare)
  const float* XthT;         // [4 ceil(d / 4)][Np] theta-scaled training points, transposed; zero rows from d on
  const float* xnorm;        // [Np] squared norms of the FP64 scaled points, rounded
  const float* gamma;        // [Np]
  const float* wvec;         // [Np]
  double gamma_l1, w_l1, nb_max;  // 1-norms of gamma and w, the largest squared norm
};
struct Bound32Args {
  const double* Xs;          // candidates, M x d row-major
  int64_t M, m0, rcount;     // total candidates; first row of the region; its rows
  int d, Np;
  int estimate_trend;        // as k_bound32_flags receives it: without a trend nothing reads w . r, and it is not summed (d <= 32)
  const double* sqrt_theta;
  Bound32Model md;
  double *mu, *wd, *na;      // [rcount] r . gamma, w . r, |a|^2 of the row's FP64 scaled point
};
hipError_t launch_bound32_prepare(int kernel, const double* XthT, const double* xnorm, const double* gamma, const double* wvec, int d, int Np,
                                  float* XthT32, float* vec32, double* stats, hipStream_t st);
hipError_t launch_bound32_sums(int kernel, const Bound32Args& a, hipStream_t st);
// PruneBoundArgs' region with mu_part = the FP32 sums (S = 1): flags and block counts as launch_prune_bound leaves them
hipError_t launch_bound32_flags(const PruneBoundArgs& pb, int kernel, int d, const double* wd, const double* na, const Bound32Model& md,
                                hipStream_t st);

// What the chunk loop and the committed model fill for a kernel that evaluates an m-target posterior over one chunk: the first part
// of EhviArgs and ConstrainedArgs, read by multi_target_moments (bogp_device.h).  Both blocks lie in memory as they did before they
// shared it (mu_out / mse_out stay where each had them): moving those two into this part cost k_ehvi<2> 2 % and gained k_ehvi<3> 2 %.
// (ConstrainedEhviArgs holds the same fields in another order, and neither order serves both: under ConstrainedEhviArgs' order
// k_constrained<5> no longer keeps its five groups of 16 gamma scalars in flight -- the fifth load waits behind the fmas of the other
// four, 2.97 -> 4.75 ms at N = 2048 over 1e6 rows --, under this one k_ehvi_constrained gets the stack frame its comment names:
// profiles/multi_target_fold.txt.  Check -Rpass-analysis=kernel-resource-usage and the loop's s_load_dwordx16 after moving a field.)
struct MultiTargetChunk {
  const double* rT;       // [Np][Mc] the chunk's correlation columns (read for the m means)
  const double* gamma;    // [m][ld_gamma] the targets' gamma columns
  int ld_gamma, N;        // Np; training points summed over
  const double* ss_part;  // [nJ][Mc]
  const double* w_part;   // [S][Mc] (constant trend with estimate_trend only)
  int S, nJ;
  int64_t Mc, mcount, m0;
  double beta, G;
  int estimate_trend;
  int m;                  // targets, 2 .. BOGP_MAX_TARGETS
  double sigma2[8];       // per target
};

// expected hypervolume improvement of an m-target model over one chunk (kernels_ehvi.hip): replaces AcqArgs / k_acquisition
// in the chunk loop of bogp_sweep_ehvi
struct EhviArgs : MultiTargetChunk {
  const double* lower;    // [C][m] cell bounds (device)
  const double* upper;    // [C][m] (+inf allowed)
  int C;
  double* ehvi_out;       // [M] (global index m0 + i)
  double* mu_out;         // [M][m] or null
  double* mse_out;        // [M][m] or null
  double* blk_val;        // per-block partial argmax
  int64_t* blk_idx;
  int64_t blk_offset;
};
hipError_t launch_ehvi(const EhviArgs& a, hipStream_t st);

// q feasibility-weighted criteria of an m-target model over one chunk (kernels_constrained.hip): target 0 is the objective, targets
// 1 .. m - 1 are constraints feasible in [lo_k, hi_k]; replaces AcqArgs / k_acquisition in the chunk loop of bogp_sweep_constrained
struct ConstrainedArgs : MultiTargetChunk {
  double lo[8], hi[8];    // per target; entry 0 is not read
  int q;
  int acq_id[64];         // BOGP_ACQ_EI / EPSILON_PI / MGFI, or BOGP_ACQ_NONE: the probability of feasibility alone
  double acq_par[64];
  double plugin;
  int minimize;
  double* acq_out;        // [q][M] (global index m0 + i)
  int64_t M;              // row stride of acq_out
  double* pof_out;        // [M] or null
  double* mu_out;         // [M][m] or null
  double* mse_out;        // [M][m] or null
  double* blk_val;        // [q][nblk_total] per-block partial argmax
  int64_t* blk_idx;
  int64_t blk_offset, nblk_total;
};
hipError_t launch_constrained(const ConstrainedArgs& a, hipStream_t st);

// feasibility-weighted EHVI of an m-target model over one chunk (kernels_ehvi_constrained.hip): targets 0 .. m_obj - 1 are the objectives
// of EhviArgs' cells, targets m_obj .. m - 1 are constraints feasible in [lo_j, hi_j]; replaces AcqArgs / k_acquisition in the chunk
// loop of bogp_sweep_ehvi_constrained
struct ConstrainedEhviArgs {
  // (the fields stand in the order the kernel reads them -- what the loop over the training points reads first, then what the moments,
  // the feasibility, the cells and the argmax read after it -- so that no group of scalars loaded together is live on both sides of that
  // loop, which holds 16 m scalar registers of gamma: with EhviArgs' order the instances with m_obj >= 4 and one constraint kept a
  // 36-byte stack frame; check -Rpass-analysis=kernel-resource-usage after moving one)
  const double* rT;       // [Np][Mc] the chunk's correlation columns (read for the m means)
  const double* gamma;    // [m][ld_gamma] the targets' gamma columns
  int ld_gamma, N;        // Np; training points summed over
  int64_t Mc, mcount, m0;
  const double* ss_part;  // [nJ][Mc]
  const double* w_part;   // [S][Mc] (constant trend with estimate_trend only)
  int S, nJ;
  double beta, G;
  int estimate_trend;
  int m, m_obj;           // targets, 3 .. BOGP_MAX_TARGETS; objectives among them, 2 .. m - 1
  double sigma2[8];       // per target
  double* mu_out;         // [M][m] or null
  double* mse_out;        // [M][m] or null
  double lo[8], hi[8];    // per constraint: entry j belongs to target m_obj + j
  double* pof_out;        // [M] or null
  const double* lower;    // [C][m_obj] cell bounds (device); not read for C == 0
  const double* upper;    // [C][m_obj] (+inf allowed)
  int C;                  // 0: the probability of feasibility alone
  double* val_out;        // [M] (global index m0 + i)
  double* blk_val;        // per-block partial argmax
  int64_t* blk_idx;
  int64_t blk_offset;
};
hipError_t launch_ehvi_constrained(const ConstrainedEhviArgs& a, hipStream_t st);

// one Kriging-believer pass over a chunk (kernels_believer.hip): the rank-one downdate of the running variance by the believed point p,
// c(x) = (k(x, p) - r(x) . a + u(x) u(p) - sum_k c_k(x) c_k(p)) / sqrt(pivot), s(x) -= sigma2 c(x)^2, and -- for the pass in front of a
// step -- that step's criterion on (mu, max(0, s)) with the per-block argmax records k_argmax_final reads (one record per 64 rows)
struct BelieverArgs {
  const double* Xs;       // candidates, M x d row-major
  const double* theta;    // d (+ the exponent of generalized_exponential / the order of the general Matern kernel)
  const double* pt;       // d: the believed point
  const double* rT;       // [Np][Mc] the chunk's correlation columns
  const double* w_part;   // [S][Mc] slice sums of w . r (ordinary kriging)
  const double* avec;     // [N] R^-1 r(p)
  int d, N, S;
  int64_t Mc, mcount, m0, M;
  int update;             // 0: criterion only (a guarded pivot: c = 0), nothing above is read
  int64_t self_row;       // the candidate row that is the believed point (a winner), -1 for a pending point
  int n_taken;            // winners of the steps before: their rows keep their criterion value but leave the argmax
  int64_t taken[32];
  double u_p, inv_root;   // u(p); 1 / sqrt(pivot)
  double G;
  int estimate_trend;
  int nprev;              // stored columns this point is orthogonalised against
  int prev_slot[32];
  double prev_c[32];      // c_k(p)
  const double* C;        // [slots][M]
  double* c_out;          // [M] this point's column, or null (the last believed point)
  double* s;              // [M] in / out
  double sigma2;
  int eval;               // evaluate one criterion behind the update
  int acq_id, minimize;
  double acq_par, plugin;
  const double* mu;       // [M]
  double* acq_out;        // [M]
  double* mse_out;        // [M]
  double* blk_val;
  int64_t* blk_idx;
  int64_t blk_offset;
};
hipError_t launch_believer(int kernel, const BelieverArgs& a, hipStream_t st);

// What the m-target halves of a believer pass share (bogp_believer_multi.h), ONE launch over all M rows behind the chunk loop in which
// k_believer stored c(x): MSE_k(x) -= sigma2_k c(x)^2 per target and -- for the pass in front of a step -- that step's criterion on
// (mu, max(0, MSE)) with one argmax record per 256 rows.  believer_run fills every field (sigma2 from the handle's sigma2_t) and hands
// it to BelieverFamily::criterion; it is the first member, `step`, of the two constrained families' argument blocks below.  It stands
// here and not in bogp_believer_multi.h because that host code needs it and that header pulls in bogp_device.h.
struct BelieverStep {
  int64_t M;
  int m;                  // targets, 2 .. BOGP_MAX_TARGETS
  int update;             // 0: criterion only (a guarded pivot: c = 0), c is not read
  const double* c;        // [M] c(x) of the believed point
  int64_t self_row;       // the candidate row that is the believed point (a winner), -1 for a pending point
  double* s;              // [M][m] running MSE per target, in / out (unclamped below pass 0's own clamp)
  double sigma2[8];       // per target
  int eval;               // evaluate the criterion behind the update
  int n_taken;            // winners of the steps before: their rows keep their value but leave the argmax
  int64_t taken[32];
  const double* mu;       // [M][m]
  double* mse_out;        // [M][m] max(0, MSE): what the step saw
  double* blk_val;        // [ceil(M / 256)]
  int64_t* blk_idx;
};

// EHVI over the step's cells (kernels_believer_ehvi.hip).  This family holds no `step`: its kernel keeps the step's fields under
// their names in its own order, the cells in front of mse_out, and its own text (profiles/believer_multi_fold.txt section 7: through
// the embedded step and the helpers k_believer_ehvi<7> gained a branch); the family copies the step it is handed field by field.
struct BelieverEhviArgs {
  int64_t M;
  int m, update;
  const double* c;
  int64_t self_row;
  double* s;
  double sigma2[8];
  int eval, n_taken;
  int64_t taken[32];
  const double* mu;
  const double* lower;    // [C][m] cell bounds of the step's front (device)
  const double* upper;    // [C][m] (+inf allowed)
  int C;
  double* ehvi_out;       // [M]
  double *mse_out, *blk_val;
  int64_t* blk_idx;
};
hipError_t launch_believer_ehvi(const BelieverEhviArgs& a, hipStream_t st);

// the step's feasibility-weighted criterion in k_constrained's expressions (kernels_believer_constrained.hip): target 0 the
// objective, targets 1 .. m - 1 constraints feasible in [lo_k, hi_k]
struct BelieverConstrainedArgs {
  BelieverStep step;
  double lo[8], hi[8];    // per target; entry 0 is not read
  int acq_id, minimize;   // BOGP_ACQ_EI / EPSILON_PI / MGFI, or BOGP_ACQ_NONE: the probability of feasibility alone
  double acq_par, plugin;
  double* acq_out;        // [M]
  double* pof_out;        // [M]
};
hipError_t launch_believer_constrained(const BelieverConstrainedArgs& a, hipStream_t st);

// feasibility-weighted EHVI over the step's cells by k_ehvi_constrained's conventions (kernels_believer_ehvi_constrained.hip):
// targets 0 .. m_obj - 1 the objectives, target m_obj + j the constraint feasible in [lo[j], hi[j]]; step.m is 3 .. BOGP_MAX_TARGETS
struct BelieverEhviConstrainedArgs {
  BelieverStep step;
  int m_obj;              // objectives among the targets, 2 .. m - 1
  double lo[8], hi[8];    // per constraint: entry j belongs to target m_obj + j
  const double* lower;    // [C][m_obj] cell bounds of the step's feasible front (device); not read for C == 0
  const double* upper;    // [C][m_obj] (+inf allowed)
  int C;                  // 0: the probability of feasibility alone
  double* val_out;        // [M]
  double* pof_out;        // [M]
};
hipError_t launch_believer_ehvi_constrained(const BelieverEhviConstrainedArgs& a, hipStream_t st);

// q sample paths over a chunk (kernels_thompson.hip): path_j(x) = mu(x) + z_j(x) - r(x) . g_j - b_j with the random-Fourier-feature draw
// z_j(x) = sum_l W[l][j] cos(omega_l . x + phase_l), one np.argmax record per path and 64 rows
struct ThompsonArgs {
  const double* X;        // rows, row-major with d columns: the candidates, or the training points (mode 0)
  int64_t row0, mcount;   // first row of this launch; rows it serves
  int d, L, N, q;         // L: features, a multiple of 16; q <= 16 paths
  const double* omega;    // [L][d]
  const double* phase;    // [L]
  const double* W;        // [L][16] weights times sqrt(2 sigma2 / L), zero columns from q on
  int mode;               // 0: z alone; 1: beta + z (prior paths); 2: the conditioned paths (everything below is read)
  const double* rT;       // [Np][ld] the chunk's correlation columns
  int64_t ld;             // Mc: stride of rT and mu_part
  const double* ngt;      // [ceil(N / 4) * 4][16] MINUS g, zero padded rows and columns
  const double* mu_part;  // [S][ld] the producer's slice sums of r . gamma
  int S;
  double beta;
  double bt[16];          // b_j
  int minimize;           // the value is negated: records and stored values are in the criterion's sign
  double* vals;           // [q][M] at the global row, or null
  int64_t M;
  double* blk_val;        // [q][nblk_total], or null (no records)
  int64_t* blk_idx;
  int64_t blk_offset, nblk_total;
};
hipError_t launch_thompson(const ThompsonArgs& a, hipStream_t st);

// q batch members' joint sample paths of the m targets of a multi-target model over a chunk (kernels_thompson_constrained.hip):
// path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x), target 0 the objective, target t >= 1 a constraint feasible in
// [lo[t], hi[t]].  Per row and member A = feasible ? +-path_{j,0} : -inf and B = 0 - max_t(excess_t inv_sd[t]); one np.argmax record
// per score and 64 rows.  DEVICE column of (member j, target t): t q + j (the ABI's is j m + t; the host permutes W and coef).
struct ThompsonConstrainedArgs {
  const double* X;        // [M][d] the candidates
  int64_t row0, mcount;   // first row of this launch; rows it serves
  int d, L, N, q, m;      // L: features, a multiple of 16; q m <= 16
  const double* omega;    // [L][d]
  const double* phase;    // [L]
  const double* W;        // [L][16] weights times sqrt(2 sigma2_t / L) in device column order, zero columns from q m on
  const double* rT;       // [Np][ld] the chunk's correlation columns
  int64_t ld;             // Mc: stride of rT
  const double* coef;     // [ceil(N / 4) * 4][16] gamma_t - g_{j,t} in device column order, zero padded rows and columns
  double beta;
  double lo[8], hi[8], inv_sd[8];  // per target; entry 0 is not read
  int minimize;           // A = -path_{j,0} where feasible
  double* scores;         // [2 q][M] at the global row: row 2 j is A_j, row 2 j + 1 is B_j; or null
  double* paths;          // [q m][M] at the global row, row j m + t, in the path's own sign; or null
  int64_t M;
  double* blk_val;        // [2 q][nblk_total]
  int64_t* blk_idx;
  int64_t blk_offset, nblk_total;
};
hipError_t launch_thompson_constrained(const ThompsonConstrainedArgs& a, hipStream_t st);

// a packed regression forest over the current candidates (kernels_forest.hip): per-tree traversal -> mean / variance over
// the trees -> the q criteria of acq_value -> per-block argmax records, one launch for all M rows
struct ForestTree {  // one tree of the packed forest
  int first, n_nodes, n_leaves, depth;  // first word; records; values behind them; longest root-to-leaf path (bounds the walk)
  double inv_count;                     // 1 / (t + 1): the running mean's weight when tree t arrives
  double pad;
};
struct ForestArgs {
  const double* Xs;               // candidates, M x d row-major
  int64_t M;                      // rows of Xs
  int64_t row0, nrows;            // rows [row0, row0 + nrows) are evaluated by this launch
  int d;
  const unsigned long long* words;  // the packed trees: per tree [n_nodes node records | n_leaves leaf values (double bits)]
  const ForestTree* tree;         // [T]
  int T;
  int tree_words;                 // largest n_nodes + n_leaves of a tree: one LDS buffer
  double* mu_out;                 // [M] or null (indexed by the global row)
  double* mse_out;                // [M] or null
  double* leaves_out;             // [nrows][T] per-tree predictions or null (indexed by row - row0)
  int q;                          // 0: moments only
  int acq_id[64];
  double acq_par[64];
  double plugin;
  int minimize;
  double* acq_out;                // [q][M] or null
  double* blk_val;                // [q][nblk_total]
  int64_t* blk_idx;
  int64_t nblk_total;
};
size_t forest_lds_bytes(int d, int tree_words);  // dynamic LDS of one workgroup of k_forest / k_forest_ehvi
hipError_t launch_forest(const ForestArgs& a, hipStream_t st);

// a packed forest with m outputs per leaf over the current candidates (kernels_forest_ehvi.hip): per-tree traversal -> mean /
// variance over the trees per output -> EHVI over the cells -> per-block argmax records, one launch for all M rows.  A tree is
// [n_nodes records | n_leaves x m values], leaf-major; tree_words is the largest n_nodes + m n_leaves.
struct ForestEhviArgs {
  const double* Xs;               // candidates, M x d row-major
  int64_t M;                      // rows of Xs
  int64_t row0, nrows;            // rows [row0, row0 + nrows) are evaluated by this launch
  int d;
  const unsigned long long* words;
  const ForestTree* tree;         // [T]
  int T;
  int tree_words;
  int m;                          // outputs, 2 .. BOGP_MAX_TARGETS
  double* mu_out;                 // [M][m] or null (indexed by the global row)
  double* mse_out;                // [M][m] or null
  double* leaves_out;             // [nrows][T][m] per-tree predictions or null (indexed by row - row0)
  int C;                          // cells; 0: moments only (nothing below is touched)
  const double* lower;            // [C][m] cell bounds (device)
  const double* upper;            // [C][m] (+inf allowed)
  double* ehvi_out;               // [M] or null
  double* blk_val;                // [blocks of this launch] per-block partial argmax
  int64_t* blk_idx;
};
hipError_t launch_forest_ehvi(const ForestEhviArgs& a, hipStream_t st);

// the fused small-N sweep (kernels_small.hip): one launch = producer + contraction + posterior + q criteria + argmax
struct SmallArgs {
  const double* Xs;          // candidates, M x d row-major
  const double* sqrt_theta;  // d
  const double* XthT;        // [d][Np]
  const double* gamma;       // Np
  const double* wvec;        // Np
  const double2* Vp;         // packed L^-1
  int64_t M;
  int d, Np, NJ16, NKP;
  int need_var;              // 0: predict without MSE (no contraction)
  double beta, G, sigma2, plugin;
  int estimate_trend, minimize, q;
  int acq_id[64];
  double acq_par[64];
  double* mu_out;            // [M] or null
  double* mse_out;           // [M] or null
  double* acq_out;           // [q][M] or null
  double* blk_val;           // [q][nblk]
  int64_t* blk_idx;
  int64_t nblk;
  unsigned int* counter;     // device word, zero between launches: ticket of the last workgroup
  double* best_val;          // [q]
  int64_t* best_idx;
  long long* stamps;         // null, or 5 device words: wave-cycles producing / contracting / waiting / epilogue, waves
  int64_t m_begin;           // first candidate of THIS launch (set by launch_sweep_small: bulk launch 0, tail launch after it)
  int64_t blk_begin;         // first partial-argmax slot of this launch
  int final_launch;          // the launch whose last workgroup reduces the partial winners
};
bool sweep_small_supported(int Np, int d, int kernel);
int64_t sweep_small_blocks(int64_t M, int n_cu);
hipError_t launch_sweep_small(int kernel, const SmallArgs& a, int n_cu, hipStream_t st);

hipError_t launch_corr_chunk(int kernel, const CorrArgs& a, int nMt, int S, hipStream_t st);
hipError_t launch_contract(const ContractArgs& a, hipStream_t st, ContractTile& ct);
hipError_t launch_contract_cross(const ContractArgs& a, int ncp, hipStream_t st);
int contract_cols_per_group();
hipError_t launch_acquisition(const AcqArgs& a, hipStream_t st);
hipError_t launch_argmax_final(const double* blk_val, const int64_t* blk_idx, int64_t nblk, int64_t stride, int q,
                               double* out_val, int64_t* out_idx, hipStream_t st);

hipError_t launch_topk(const double* vals, int64_t M, int q, int k, double* blk_val, int64_t* blk_idx, double* out_val,
                       int64_t* out_idx, hipStream_t st);

// the box penalty of a lifted sweep and the compaction of its feasible rows (kernels_lift.hip)
struct LiftArgs {
  const double* Z;      // candidates of the reduced space, M x r row-major
  int64_t M;
  int r, D;             // reduced / original dimensions
  const double* lift;   // [A (r x D row-major) | mean (D) | center (D) | lo (D) | hi (D)]
  double* penalty;      // [M]: -(sum of the box violations of x_), -0.0 <=> feasible
  int* blk_count;       // [ceil(M / 256)] feasible rows per workgroup
};
size_t lift_lds_bytes(int r, int D);  // dynamic LDS of one workgroup of k_lift_penalty
hipError_t launch_lift_penalty(const LiftArgs& a, hipStream_t st);
hipError_t launch_lift_scan(const int* blk_count, int64_t nblk, int64_t* offsets, hipStream_t st);  // offsets: nblk + 1, the last = M_f
hipError_t launch_lift_compact(const double* Z, int64_t M, int r, const double* penalty, const int64_t* offsets, double* Zc,
                               int64_t* map, hipStream_t st);
// val[c][m] (q x M) = penalty[m], then val[c][map[i]] = acq[c][i] (q x Mf) for the Mf survivors
hipError_t launch_lift_merge(const double* penalty, int64_t M, const double* acq, const int64_t* map, int64_t Mf, int q,
                             double* val, hipStream_t st);

hipError_t launch_generate_uniform(double* Xs, int64_t n_elem, int d, const double* lo, const double* hi, uint64_t seed,
                                   uint64_t first_elem, hipStream_t st);
hipError_t launch_generate_lhs(double* Xs, int64_t n_elem, int d, const double* lo, const double* hi, uint64_t seed,
                               uint64_t first_elem, uint64_t n_strata, hipStream_t st);
hipError_t launch_candidates_transform(double* Xs, int64_t n_elem, int d, const double* spec, hipStream_t st);
// mixed spaces: column k is real (levels[k] == 0: lo + (hi - lo) u) or discrete with levels[k] = L levels
// (index = min(floor(u L), L - 1), value lo + index (hi - lo) / (L - 1)); levels holds d doubles
hipError_t launch_generate_mixed(double* Xs, int64_t n_elem, int d, const double* lo, const double* hi, const double* levels,
                                 uint64_t seed, uint64_t first_elem, hipStream_t st);
hipError_t launch_generate_sobol(double* Xs, int64_t n_elem, int d, const double* lo, const double* hi, const uint64_t* sv,
                                 int bits, uint64_t first_elem, hipStream_t st);

// fit-path kernels (kernels_fit.hip)
hipError_t launch_min_pdist2(const double* X, int M, int d, unsigned long long* out, hipStream_t st);
hipError_t launch_build_R(int kernel, const double* X, int N, int d, const double* theta, double off_scale, double diag,
                          double* R, int ld, hipStream_t st);
hipError_t launch_build_R_div(int kernel, const double* X, int N, int d, const double* theta, double mul, double div,
                              double diag, double* R, int ld, hipStream_t st);
hipError_t launch_resid_gamma(int kernel, bool div, const double* X, int N, int d, const double* theta, double a, double b,
                              double diag, const double* bvec, const double* gamma, double* res, hipStream_t st);
hipError_t launch_sub_const(const double* y, double c, double* out, int N, hipStream_t st);
hipError_t launch_add_vec(double* y, const double* x, int N, hipStream_t st);
hipError_t launch_scale_transpose(const double* X, int N, int d, int Np, const double* sqrt_theta, double* XthT, double* xnorm,
                                  hipStream_t st);
hipError_t launch_pack_V(const double* Vcm, int N, int ld, int Np, double2* Vp, hipStream_t st);
hipError_t launch_logdet(const double* L, int N, int ld, double* out, hipStream_t st);
// kernels_chol.hip: in-place lower Cholesky of a column-major matrix whose ld is a multiple of 64 (identity padded)
// ---- kernels_gemm.hip: the small dense products that used to be library calls ------------------------------------
struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  int m, n, k, ldc;
  long sai, sak;  // op(A)(i, kk) at A[i * sai + kk * sak]
  long sbj, sbk;  // op(B)(kk, j) at B[j * sbj + kk * sbk]
  double alpha, beta;
  int tri;  // 1 / 2: op(A) square lower / upper triangular (zeros stored): the k range of a row tile shrinks
  double* scratch;        // split K (gridDim.z > 1): [tile][slice][64 x 64] partial tiles
  unsigned int* tickets;  // one zeroed word per tile
};
struct GemmSplit {  // what launch_gemm needs to split K: scratch of `cap` doubles, `max_tiles` zeroed ticket words
  double* scratch;
  size_t cap;
  unsigned int* tickets;
  int max_tiles;
};
// C (m x n) = alpha op(A) op(B) + beta C, column-major; ta / tb != 0: the stored matrix is the transpose (any shape)
hipError_t launch_gemm(int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb,
                       double beta, double* C, int ldc, hipStream_t st, int tri = 0, const GemmSplit* sp = nullptr);
// out[c + r * ldo] = in[r + c * ldi], r < rows, c < cols, zero for cols <= c < ldo
hipError_t launch_transpose_pad(const double* in, int ldi, int rows, int cols, double* out, int ldo, hipStream_t st);
// kernels_chol.hip, k_mm128 on a plain product: out (128 TI x 128 TJ, ldo) = sum_{k < K} Rs(row, k) Cs(col, k), element (row, k)
// at Rs[row + k * ldr], (col, k) at Cs[col + k * ldc]; K a multiple of 16, every tile complete
hipError_t launch_mm128_gen(const double* Rs, int ldr, const double* Cs, int ldc, double* out, int ldo, int TI, int TJ, int K,
                            hipStream_t st);
hipError_t launch_pad_identity(double* A, int N, int ld, hipStream_t st);
// st2 + ev[2] (optional): a second stream and two events for the look-ahead of the large-matrix path; N (optional): the
// data columns -- [N, ld) is identity padding whose diagonal-block steps are skipped; chain_flags (optional, with st2 and ev):
// 2 * (ld / 64) words for the resident diagonal chain of the fused block columns (k_chol_chain)
int chol_wide_panels(int ld, int* widths, int cap);  // wide first panels launch_chol_lower takes at this leading dimension (host only)
hipError_t launch_chol_lower(double* A, int ld, double* Winv, int* info, hipStream_t st, hipStream_t st2 = nullptr,
                             hipEvent_t* ev = nullptr, double* scratch = nullptr, int N = 0, unsigned int* chain_flags = nullptr);
hipError_t launch_tri_inverse(const double* L, const double* Winv, double* V, double* U, double* T, int ld, hipStream_t st);
constexpr int UUT_PARTS = 4;  // R^-1 = U U^T is produced as this many K-slices (ld*ld doubles apart) that the consumers add
hipError_t launch_uut(const double* U, double* Rinv, int ld, hipStream_t st, int* nparts);
hipError_t launch_copy_lower(const double* L, int N, int ld, double* dst, hipStream_t st);
// the rank-1 terms of the likelihood gradient: vectors v + t * stride (t < n) with weights cA (theta contractions) and
// cB (R0 contraction); c0 multiplies R^-1
struct GradVecs {
  const double* v;
  size_t stride;
  int n;
  double c0;
  double cA[BOGP_MAX_TARGETS], cB[BOGP_MAX_TARGETS];
  const double* dcoef = nullptr;  // if set: cA = dcoef[0..7], cB = dcoef[8..15] read on the device (k_grad_coef) instead
};
hipError_t launch_grad_contract(int kernel, const double* X, int N, int d, const double* theta, const GradVecs& gv,
                                const double* qv, double c2, const double* Rinv, int ld, int nparts,
                                size_t part_stride, double* partial, int nblk, hipStream_t st);
hipError_t launch_grad_reduce(const double* partial, int nblk, int nout, double* out, hipStream_t st);
int grad_contract_blocks(int N);
size_t gemv2_scratch_doubles(int N);
// polynomial trends (p > 1)
hipError_t launch_trend_train(int trend, const double* X, int N, int d, double* F, hipStream_t st);
hipError_t launch_pack_Vx(const double* Vcm, int N, int ld, const double* At, int ldA, const double* Ginv, int p, int Ne, int Nt,
                          double2* Vp, hipStream_t st);
hipError_t launch_trend_rows(int trend, const double* Xs, int64_t m0, int64_t mcount, int64_t mrows, int d, int64_t Mc, const double* beta,
                             double* Rext, int p, int prows, double* mtrend, hipStream_t st);
hipError_t launch_trend_terms(int trend, const double* Xs, int64_t m0, int64_t mcount, int d, int64_t Mc, const double* beta,
                              double* T, double* mtrend, hipStream_t st);
// small polynomial bases after the fused producer: T = sum of the slice sums, c = T - f(x*), mtrend = f(x*) . beta, uu = c^T Sinv c in ONE launch
hipError_t launch_trend_small(int trend, const double* Xs, int64_t m0, int64_t mcount, int d, int64_t Mc, const double* beta, const double* t_part,
                              int S, int pv, int p, const double* Sinv, double* mtrend, double* uu, hipStream_t st);
hipError_t launch_rowdot(const double* Cm, const double* CS, int64_t Mc, int64_t mcount, int p, double* uu, hipStream_t st);
hipError_t launch_sumsq(const double* v, int N, double* out, hipStream_t st);
// the one-launch likelihood of a small training set (kernels_nllsmall.hip)
struct NllSmallArgs {
  const double* X;  // N x d, row-major
  const double* y;  // N
  int N, d;
  double theta[64];  // d entries
  double pexp;       // generalized_exponential's exponent
  double a, b, diag;  // off-diagonal = a corr (/ b if div), diagonal = diag: k_build_R's arguments
  int div, estimate_trend, mode;
  double beta, s2t_host;
  double* out_scal;  // 64 doubles (device address of pinned host memory)
  double* out_S;     // d + 3 doubles
  unsigned long long* flag;
  unsigned long long seq;
  // bogp_nll_batch: P parameter vectors, one workgroup each.  bpar[s][NS_BPAR] = theta (64) | pexp | a | b | diag | s2t_host | div of
  // slot s (what `theta` .. `s2t_host` above are for one evaluation), bout[s][NS_BOUT] = its 64 scalars | d + 3 sums, bticket = one
  // zeroed device word (the last workgroup publishes `seq`).  bpar == nullptr: the one-evaluation launch.
  const double* bpar = nullptr;
  double* bout = nullptr;
  unsigned int* bticket = nullptr;
  int P = 1;
  int bout_stride = 0;  // doubles per slot of bout: 64 scalars + the d + 3 sums
};
constexpr int NS_BPAR = 72;   // doubles per slot of NllSmallArgs::bpar
int nll_small_max_n();
bool nll_small_fits(int N, int d);
// the elimination at 64-block granularity (kernels_chol.hip: k_elim_*): 157 <= N <= 1024, constant basis, one target
struct ElimArgs {
  double* E;    // ld x ld, column-major: the state blocks (k_build_R's output to start with)
  double* Eb;   // 64 x ld (leading dimension 64): block row nb = the right-hand sides [y; 1; 0 ...]
  int ld, nb, N;
  double* yt;   // ld: L^-1 y
  double* ft;   // ld: L^-1 1
  double* logpart;  // nb: sum(log diag L_kk)
  int* info;
};
// one parameter vector of bogp_nll_batch on the elimination path: its workspace (fixed while the batch buffers live) and where this
// evaluation's parameters are (rewritten by every call) -- an array of these in device memory is what the *_b kernels index by slot
struct BatchSlot {
  const double* theta;  // d + 1 doubles: theta, then the exponent of generalized_exponential
  const double* par;    // [0] a, [1] b, [2] diag (k_build_R's arguments), [3] sigma2 + noise_var (noisy mode)
  ElimArgs ea;          // state blocks, block row nb, Yt, Ft, log-determinant parts; ea.info = (int*)(scal + 62)
  double* Winv;         // (nb + 1) x 64 x 64: inverses of the diagonal blocks
  double* panels;       // 2 x (ld + 64) x 64: the two raw panels
  double* xpanel;       // 4 x (nb + 1) x 64 x 64: the solved panels of split steps, by k mod 4 (k_elim_panel_b -> k_elim_update_b / updateG_b / updateS_b)
  double* Rinv;         // ld x ld
  double* gamma;        // Np
  double* scal;         // 64: [0..3] the likelihood's scalars, [32..48) the gradient's weights, [62] info
  double* partial;      // grad_contract_blocks(N) x (d + 1) tile sums
  double* S;            // d + 3 gradient sums
  unsigned int* ticket; // zeroed word of k_grad_finish_b
};
hipError_t launch_build_R_batch(int kernel, bool div, const double* X, int N, int d, const BatchSlot* slots, int P, int ld, hipStream_t st);
hipError_t launch_elim_batch(const BatchSlot* slots, int P, int ld, const double* y, int estimate_trend, int mode, double beta, hipStream_t st);
hipError_t launch_grad_contract_batch(int kernel, const double* X, int N, int d, const BatchSlot* slots, int P, int Np, int ld, hipStream_t st);
hipError_t launch_grad_finish_batch(const BatchSlot* slots, int P, int nblk, int nout, int ld, int N, int with_trace, double* bout,
                                    int bout_stride, unsigned long long* flag, unsigned long long seq, unsigned int* gticket, hipStream_t st);
hipError_t launch_fit_gather_batch(const BatchSlot* slots, int P, double* bout, int bout_stride, unsigned long long* flag,
                                   unsigned long long seq, unsigned int* gticket, hipStream_t st);
hipError_t launch_elim(const ElimArgs& a, const double* y, double* Winv, double* panels, double* Rinv, int ldr, double* gamma, double* scal,
                       double* coefw, int estimate_trend, int mode, double beta, double s2t_host, hipStream_t st);
hipError_t launch_nll_small(int kernel, bool grad, const NllSmallArgs& a, hipStream_t st);
hipError_t launch_fit_gather(const double* scal, const double* S, int nS, double* out_scal, double* out_S, unsigned long long* flag,
                             unsigned long long seq, hipStream_t st);
hipError_t launch_grad_coef(const double* scal, int n_t, int mode, int N, int krank, double s2t_host, double* coef, hipStream_t st);
hipError_t launch_gemv2(const double* M, int ld, int N, int tri, const double* x0, const double* x1, double* y0, double* y1,
                        double* scratch, hipStream_t st);
// Lfac != null: also scal[0] = sum(log(diag(Lfac))) (what launch_logdet writes, in the same launch)
hipError_t launch_fit_rho(const double* Yt, const double* Ft, int N, int estimate_trend, double beta, double* rho, double* scal,
                          hipStream_t st, const double* Lfac = nullptr, int ldL = 0, double* coef = nullptr, int mode = 0,
                          double s2t_host = 0.0);
hipError_t launch_grad_finish(const double* partial, int nblk, int nout, double* out, const double* Rinv, int ld, int nparts,
                              size_t part_stride, int N, const double* gamma, int with_trace, const double* scal, double* out_scal,
                              double* out_S, unsigned long long* flag, unsigned long long seq, unsigned int* ticket, hipStream_t st);
hipError_t launch_trace_gg(const double* Rinv, int ld, int nparts, size_t part_stride, int N, const double* gamma,
                           const double* qv, double* out, hipStream_t st);
hipError_t launch_point_hessian(const double* X, int N, int d, const double* theta, const double* x, const double* r,
                                const double* rdx, const double* gamma, double* H, hipStream_t st);
hipError_t launch_point_corr(int kernel, const double* X, int N, int d, const double* theta, const double* x,
                             double* r, double* rdx, hipStream_t st);

hipError_t launch_col_reduce(const double* r, const double* rt, int N, int B, const double* gamma, const double* wvec,
                             double* mu, double* wd, double* ss, hipStream_t st);
hipError_t launch_batch_corr(int kernel, const double* X, int N, int d, const double* theta, const double* Xb, int B,
                             double* r, double* s2, hipStream_t st);
hipError_t launch_batch_grad(int kernel, const double* X, int N, int d, const double* theta, const double* Xb, int B,
                             const double* r, const double* s2, const double* Z, const double* gamma,
                             const double* wvec, double* out, hipStream_t st);


// ---- one-point / B-point evaluation and the lock-step polish (kernels_point.hip) -------------------------------------
constexpr int BOGP_POINT_MAX_D = 320;   // = BOGP_MAX_DIM: input dimensions the finishing workgroup stages in LDS
constexpr int BOGP_POINT_ARG_D = 64;    // a single point of at most this many dimensions travels as a kernel argument
constexpr int POLISH_M = 8;             // curvature pairs of the lock-step L-BFGS
struct PointRhsArgs {
  const double* X;      // N x d training points, row-major
  const double* theta;  // d
  const double* Xb;     // B x d points (device), or null: ONE point in `x`
  double x[BOGP_POINT_ARG_D];
  double* rhs;          // [B][npass][Npp][NC]
  int N, d, Npp, npass;
};
struct PointTriArgs {
  const double* V;      // L^-1, column-major, leading dimension ld, exact zeros above the diagonal
  const double* gamma;  // Np
  const double* wvec;   // Np (zeros under simple kriging)
  const double* rhs;
  double* part;         // [B][npass][nRB + 1][2 NC] block records
  double* split_scratch;        // [B][npass][nRB + 1][nsplit][rb x NC] partial tiles of a split row block (nsplit > 1)
  unsigned int* split_counter;  // [B][npass][nRB + 1] arrival tickets of the splits, zero between launches
  int rb, nsplit;               // rows of V per workgroup (16 / 32 / 64); workgroups per row block
  unsigned int* counter;  // [B] arrival tickets, zero between launches
  double* out;          // [B][rec_stride]: mu, mse, acq (q), dmu (d), dmse (d), dacq (q x d)
  int ld, Npp, Nr32, nRB, npass, d;
  int rec_stride, q, want_dacq, estimate_trend, minimize;
  int acq_id[64];
  double acq_par[64];
  double plugin, beta, G, ftft, sigma2;
  const double* trend_rec;  // [B][2 + 2 d] = mu_t, uu, dmu_t, duu of a linear trend basis (k_point_trend_fin), or null: constant basis
  unsigned long long* done_flag;  // device-mapped pinned word k_point_finish stores `done_seq` into last (one-point calls), or null
  unsigned long long done_seq;
};
struct PolishArgs {
  double* state;        // [B][state_stride]
  const double* rec;    // the records k_point_tri wrote for the current trial points
  double* Xt;           // [B][d] trial points (read: the evaluated ones; written: the next ones)
  const double *lo, *hi;  // d each
  unsigned int* n_done;
  int d, q, rec_stride, state_stride, max_evals;
  double pgtol, factr_eps, first_step;
};
int point_columns_per_pass(int d);
int point_passes(int d);
void point_tri_geometry(int N, int d, int B, int* rb, int* nsplit);
hipError_t launch_point_rhs(int kernel, const PointRhsArgs& a, int B, hipStream_t st);
hipError_t launch_point_tri(const PointTriArgs& a, int B, hipStream_t st, bool finish = true);  // !finish: k_point_tri alone (another finishing kernel follows)
hipError_t launch_point_trend(const PointRhsArgs& ra, const double* W, int ldW, int p, const double* betav, const double* Sinv,
                              int estimate_trend, double* Tw, double* trec, int B, hipStream_t st);
// MFMA flavour of the B-point path (kernels_point.hip): ncp = point_mfma_columns(d) right-hand-side columns per point (0: d too large)
int point_mfma_columns(int d);
hipError_t launch_point_rhs_T(int kernel, const PointRhsArgs& a, int ncp, double* rT, long long Mc, int Np, int B, hipStream_t st);
hipError_t launch_point_gw(int ncp, const double* rT, long long Mc, const double* gamma, const double* wvec, int Nr32, int B, int nJ,
                           double* part, hipStream_t st);
hipError_t launch_point_finish_mfma(const PointTriArgs& a, int ncp, int B, hipStream_t st);
size_t polish_state_doubles(int d);
hipError_t launch_polish_step(const PolishArgs& a, int B, hipStream_t st);
// EHVI and its input gradient at B points of an m-target model (kernels_point_ehvi.hip): the finishing kernel behind k_point_rhs + k_point_tri
// (VALU flavour) in place of k_point_finish
struct PointEhviArgs {
  const double* part;   // [B][npass][nRB + 1][2 NC] block records of k_point_tri
  const double* rhs;    // [B][npass][Npp][NC] right-hand sides of k_point_rhs
  const double* gamma;  // [m][ld_gamma] the targets' gamma columns (gamma_base)
  const double* lower;  // [C][m] cell bounds (device)
  const double* upper;  // [C][m] (+inf allowed)
  double* out;          // [B][rec_stride]: mu_0, MSE_0, EHVI, dmu_0 (d), dMSE_0 (d), dEHVI (d) -- k_point_finish's record with q = 1
  double* mom;          // [B][mom_stride]: mu (m), MSE (m), dmu (m x d), dMSE (m x d), or null
  int ld_gamma, N, Npp, nRB, npass, d, rec_stride, mom_stride;
  int m, C, estimate_trend;
  double beta, G, ftft;
  double sigma2[8];     // per target
  unsigned long long* done_flag;  // as PointTriArgs
  unsigned long long done_seq;
};
hipError_t launch_point_ehvi_finish(const PointEhviArgs& a, int B, hipStream_t st);
// q feasibility-weighted criteria and their input gradients at B points of an m-target model (kernels_point_constrained.hip): the
// finishing kernel behind k_point_rhs + k_point_tri (VALU flavour) in place of k_point_finish; target 0 the objective, targets
// 1 .. m - 1 constraints feasible in [lo_k, hi_k] (ConstrainedArgs' convention)
struct PointConstrainedArgs {
  const double* part;   // [B][npass][nRB + 1][2 NC] block records of k_point_tri
  const double* rhs;    // [B][npass][Npp][NC] right-hand sides of k_point_rhs
  const double* gamma;  // [m][ld_gamma] the targets' gamma columns (gamma_base)
  double* out;          // [B][rec_stride]: mu_0, MSE_0, acq (q), dmu_0 (d), dMSE_0 (d), dacq (q x d) -- k_point_finish's record
  double* mom;          // [B][mom_stride]: P, dP (d), mu (m), MSE (m), dmu (m x d), dMSE (m x d), or null
  int ld_gamma, N, Npp, nRB, npass, d, rec_stride, mom_stride;
  int m, q, estimate_trend, minimize;
  double beta, G, ftft, plugin;
  double sigma2[8];     // per target
  double lo[8], hi[8];  // per target; entry 0 is not read
  int acq_id[64];       // BOGP_ACQ_EI / EPSILON_PI / MGFI, or BOGP_ACQ_NONE
  double acq_par[64];
  unsigned long long* done_flag;  // as PointTriArgs
  unsigned long long done_seq;
};
hipError_t launch_point_constrained_finish(const PointConstrainedArgs& a, int B, hipStream_t st);
// feasibility-weighted EHVI and its input gradient at B points of an (m_obj + n_con)-target model (kernels_point_ehvi_constrained.hip): the
// finishing kernel behind k_point_rhs + k_point_tri (VALU flavour) in place of k_point_finish; targets 0 .. m_obj - 1 the objectives of
// the cells, target m_obj + j the constraint feasible in [lo[j], hi[j]] (ConstrainedEhviArgs' convention).  The fields stand in the
// order the kernel reads them (sums, moments, constraints, cells, records), as ConstrainedEhviArgs' do.
struct PointEhviConstrainedArgs {
  const double* part;   // [B][npass][nRB + 1][2 NC] block records of k_point_tri
  const double* rhs;    // [B][npass][Npp][NC] right-hand sides of k_point_rhs
  const double* gamma;  // [m][ld_gamma] the targets' gamma columns (gamma_base)
  int ld_gamma, N, Npp, nRB, npass, d;
  int m, m_obj, estimate_trend;
  double beta, G, ftft;
  double sigma2[8];     // per target
  double lo[8], hi[8];  // per constraint: target m_obj + j
  const double* lower;  // [C][m_obj] cell bounds (device), or null for C == 0
  const double* upper;  // [C][m_obj] (+inf allowed)
  int C;                // 0: the probability of feasibility alone
  int rec_stride, mom_stride;
  double* out;          // [B][rec_stride]: mu_0, MSE_0, value, dmu_0 (d), dMSE_0 (d), dvalue (d) -- k_point_finish's record with q = 1
  double* mom;          // [B][mom_stride]: P, dP (d), E, dE (d), mu (m), MSE (m), dmu (m x d), dMSE (m x d), or null
  unsigned long long* done_flag;  // as PointTriArgs
  unsigned long long done_seq;
};
hipError_t launch_point_ehvi_constrained_finish(const PointEhviConstrainedArgs& a, int B, hipStream_t st);

}  // namespace bogp
