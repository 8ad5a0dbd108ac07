/* bogp.h -- C ABI of libbogp.so: the MI355X (gfx950) GP-surrogate + batch-acquisition engine.
 *
 * The reference (wangronin/Bayesian-Optimization, `bayes_optim` 0.3.0) is pure Python: it has no FFI for
 * this path.  The drop-in boundary is three Python duck-typed protocols; the entry
 * points below are what a binding for those protocols needs, and each one names the reference code it
 * replaces (paths relative to bayes_optim/).  `INTEGRATION.md` shows the ctypes stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every host array is C-contiguous float64 / int32 / int64
 *   - return value: 0 = BOGP_OK, < 0 = error code (never throws across the ABI);
 *     `bogp_last_error(h)` gives a human-readable message for the last failing call on that handle
 *   - BOGP_ERR_NOT_POSDEF is the "Cholesky failed" outcome (LAPACK-style info > 0); the Python host maps it to
 *     llf = -inf exactly like the reference maps LinAlgError (surrogate/gaussian_process/gpr.py:946-947,
 *     960-961, 978-979)
 *   - the library owns all device memory; the caller owns all host buffers
 *   - one handle per device; calls on one handle must be serialised by the caller (ctypes releases the GIL)
 *   - all arithmetic is IEEE float64 on the device; there is NO host/CPU fallback path
 */
#ifndef BOGP_H
#define BOGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bogp_handle bogp_handle;

/* error codes */
#define BOGP_ABI_VERSION 9 /* what bogp_abi_version() of a matching library returns */
#define BOGP_OK 0
#define BOGP_ERR_INVALID (-1)      /* bad argument / call order                                           */
#define BOGP_ERR_HIP (-2)          /* HIP runtime failure (or an in-kernel hand-over that timed out)       */
#define BOGP_ERR_NOT_POSDEF (-3)   /* correlation matrix not positive definite (potrf info > 0)            */
#define BOGP_ERR_UNSUPPORTED (-4)  /* valid in the reference but not built yet (see DESIGN.md "out of scope") */
#define BOGP_ERR_NO_DEVICE (-5)    /* no usable gfx950 device                                              */
#define BOGP_ERR_LLF_POSITIVE (-6) /* llf > 0: the reference rejects it as -inf (gpr.py:981-982)           */

/* correlation functions: surrogate/gaussian_process/kernel.py
 *   SE        squared_exponential :289-329   exp(-sum_k theta_k d_k^2)
 *   MATERN12  matern nu=0.5       :190       exp(-s),                     s = sqrt(sum_k theta_k d_k^2)
 *   MATERN32  matern nu=1.5       :193-196   (1+t) exp(-t),               t = sqrt(3) s   [corr="matern"]
 *   MATERN52  matern nu=2.5       :198-200   (1+t+t^2/3) exp(-t),         t = sqrt(5) s                    */
#define BOGP_KERNEL_SE 0
#define BOGP_KERNEL_MATERN12 1
#define BOGP_KERNEL_MATERN32 2
#define BOGP_KERNEL_MATERN52 3
#define BOGP_KERNEL_ABSEXP 4 /* absolute_exponential :247-286   exp(-sum_k theta_k |d_k|) */
#define BOGP_KERNEL_GENEXP 6 /* exp(-sum_k theta_k |d_k|^p), kernel.py:332-379; theta = [theta_1 .. theta_d, p] (d + 1 entries, or [theta, p]):
                                values only, like BOGP_KERNEL_CUBIC */
#define BOGP_KERNEL_MATERN_NU 7 /* matern with any nu > 0, kernel.py:201-207: (2^(1-nu) / Gamma(nu)) t^nu K_nu(t), t = sqrt(2 nu) s (scipy.special.kv there, a device
                                   K_nu here); theta = [theta_1 .. theta_d, nu] (or [theta, nu]); values only -- corr_grad_theta / corr_dx define nothing for it */
#define BOGP_KERNEL_CUBIC 5 /* prod_k max(0, 1 - 3 (theta_k d_k)^2 + 2 (theta_k d_k)^3), kernel.py:419-466: likelihood VALUE, commit,
                               predict, sweep -- no derivatives, like the reference (corr_grad_theta / corr_dx leave it undefined) */

/* estimation modes: gpr.py:252-263; parameter layouts gpr.py:1073-1086
 *   NOISELESS   par = [theta]          sigma2 = sum(rho^2)/(N-k)
 *   NOISY       par = [theta, sigma2]  R = (sigma2 R0 + noise_var I)/(sigma2 + noise_var)
 *   NOISE_ESTIM par = [theta, alpha]   R = alpha R0 + (1-alpha) I                                        */
#define BOGP_MODE_NOISELESS 0
#define BOGP_MODE_NOISY 1
#define BOGP_MODE_NOISE_ESTIM 2

/* acquisition functions: acquisition/acquisition_fun.py (EI :150-189, EpsilonPI/PI :192-235, UCB :107-147,
 * MGFI :238-310).  `acq_par` is unused for EI, epsilon for EPSILON_PI, alpha for UCB, t for MGFI.          */
#define BOGP_ACQ_EI 0
#define BOGP_ACQ_EPSILON_PI 1
#define BOGP_ACQ_UCB 2
#define BOGP_ACQ_MGFI 3

/* trend (prior mean) bases: surrogate/gaussian_process/trend.py; all three are built (fit, predict, sweep) */
#define BOGP_TREND_CONSTANT 0
#define BOGP_TREND_LINEAR 1    /* [1, x]                      trend.py:94-118  */
#define BOGP_TREND_QUADRATIC 2 /* [1, x, x_k x_j (j >= k)]    trend.py:121-142 */

#define BOGP_MAX_DIM 320   /* input dimensions d (64 x d doubles of LDS in the sweep's producer) */
#define BOGP_MAX_TARGETS 8 /* columns of y (n_targets, gpr.py:463) */
#define BOGP_MAX_Q 64    /* criteria evaluated in one sweep (ParallelBO batch size q) */
#define BOGP_MAX_TOPK 32 /* ranks returned per criterion by bogp_sweep_topk */
#define BOGP_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */

/* ---- lifetime ------------------------------------------------------------------------------------- */
int bogp_create(int device, bogp_handle** out);
void bogp_destroy(bogp_handle* h);
const char* bogp_last_error(const bogp_handle* h); /* h may be NULL: message of the last failed bogp_create */
int bogp_abi_version(void);                        /* bumps whenever a signature below changes            */

/* ---- training set --------------------------------------------------------------------------------
 * Replaces GaussianProcess._check_data (gpr.py:279-310): X (N x d, row-major), y (N x n_targets).
 * The pair-distance list D of the reference (gpr.py:48-61, 13.4 GB at N=8192,d=50) is never built.
 * 1 <= n_targets <= BOGP_MAX_TARGETS.  With several targets (gpr.py:463, 490, 502-505, 931-1040) the correlation
 * model and its factorisation are shared and Yt / rho / gamma / sigma2 exist once per target: bogp_nll returns the SUM
 * of the per-target likelihoods and of their gradients exactly as the reference forms them, bogp_commit commits all
 * targets, and every per-target consumer (bogp_get_state, bogp_predict, bogp_sweep*, bogp_gradient*) works on the
 * target chosen with bogp_select_target (0 after set_train / commit).  As in the reference, only a FIXED constant
 * trend works with n_targets > 1 (estimating it raises at gpr.py:787); REML is single-target.                  */
int bogp_set_train(bogp_handle* h, const double* X, const double* y, int N, int d, int n_targets);
int bogp_select_target(bogp_handle* h, int target);

/* ---- likelihood -----------------------------------------------------------------------------------
 * Replaces GaussianProcess.log_likelihood_concentrated(par, eval_grad) (gpr.py:920-1040):
 * correlation_matrix (:772-782) -> _compute_aux_var (:790-811: potrf, L^-1 y, trend QR, rho) -> llf ->
 * gradient (:994-1038: gamma, R^-1 = L^-T L^-1, corr_grad_theta contraction without the (N,N,d) tensor).
 *   par           [theta (n_theta = d or 1), then sigma2 | alpha per mode], NOT log10
 *   noise_var     nugget tau^2 (NOISY mode); ignored otherwise
 *   estimate_trend 1: beta is GLS-estimated (ordinary kriging);  0: fixed `beta` (simple kriging)
 *   llf           out, scalar
 *   grad          out, n_par doubles, d llf / d par (the un-scaled gradient the reference hands L-BFGS-B,
 *                 SURVEY 8a quirks); NULL to skip the gradient (saves R^-1 + contraction)
 * Returns BOGP_ERR_NOT_POSDEF / BOGP_ERR_LLF_POSITIVE where the reference returns -inf.                 */
int bogp_nll(bogp_handle* h, int kernel, int mode, const double* par, int n_par, double noise_var, int trend,
             int estimate_trend, double beta, double* llf, double* grad);

/* P likelihood (+ gradient) evaluations in ONE device round trip: the restarts of GaussianProcess._optimize_hyperparameter
 * (gpr.py:1127-1162) are independent L-BFGS-B runs whose objective calls (gpr.py:1113-1123 -> log_likelihood_concentrated) can be
 * evaluated together -- at the sizes of a BO run one evaluation occupies one workgroup of the 256 CUs.
 *   par   P x n_par row-major (row s: the parameter vector of slot s, layout as bogp_nll);  llf (P);  grad (P x n_par) or NULL
 *   info  P per-slot outcomes: BOGP_OK, BOGP_ERR_NOT_POSDEF, BOGP_ERR_LLF_POSITIVE (llf[s] then holds the finite value), or
 *         BOGP_ERR_INVALID (a non-finite / non-positive parameter: that slot is skipped, the others are evaluated); llf[s] is NaN
 *         and grad row s zero for a failed slot
 * Slot s returns exactly the bits the s-th of P sequential bogp_nll calls returns.  The return value is BOGP_OK when the batch ran
 * (whatever the slots' outcomes) and an error code for what stops a bogp_nll call before the device (bad ids, no training set, HIP).
 * N <= 156: one launch, one workgroup a slot; N <= 3072: the elimination kernels over P workspaces (2 ld^2 doubles a slot, groups
 * bounded by BOGP_BATCH_MAX_MB, default 8192); above, and for polynomial trends / several targets: the P sequential calls,
 * dealt over up to three handles of the library's own (the caller's + helpers with their own stream and factor buffers, one host
 * thread each; two above N = 4096; BOGP_NLL_WORKERS) so that independent evaluations interleave on the device -- C5: 15.4 -> 13.4 ms
 * per evaluation, a linear-trend model at N = 2048: 1.86 -> 0.98 ms.  The two batched paths leave the handle's factor buffers -- a
 * committed model -- untouched.                                                                                                */
int bogp_nll_batch(bogp_handle* h, int kernel, int mode, int P, const double* par, int n_par, double noise_var, int trend,
                   int estimate_trend, double beta, double* llf, double* grad, int* info);

/* ---- the restarts of the MLE in lock step --------------------------------------------------------------
 * Replaces the restart loop of GaussianProcess._optimize_hyperparameter (gpr.py:1127-1162: `random_start` runs of
 * scipy.optimize.fmin_l_bfgs_b over log10(parameters), one after the other) by R bound-constrained L-BFGS runs that advance
 * TOGETHER: every round evaluates the current trial point of each active run with one bogp_nll_batch call.  Kept from the reference:
 * the log10 search space and bounds (:1088-1090), the objective -llf(10^x) with the UN-scaled gradient -d llf / d par (:1113-1123),
 * +inf / zero gradient where the likelihood is rejected, fmin_l_bfgs_b's defaults (m = 10, factr = 1e7, pgtol = 1e-5) and its rule
 * that budgets are tested when an iterate is accepted, never inside a line search.  Relaxed (hence opt-in on the Python side): the
 * evaluation budget is shared by runs that all start, so `wait_iter` has nothing to count.
 *   restricted  0: concentrated likelihood (bogp_nll_batch);  1: REML (bogp_nll_restricted per slot; par layout gpr.py:826-834)
 *   x0          R x n_par starting points in log10 space (clipped into the bounds);  lo, hi: n_par log10 bounds
 *   eval_budget evaluations allowed in total over all runs (<= 0: 15000 per run)
 *   m, factr, pgtol  <= 0: the defaults above
 *   prune_reserve  0: every run keeps going until the shared budget is spent.  > 0: while fewer than this many evaluations per active
 *               run are left, the run with the worst value so far is stopped (status 2, its last iterate returned): the budget
 *               is concentrated on the leading runs as it runs out, where equal shares would leave all R runs unconverged
 *   flags       0: the reference's gradient.  BOGP_MLE_CHAIN_RULE: hand the optimiser d(-llf) / d log10(par) = ln(10) par d / d par,
 *               the gradient of the function it actually minimises -- NOT what the reference does (an extension: ~4 x fewer
 *               evaluations per run from a start inside a basin, an immediate stop on the flat plateau of huge theta)
 *   xopt (R x n_par, log10), fopt (R: -llf at xopt, +inf if a run never saw a finite value), n_evals (R), status (R: 0 projected
 *   gradient <= pgtol, 1 relative reduction <= factr eps, 2 budget, 3 iterations, 4 line search failed, 5 start not finite),
 *   n_rounds: batched device calls made; the last three may be NULL.                                                        */
#define BOGP_MLE_CHAIN_RULE 1 /* flags bit 0 */
int bogp_mle_batch(bogp_handle* h, int kernel, int mode, int restricted, int R, const double* x0, int n_par, const double* lo,
                   const double* hi, double noise_var, int trend, int estimate_trend, double beta, int eval_budget, int m, double factr,
                   double pgtol, int flags, int prune_reserve, double* xopt, double* fopt, int* n_evals, int* status, int* n_rounds);

/* ---- commit a fitted state ------------------------------------------------------------------------
 * Replaces the tail of GaussianProcess.fit (gpr.py:402-415) + compute_beta_gamma (:784-788): factorise at
 * the final parameters and keep L, V = L^-1 (packed for the MFMA sweep), gamma, beta, w = L^-T Ft on the
 * device.  Same arguments as bogp_nll.                                                                  */
int bogp_commit(bogp_handle* h, int kernel, int mode, const double* par, int n_par, double noise_var, int trend,
                int estimate_trend, double beta, double* llf);

/* Read the committed state back (so the Python attributes C, gamma, rho, Yt, Ft, G, Q, beta, sigma2 stay
 * populated and the object stays picklable, base.py:499-540).  Any pointer may be NULL.
 *   C (N x N row-major lower Cholesky factor, strict upper = 0), gamma/rho/Yt/Ft/Q (N), G, beta, sigma2,
 *   noise_var (scalars).                                                                                */
int bogp_get_state(bogp_handle* h, double* C, double* gamma, double* rho, double* Yt, double* Ft, double* Q,
                   double* G, double* beta, double* sigma2, double* noise_var);

/* ---- restricted (REML) likelihood ---------------------------------------------------------------------
 * Replaces GaussianProcess.log_likelihood_restricted(par, eval_grad) (gpr.py:813-918).  Parameter layout (:826-834):
 * NOISELESS [theta, sigma2]; NOISY [theta, sigma2] with the fixed `noise_var`; NOISE_ESTIM [theta, sigma2, noise_var].
 * All three trend bases (constant, linear, quadratic; estimated or fixed coefficients) with one target; with several targets (fixed
 * constant trend only, as everywhere) the VALUE the reference's arithmetic yields -- the scalar terms broadcast over the n_t x n_t matrix
 * rho^T rho and everything summed (:861-866) -- and BOGP_ERR_UNSUPPORTED for its gradient (ValueError there, :875, :896).  Quirks kept: the simple-kriging value subtracts the log-determinant term (:861-866);
 * exp(llf) > 1 is rejected (:868-871): BOGP_ERR_LLF_POSITIVE, with *llf = the finite value and grad (if requested)
 * filled as the reference returns it.  The state for prediction at REML parameters is the NOISY-mode one:
 * bogp_commit(mode = BOGP_MODE_NOISY, par = [theta, sigma2], noise_var).                                       */
int bogp_nll_restricted(bogp_handle* h, int kernel, int mode, const double* par, int n_par, double noise_var, int trend,
                        int estimate_trend, double beta, double* llf, double* grad);

/* ---- polynomial trend bases (trend.py:66-142) --------------------------------------------------------
 * `trend` in bogp_nll / bogp_commit selects the basis F: BOGP_TREND_CONSTANT (p = 1, the scalar `beta` argument),
 * BOGP_TREND_LINEAR (p = d + 1), BOGP_TREND_QUADRATIC (p = (d+1)(d+2)/2).  With estimate_trend = 1 the coefficients are
 * the GLS estimate (universal kriging, gpr.py:801-806: Ft = L^-1 F, Q G = Ft, rho = Yt - Q Q^T Yt, beta = G^-1 Q^T Yt);
 * with estimate_trend = 0 and p > 1 they are the p values last given to bogp_set_trend_beta (the scalar `beta` argument
 * is ignored).  The QR factor G has a positive diagonal (LAPACK's Householder G differs by row signs; beta, rho, the
 * predictor and the likelihood do not depend on them).
 *   bogp_trend_size       p for a basis id and d
 *   bogp_get_trend_state  Ft, Q (N x p row-major), G (p x p row-major), beta (p) of the committed model; any may be NULL */
int bogp_trend_size(int trend, int d);
int bogp_set_trend_beta(bogp_handle* h, const double* beta, int p);
int bogp_get_trend_state(bogp_handle* h, double* Ft, double* Q, double* G, double* beta);

/* ---- candidates -----------------------------------------------------------------------------------
 * M x d row-major float64.  `upload` copies from host (PCIe); `bind` adopts caller-owned DEVICE memory
 * (e.g. a torch tensor's data_ptr()) without copying -- it must stay alive until the next upload/bind.   */
int bogp_candidates_upload(bogp_handle* h, const double* Xs, int64_t M);
/* The same upload, overlapped with the sweep that follows: only the first 8 MB are copied here; the next bogp_predict / bogp_sweep /
 * bogp_sweep_topk copies the rows of candidate chunk c + 1 on a copy stream WHILE chunk c is contracted (a host-sampled ask() of
 * optimizer="sweep", acquisition/optim/__init__.py:55-153, no longer pays the H2D copy of its M x d candidates in front of the
 * sweep).  `Xs` must stay valid and unchanged until that next call returns -- it returns with every row resident, later calls
 * need the buffer no more.  One-launch sweeps (N <= 512) and single-chunk sweeps finish the upload first.                       */
int bogp_candidates_upload_lazy(bogp_handle* h, const double* Xs, int64_t M);
int bogp_candidates_bind(bogp_handle* h, const void* d_Xs, int64_t M);
/* `generate` draws M uniform points in the box [lo, hi] ON the device (replaces RealSpace._sample,
 * search_space/search_space.py:742-754, and the H2D copy): counter-based Philox4x32-10, element (row, k) is a pure
 * function of (seed, (first_row + row) * d + k), so shards of one stream are drawn independently per rank.
 * `read` copies chosen rows (e.g. the argmax) of the current candidates back: out is n x d.                  */
int bogp_candidates_generate(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                             int64_t first_row);
/* `generate_lhs`: rows [first_row, first_row + M) of an n_strata-point Latin hypercube (method "LHS",
 * search_space.py:747-751 -> pyDOE.lhs): per dimension one point in each of n_strata equal strata, the strata
 * visited in a keyed pseudo-random permutation (Feistel network + cycle walking, evaluated per element, so no sort
 * and no exchange between ranks), jitter inside the stratum from the uniform stream.
 * `generate_lhs_maximin`: what the reference's DoE call actually asks pyDOE for (search_space.py:751: lhs(dim, samples=N,
 * criterion="maximin"), pyDOE's _lhsmaximin): `iterations` (pyDOE: 5) independent M-point hypercubes in the UNIT cube --
 * trial t is stream seed + 0x9E3779B97F4A7C15 * t -- are measured by the minimum pairwise Euclidean distance (the O(M^2 d)
 * pair sweep of `min_pdist2`; M <= 2^18) and the FIRST design with the largest minimum (pyDOE's `if maxdist < min(d)`) is
 * generated into the box [lo, hi] (+ the transform below); its minimum distance and trial number are returned.  Whole
 * designs only (no row shards: the criterion needs every pair).
 * `min_pdist2`: min over i < j of |x_i - x_j|^2 of the current candidates (sequential, un-fused sum over the dimensions:
 * bit-reproducible), +inf for fewer than two points.
 * `generate_sobol`: points [first_index, first_index + M) of the unscrambled Sobol' sequence (method "sobol",
 * search_space.py:752-753 -> sobol_seq.i4_sobol_generate, whose skip = 1 is first_index = 1) for caller-supplied
 * direction numbers sv (d x bits, row-major, sv[k][b] is XORed in when bit b of the Gray code of the index is set --
 * the layout of scipy.stats.qmc.Sobol._sv); value = integer * 2^-bits, then lo + (hi - lo) * value.            */
int bogp_candidates_generate_lhs(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                                 int64_t first_row, int64_t n_strata);
int bogp_candidates_generate_sobol(bogp_handle* h, const double* lo, const double* hi, int64_t M, int64_t first_index,
                                   const uint64_t* sv, int bits);
int bogp_candidates_generate_lhs_maximin(bogp_handle* h, const double* lo, const double* hi, int64_t M, uint64_t seed,
                                         int iterations, double* best_min_dist, int* best_iteration);
int bogp_candidates_min_pdist2(bogp_handle* h, double* min_sq);
int bogp_candidates_read(bogp_handle* h, const int64_t* rows, int n, double* out);
/* Per-variable post-processing of the three generators above, as RealSpace._sample applies it (search_space.py:754:
 * `self.round(self.to_linear_scale(X))`): draw in the TRANSFORMED box (pass trans(lo), trans(hi) to the generator:
 * Real._bounds_transformed, variable.py:246), map every coordinate back with the inverse of its scale (variable.py:40-55)
 * and, where precision[k] >= 0, round to that many decimals and clip to [lo[k], hi[k]] (the variable's own bounds,
 * variable.py:250-257).  scale / precision / lo / hi hold d entries; scale == NULL && precision == NULL switches the
 * post-processing off again.  The setting persists on the handle until changed (it needs bogp_set_train for d).      */
#define BOGP_SCALE_LINEAR 0
#define BOGP_SCALE_LOG 1   /* x = exp(u)                      */
#define BOGP_SCALE_LOG10 2 /* x = 10^u                        */
#define BOGP_SCALE_LOGIT 3 /* x = 1 / (1 + exp(-u))           */
#define BOGP_SCALE_BILOG 4 /* x = sign(u) (exp(|u|) - 1)      */
int bogp_candidates_set_transform(bogp_handle* h, const int* scale, const int* precision, const double* lo, const double* hi);

/* ---- posterior ------------------------------------------------------------------------------------
 * Replaces GaussianProcess.predict(X, eval_MSE) (gpr.py:486-510) on the current candidates:
 * mu (M) and mse (M, may be NULL) are HOST buffers.  With mse == NULL the N^2-per-candidate variance contraction is
 * not run at all (the reference's eval_MSE=False path also returns before its triangular solve, :491).          */
int bogp_predict(bogp_handle* h, double* mu, double* mse);

/* ---- sweep: posterior + q acquisition criteria + argmax ---------------------------------------------
 * Replaces the inner maximiser behind acquisition/optim/__init__.py:55-153 (argmax_restart) for
 * optimizer="sweep", evaluating AcquisitionFunction.__call__ row by row (acquisition_fun.py:127-135,
 * 153-176, 208-217, 265-290; _predict :52-64; plugin :96-104) for q criteria that share (mu, MSE)
 * (ParallelBO._batch_arg_max_acquisition, bayes_opt.py:100-115).
 *   plugin    effective plugin as stored by ImprovementBased.plugin (already negated when maximising)
 *   minimize  0/1 as AcquisitionFunction.minimize
 *   best_val  out (q): acquisition value at the argmax;  best_idx out (q): np.argmax index (first
 *             maximum; a NaN, if present, wins at its first position) -- local to these M candidates
 *   acq_out   optional HOST buffer (q x M row-major) receiving every acquisition value; NULL to skip
 * best_val and best_idx may BOTH be NULL: the sweep is then only queued on the handle's stream (no host wait, no
 * read-back) and its winners stay on the device for the bogp_exchange_argmax call that follows (multi-GPU step).  */
int bogp_sweep(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
               double* best_val, int64_t* best_idx, double* acq_out);

/* Same sweep, returning the k best candidates per criterion (best_val, best_idx: q x k row-major, rank 0 = the
 * argmax; ties -> lower index; slots beyond M are (-inf, -1)).  Gives BO.pre_eval_check (bayes_opt.py:27-55)
 * and ParallelBO's q criteria fall-backs instead of the reference's random padding (base.py:282-289) when
 * several criteria -- or a criterion and the history -- agree on the same candidate.                        */
int bogp_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                    int k, double* best_val, int64_t* best_idx);

/* ---- sweep: expected hypervolume improvement of a multi-target model --------------------------------
 * Replaces the reference's EHVI.forward (multi_objective/analytic.py:176-274) as MOBO maximises it
 * (mobo.py:168-186), evaluated for every current candidate in one chunked device pass: the posterior of all m targets
 * (gpr.py:486-510; the correlation chunk and |L^-1 r|^2 shared, mu_k / MSE_k per target), sigma_k =
 * sqrt(max(MSE_k, 1e-9)) (analytic.py:233), and EHVI = sum over the C cells of prod_k E[(min(Y_k, u_ck) - l_ck)^+] --
 * the reference's sum over 2^m subsets of psi / nu factors, as one product.  Targets are maximised as given.
 *   m            targets of the committed model (n_targets), 2 <= m <= BOGP_MAX_TARGETS
 *   lower/upper  C x m row-major HOST arrays of cell bounds, 1 <= C <= BOGP_MAX_EHVI_CELLS; lower finite, upper >= lower
 *                and may be +inf (the exact limit; the reference clamps it to 1e10, :236-238); NaN is invalid
 *   k            1 <= k <= BOGP_MAX_TOPK winners: best_val / best_idx (k) follow bogp_sweep_topk's rules (rank 0 is the
 *                argmax, ties -> lower index, NaN maximal, slots beyond M are (-inf, -1))
 *   ehvi_out (M), mu_out (M x m), mse_out (M x m): optional HOST buffers (NULL to skip)
 * The time of the EHVI kernel is reported as acquisition_ms by bogp_last_timing.                               */
#define BOGP_MAX_EHVI_CELLS 65536
int bogp_sweep_ehvi(bogp_handle* h, int m, int C, const double* lower, const double* upper, int k, double* best_val,
                    int64_t* best_idx, double* ehvi_out, double* mu_out, double* mse_out);

/* ---- sweep: modelled constraints, feasibility-weighted criteria ---------------------------------------
 * The reference accepts the values of expensive constraints and drops them (BaseBO.tell: base.py:328; BaseMOBO.tell:
 * mobo.py:117-118); its cheap callables h / g are handled by a penalty or a filter.  Here the committed model has m = n_targets
 * >= 2 columns: target 0 is the objective, targets 1 .. m - 1 are constraints, constraint j feasible when lo_j <= c_j(x) <= hi_j
 * (g <= 0 is (-inf, 0]; |h| <= tol is [-tol, tol]).  Per candidate, from the posterior of all m targets (as bogp_sweep_ehvi forms
 * it, the same bits -- the correlation chunk and |L^-1 r|^2 are shared, so the constraints cost one more read of the chunk):
 *   PoF_j  = bogp_feasibility(mu_j, MSE_j, sigma2_j, lo_j, hi_j);  P = PoF_1 * ... * PoF_{m-1} (in this order, from 1.0)
 *   value_c = base_c * P,  base_c the criterion c of bogp_sweep on target 0 (EI, EpsilonPI or MGFI: the non-negative ones), or 1 for
 *             BOGP_ACQ_NONE: the probability of feasibility alone, the usual criterion while no feasible point is known
 *             (Gelbart, Snoek, Adams 2014).  UCB changes sign and is refused.  NaN propagates and is maximal in the argmax.
 *   n_con        m - 1;  lo / hi: n_con HOST values each, either may be infinite, NaN and hi < lo are invalid (hi == lo is allowed)
 *   k            1 <= k <= BOGP_MAX_TOPK: best_val / best_idx are q x k row-major and follow bogp_sweep_topk's rules
 *   acq_out (q x M), pof_out (M), mu_out (M x m), mse_out (M x m): optional HOST buffers (NULL to skip)
 * Always the chunked, unpruned sweep with the variance; the kernel's time is reported as acquisition_ms by bogp_last_timing.
 * BOGP_ERR_INVALID: no committed model, no candidates, n_targets < 2, n_con != n_targets - 1, q outside [1, BOGP_MAX_Q], k outside
 * [1, BOGP_MAX_TOPK], an id other than EI / EpsilonPI / MGFI / BOGP_ACQ_NONE, a parameter the criterion refuses, a NaN bound,
 * hi < lo, a null required array.  BOGP_ERR_UNSUPPORTED: a lift is set, the handle holds a forest, a polynomial trend basis.
 *
 * bogp_feasibility (host only, no handle, no device call): P(lo <= Y <= hi) for Y ~ N(mu, mse), sd = sqrt(mse) without a floor;
 * sd / sqrt(sigma2) < 1e-6 (EI's guard, acquisition_fun.py:153-176) gives the indicator of lo <= mu <= hi; otherwise, with
 * za = (lo - mu) / sd and zb = (hi - mu) / sd, Phi(-za) - Phi(-zb) for za > 0 and Phi(zb) - Phi(za) else (the difference is taken
 * in the tail the interval lies in), Phi(-inf) = 0 and Phi(+inf) = 1 exactly.                                           */
#define BOGP_ACQ_NONE (-1)
double bogp_feasibility(double mu, double mse, double sigma2, double lo, double hi);
int bogp_sweep_constrained(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize, int n_con,
                           const double* lo, const double* hi, int k, double* best_val, int64_t* best_idx, double* acq_out,
                           double* pof_out, double* mu_out, double* mse_out);

/* ---- sweep: modelled constraints of a multi-objective run, feasibility-weighted EHVI ------------------
 * The reference leaves this as a TODO (BaseMOBO.tell, mobo.py:117-118: "implement method to handle known, expensive constraints
 * `h_vals` and `g_vals`").  Here the committed model has n_targets = m_obj + n_con columns: targets 0 .. m_obj - 1 are the objectives,
 * maximised as given (bogp_sweep_ehvi's convention), targets m_obj .. m_obj + n_con - 1 are constraints, constraint j feasible when
 * lo_j <= c_j(x) <= hi_j.  Per candidate, from the posterior of all targets (as bogp_sweep_ehvi and bogp_sweep_constrained form it, the
 * same bits -- the correlation chunk and |L^-1 r|^2 are shared):
 *   P     = PoF_0 * ... * PoF_{n_con-1} (in this order, from 1.0),  PoF_j = bogp_feasibility(mu, MSE, sigma2 of target m_obj + j, lo_j, hi_j)
 *   E     = bogp_sweep_ehvi's EHVI of the objectives over the C cells (sd_k = sqrt(max(MSE_k, 1e-9)))
 *   value = +0.0 where P == 0.0 (whatever E is: such a row's cells are not evaluated);  otherwise E * P for C >= 1;  otherwise P for
 *           C == 0: the probability of feasibility alone, the criterion while no feasible observation exists (Gelbart, Snoek,
 *           Adams 2014).  A NaN P is not == 0: it propagates and is maximal in the argmax.
 *   m_obj        2 <= m_obj;  n_con >= 1;  m_obj + n_con == n_targets <= BOGP_MAX_TARGETS
 *   lower/upper  C x m_obj row-major HOST arrays of cell bounds as bogp_sweep_ehvi takes them, 0 <= C <= BOGP_MAX_EHVI_CELLS; with
 *                C == 0 both may be NULL
 *   lo / hi      n_con HOST values each, either may be infinite, NaN and hi < lo are invalid (hi == lo is allowed: every value is +0.0)
 *   k            1 <= k <= BOGP_MAX_TOPK winners: best_val / best_idx (k) follow bogp_sweep_topk's rules
 *   val_out (M), pof_out (M), mu_out (M x n_targets), mse_out (M x n_targets): optional HOST buffers (NULL to skip)
 * Always the chunked, unpruned sweep with the variance; the kernel's time is reported as acquisition_ms by bogp_last_timing.
 * BOGP_ERR_INVALID: no committed model, no candidates, m_obj < 2, n_con < 1, m_obj + n_con != n_targets, C outside
 * [0, BOGP_MAX_EHVI_CELLS], k outside [1, BOGP_MAX_TOPK], a non-finite lower cell bound, a NaN upper cell bound, upper < lower, a NaN
 * constraint bound, hi < lo, a null required array.  BOGP_ERR_UNSUPPORTED: a lift is set, the handle holds a forest, a polynomial
 * trend basis.                                                                                                          */
int bogp_sweep_ehvi_constrained(bogp_handle* h, int m_obj, int C, const double* lower, const double* upper, int n_con, const double* lo,
                                const double* hi, int k, double* best_val, int64_t* best_idx, double* val_out, double* pof_out,
                                double* mu_out, double* mse_out);

/* ---- sweep: Kriging-believer batches ------------------------------------------------------------------
 * q proposals per call from q criteria, where step j sees the variance conditioned on the points believed before it
 * (Ginsbourger, Le Riche, Carraro 2010).  The reference has no such strategy: ParallelBO's q criteria share one posterior
 * and differ only in a sampled t / alpha (bayes_opt.py:82-115; EI raises, :86), MOBO's "EHVI with Kriging believer" is a
 * TODO (mobo.py:168-178) and set_X_pending raises (multi_objective/analytic.py:95-96).  Believing y = mu(p) at fixed
 * hyper-parameters leaves the mean (gpr.py:490) unchanged and takes a rank-one term off the bracket of gpr.py:502-510.
 * With kappa0(x, x') = k(x, x') - r(x)^T R^-1 r(x') + u(x) u(x') (k the committed correlation, u = (w.r - 1) / G under
 * ordinary kriging, else 0) and the believed points p_1 .. p_B -- the pending rows first, then each step's winner:
 *   b_i(x) = kappa0(x, p_i) - sum_{k<i} c_k(x) c_k(p_i),  pivot_i = b_i(p_i),  c_i(x) = b_i(x) / sqrt(pivot_i),
 *   s_i(x) = s_{i-1}(x) - c_i(x)^2,  s_0(x) = kappa0(x, x),   MSE_j(x) = sigma2 max(0, s_B(x)),  mean mu(x)
 * A pivot <= 1e-12 (a training point of a noiseless model, a repeated point) gives c_i = 0.  On the candidate row that is a
 * winner, c_i(p_i)^2 = pivot_i = s_{i-1}(p_i): its s is set to exactly 0.  Step j maximises criterion j on (mu, MSE_j) with
 * bogp_sweep's argmax rule OVER THE ROWS THAT ARE NOT WINNERS YET: a winner's row keeps its criterion value in acq_out but does
 * not compete again (on its zero variance EpsilonPI is Phi(+-inf), exactly 1 once its mean has become the plugin, and UCB is
 * its bare mean), so the q winners are q distinct rows and q <= M is required.  Without pending points step 0 IS bogp_sweep
 * with criterion 0, bit for bit.
 *   q, acq_id, acq_par, plugin, minimize   as bogp_sweep; 1 <= q, q + n_pending <= BOGP_MAX_BELIEVED
 *   believe_plugin   1: the plugin of a step is the best of the given one and the means believed so far, in the
 *                    criterion's sign -- min(plugin, mu(p)) when minimising, min(plugin, -mu(p)) otherwise (the plugin
 *                    arrives negated when maximising: the largest believed mean); 0: as given
 *   pending          n_pending x d HOST rows (submitted, not yet evaluated), NULL for n_pending = 0
 *   best_val, best_idx (q), best_x (q x d, may be NULL): each step's winner among the current candidates
 *   pivots (n_pending + q), acq_out (q x M), mse_out (q x M): optional HOST buffers; row j is what step j saw
 * Per believed point: one solve R^-1 r(p) and ONE pass over the candidates (correlation producer + k_believer, 8 N bytes
 * per candidate; the producer runs once when one chunk holds all candidates); the N^2 contraction runs once, in pass 0.  Works on the current candidates however they were set.
 * BOGP_ERR_INVALID: no committed model, no candidates, q < 1, q > M, the limit exceeded, a null required array, a non-finite
 * pending entry.  BOGP_ERR_UNSUPPORTED: a polynomial trend basis, several targets, a lift on the handle, a communicator of
 * more than one rank.  The handle's model, candidates and later plain sweeps are unaffected.
 * `believer_last`: of the last call, the time of the producer launches, of the solves and of k_believer in ms, and the
 * candidate passes behind pass 0; any pointer may be NULL.                                                          */
#define BOGP_MAX_BELIEVED 32
int bogp_sweep_believer(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                        int believe_plugin, const double* pending, int n_pending, double* best_val, int64_t* best_idx,
                        double* best_x, double* pivots, double* acq_out, double* mse_out);
int bogp_believer_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* believer_ms, int* n_passes);

/* ---- sweep: Thompson-sampling batches ------------------------------------------------------------------
 * q sample paths of the committed surrogate over the current candidates, each with its k best rows.  The reference declares
 * GaussianProcess.sampling_prior / sampling_posterior and leaves both as `pass` (gpr.py:312-316).  By pathwise conditioning
 * (Matheron's rule on a random-Fourier-feature prior draw; Wilson et al. 2020), with R, r(x), sigma2, gamma, beta the committed
 * model's (mu(x) = beta + r(x) . gamma, MSE(x) = sigma2 (1 - r^T R^-1 r + u^2), gpr.py:486-510) and L features shared by the paths:
 *   z_j(x)    = sqrt(2 sigma2 / L) sum_l W[l][j] cos(omega_l . x + phase_l)          the prior draw
 *   s_j       = z_j(X) + sqrt(sigma2 (diag(R) - 1)) E[:, j]                           what it "observes" at the training rows
 *   b_j       = 1^T R^-1 s_j / (1^T R^-1 1) under ordinary kriging, 0 under simple kriging
 *   g_j       = R^-1 (s_j - b_j 1)
 *   path_j(x) = mu(x) + z_j(x) - r(x) . g_j - b_j                                     conditioned = 1
 *   path_j(x) = beta + z_j(x)                                                         conditioned = 0 (a prior path)
 * With omega drawn from the kernel's spectral density, phase ~ U[0, 2 pi) and W, E standard normal, E[path] = mu and
 * Var[path] = MSE.  ALL of the draw is an input, made on the host (bogp.thompson.draw); the library never sees a seed.  In the
 * noiseless mode -- the one served -- diag(R) = 1, so eps is validated and has no effect.
 *   q (1 .. BOGP_MAX_PATHS), L (a multiple of 16 in [16, BOGP_MAX_FEATURES])
 *   omega (L x d), phase (L), weights (L x q), eps (N x q or NULL = zeros): HOST arrays, row-major
 *   minimize   1: each path is minimised (its criterion is -path), 0: maximised;  k (1 .. BOGP_MAX_TOPK) ranks per path
 *   best_val, best_idx (q x k): the criterion values and rows by bogp_sweep's rule (first maximum, NaN maximal), rank 0 first;
 *              slots beyond M are (-inf, -1).  best_x (q x k x d, may be NULL; NaN rows for such slots)
 *   paths_out (q x M, may be NULL): the paths' own values;  coef_out ((N + 1) x q, may be NULL): the rows of g, then b
 * Per call: the draw at the training rows and one N x q solve with the committed factor; per candidate chunk the correlation
 * producer and k_thompson (kernels_thompson.hip: 8 N bytes and L cos per candidate for all q paths).  The N^2 variance
 * contraction never runs.  Every sum's order depends on N, d and L alone: the outputs are bit-identical for any BOGP_CHUNK_MB,
 * and path j does not depend on q.
 * BOGP_ERR_INVALID: no committed model, no candidates, q, L or k out of range, a null required array, a non-finite entry in
 * omega / phase / weights / eps.  BOGP_ERR_UNSUPPORTED: the noisy and noise-estimating modes (the reference pairs an unscaled
 * r(x) with a rescaled R there, gpr.py:949-979: no Gaussian process has that mean / MSE pair as its conditional law), a
 * polynomial trend basis, several targets, the cubic and generalized-exponential kernels (no spectral draw), a lift on the
 * handle, a forest, a communicator of more than one rank.  The handle's model, candidates and later sweeps are unaffected.
 * `thompson_last`: of the last call, the time of the producer launches, of the draw at the training rows with its solves, and
 * of k_thompson over the candidates in ms, and the chunks; any pointer may be NULL.                                        */
#define BOGP_MAX_PATHS 16
#define BOGP_MAX_FEATURES 16384 /* L: a multiple of 16, >= 16 */
int bogp_sweep_thompson(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                        const double* eps, int conditioned, int minimize, int k, double* best_val, int64_t* best_idx,
                        double* best_x, double* paths_out, double* coef_out);
int bogp_thompson_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks);

/* ---- sweep: Thompson-sampling batches under modelled constraints ------------------------------------------
 * Joint sample paths of the objective and the modelled constraints (Eriksson & Poloczek 2021, SCBO).  The model is
 * bogp_sweep_constrained's: a committed multi-target model with m = 1 + n_con targets, target 0 the objective, target t >= 1 a
 * constraint that is feasible in [lo[t-1], hi[t-1]]; noiseless mode, constant basis (a multi-target commit has a FIXED constant
 * trend, so the conditional law is the simple-kriging one and there is no b).  A call carries q batch members, q m <=
 * BOGP_MAX_PATHS columns; column (j, t) -- index j m + t in weights, eps, paths_out and coef_out -- is member j's path of
 * target t.  The L features are shared, weights and eps are per column, so the targets are independent as in the model:
 *   z_{j,t}(x)    = sqrt(2 sigma2_t / L) sum_l W[l][j m + t] cos(omega_l . x + phase_l)
 *   s_{j,t}       = z_{j,t}(X) + sqrt(sigma2_t (diag(R) - 1)) E[:, j m + t]
 *   g_{j,t}       = R^-1 s_{j,t}
 *   path_{j,t}(x) = beta + r(x) . (gamma_t - g_{j,t}) + z_{j,t}(x)
 * Selection per row x and member j, with c_t = path_{j,t}(x), s = -1 when minimising and +1 otherwise:
 *   e_t    = max(lo_t - c_t, c_t - hi_t, 0)
 *   viol   = max_{t >= 1} (e_t inv_sd_t),   inv_sd_t = 1 / sqrt(sigma2_t) (formed on the host)
 *   feas   = every (lo_t <= c_t) and (c_t <= hi_t) holds
 *   A_j(x) = feas ? s path_{j,0}(x) : -inf          the objective among the rows whose drawn constraints hold
 *   B_j(x) = 0.0 - viol                             the least violating row, for a member without a feasible row
 * A row with a NaN among its m path values has A = B = -inf.  viol is a maximum of single products: no sum is formed, so A and B
 * follow from the returned path values exactly.
 *   omega (L x d), phase (L), weights (L x q m), eps (N x q m or NULL = zeros): HOST arrays, row-major
 *   best_val, best_idx (q x 2 x k): per member the k best rows of A, then the k best rows of B, by bogp_sweep_topk's rules (first
 *              maximum, ties to the lower index, slots beyond M are (-inf, -1));  best_x (q x 2 x k x d, may be NULL)
 *   paths_out (q x m x M, may be NULL): the paths' own values;  coef_out (N x q m, may be NULL): g
 * Per call: the draw at the training rows and one N x q m solve; per candidate chunk the correlation producer and
 * k_thompson_constrained (kernels_thompson_constrained.hip).  The outputs are bit-identical for any BOGP_CHUNK_MB, with and
 * without paths_out, and a member's do not depend on the members beside it.
 * BOGP_ERR_INVALID: no committed model, no candidates, a model of one target (bogp_sweep_thompson serves it), n_con != n_targets
 * - 1, q < 1 or q m > BOGP_MAX_PATHS, L or k out of range, a null required array, a NaN bound, hi < lo, a non-finite entry in
 * omega / phase / weights / eps.  BOGP_ERR_UNSUPPORTED: the noisy and noise-estimating modes, the cubic and
 * generalized-exponential kernels, a polynomial trend basis, a lift on the handle, a forest, a communicator of more than one
 * rank.  `thompson_constrained_last`: as bogp_thompson_last, of the last constrained call.                                  */
int bogp_sweep_thompson_constrained(bogp_handle* h, int q, int L, const double* omega, const double* phase, const double* weights,
                                    const double* eps, int minimize, int n_con, const double* lo, const double* hi, int k,
                                    double* best_val, int64_t* best_idx, double* best_x, double* paths_out, double* coef_out);
int bogp_thompson_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* paths_ms, int* n_chunks);

/* ---- sweep: Kriging-believer batches for EHVI -------------------------------------------------------------
 * q proposals per call for a multi-objective run -- what the reference names and leaves open: `class MOBO: """EHVI with
 * Kriging believer"""` stands over `# TODO: implement the Kriging believer strategy` (mobo.py:168-178), and MOBO(n_point > 1)
 * .ask() ends in BaseBO._batch_arg_max_acquisition, which raises NotImplementedError (base.py:496-497).  The model is
 * bogp_sweep_ehvi's: m = 2 .. BOGP_MAX_TARGETS targets, constant basis, targets maximised as given.  With several targets the
 * bracket 1 - |L^-1 r|^2 + u^2 is shared, MSE_k = sigma2_k bracket (gpr.py:502-510), so kappa0, b_i, pivot_i and c_i are those of
 * bogp_sweep_believer above (pivot floor 1e-12 -> c_i = 0; the candidate row that is a winner gets variance exactly 0) and step j
 * sees the means unchanged and  MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2).
 * The front: F_0 = the non-dominated rows of `front` strictly above ref_point in every objective (of identical rows the first);
 * with believe_front = 1 every believed mean mu(p) (an m-vector: beta + r(p).gamma_k for a pending point, the sweep's own mean
 * for a winner) joins it, F_B = front(F_{B-1} u {mu(p_B)}); with 0 the front stays F_0 and only the variance is conditioned.
 * The cells of step j are bogp_ehvi_grid_cells of the front as it stands; EHVI is bogp_sweep_ehvi's (sd = sqrt(max(MSE, 1e-9))).
 * Step j takes the argmax by bogp_sweep's rule over the rows that are not winners yet; the q winners are q distinct rows.
 * Without pending points step 0 IS bogp_sweep_ehvi called with bogp_ehvi_grid_cells' cells, bit for bit.
 *   front        n_front x m HOST rows (objective vectors seen so far), NULL for n_front = 0: one cell [ref_point, +inf)
 *   pending      n_pending x d HOST rows, NULL for n_pending = 0;  1 <= q <= M, q + n_pending <= BOGP_MAX_BELIEVED
 *   best_val, best_idx (q): each step's winner.  Optional HOST buffers (NULL to skip): best_x (q x d), best_mu (q x m: the
 *   believed means), pivots (n_pending + q), n_cells (q: the cells step j used), ehvi_out (q x M), mse_out (q x M x m).
 * Per believed point: the solve of bogp_sweep_believer, one streaming pass (producer + k_believer for c(x), per chunk) and one
 * launch of k_believer_ehvi over all rows; the N^2 contraction runs once, in pass 0.
 * BOGP_ERR_INVALID: no committed model, no candidates, m != n_targets, m outside [2, BOGP_MAX_TARGETS], q < 1, q > M, the limit
 * exceeded, a null required array, a non-finite entry, more than BOGP_MAX_EHVI_CELLS cells at any step (the message names the
 * step and the count; step 0's count is checked before any device work).  BOGP_ERR_UNSUPPORTED: a polynomial trend basis, a
 * lift, a forest handle, a communicator of more than one rank.  The handle's model, candidates and later sweeps are unaffected.
 * `believer_ehvi_last`: of the last call, the time of the producer launches, of the solves, of k_believer and of
 * k_believer_ehvi in ms, and the candidate passes behind pass 0; any pointer may be NULL.
 *
 * `ehvi_grid_cells` (host only: no handle, no device call): the grid decomposition of the region above ref_point that the front
 * of Y (n x m) does not dominate -- along each of the first m - 1 axes the edges are ref_k, the distinct front coordinates and
 * +inf; cells in row-major order of the grid (last grid axis fastest); the last lower bound is the largest last coordinate of
 * the front points covering the column, else ref_m; the last upper bound +inf.  Only input values are selected, none computed.
 * Returns the cell count, also with lower == upper == NULL (count only; `cap` is then not looked at), or BOGP_ERR_INVALID: m
 * outside [2, BOGP_MAX_TARGETS], a non-finite input, a count above `cap` (rows of lower / upper) or BOGP_MAX_EHVI_CELLS.     */
int bogp_ehvi_grid_cells(int m, int n, const double* Y, const double* ref_point, double* lower, double* upper, int64_t cap);
int bogp_sweep_believer_ehvi(bogp_handle* h, int m, int q, const double* ref_point, const double* front, int n_front,
                             int believe_front, const double* pending, int n_pending, double* best_val, int64_t* best_idx,
                             double* best_x, double* best_mu, double* pivots, int* n_cells, double* ehvi_out, double* mse_out);
int bogp_believer_ehvi_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* ehvi_ms, int* n_passes);

/* ---- sweep: Kriging-believer batches under modelled constraints --------------------------------------------
 * q proposals per call for a run whose simulation returns the objective and its constraints (bogp_sweep_constrained's model:
 * target 0 the objective, targets 1 .. m - 1 constraints feasible in [lo_k, hi_k], constant basis).  The bracket is shared by
 * the m targets, so kappa0, b_i, pivot_i and c_i are those of bogp_sweep_believer (pivot floor 1e-12 -> c_i = 0; the candidate
 * row that is a winner gets variance exactly 0) and step j sees the means unchanged and
 *   MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2),   value_j = base_j * P   as bogp_sweep_constrained forms them
 * from these moments (sd = sqrt(MSE) without a floor, P the product of bogp_feasibility over the constraints in index order).
 * The criteria are exactly acq_id / acq_par (q of them: EI, EpsilonPI, MGFI or BOGP_ACQ_NONE; a BOGP_ACQ_NONE step stays
 * feasibility-only); the bounds, the hyper-parameters and sigma2_k stay fixed.
 * The plugin: with believe_plugin = 1, a believed point p whose m means mu(p) (beta + r(p).gamma_k for a pending point, the
 * sweep's own means for a winner) are feasible by belief -- lo_k <= mu_k(p) <= hi_k for every constraint -- lowers it,
 * plug = min(plug, +-mu_0(p)) (the plugin arrives in the criterion's own sign: negated when maximising); an infeasible one and
 * believe_plugin = 0 leave it.  Step j takes the argmax by bogp_sweep's rule over the rows that are not winners yet; the q
 * winners are q distinct rows.  Without pending points step 0 IS bogp_sweep_constrained(q = 1, criterion 0), bit for bit.
 *   n_con, lo, hi   as bogp_sweep_constrained;  pending: n_pending x d HOST rows, NULL for n_pending = 0
 *   1 <= q <= M, q + n_pending <= BOGP_MAX_BELIEVED
 *   best_val, best_idx (q): each step's winner.  Optional HOST buffers (NULL to skip): best_x (q x d), best_mu (q x m: the
 *   believed means), pivots (n_pending + q), plugin_out (q: the plugin step j used), acq_out (q x M), pof_out (q x M),
 *   mse_out (q x M x m).
 * Per believed point: the solve of bogp_sweep_believer, one streaming pass (producer + k_believer for c(x), per chunk) and one
 * launch of k_believer_constrained over all rows (8 (3 + 4 m) bytes a row); the N^2 contraction runs once, in pass 0.  No bit
 * depends on BOGP_CHUNK_MB.
 * BOGP_ERR_INVALID: no committed model, no candidates, everything bogp_sweep_constrained refuses about the targets, the criteria
 * and the bounds, q < 1, q > M, the limit exceeded, a null required array, a non-finite pending entry.  BOGP_ERR_UNSUPPORTED: a
 * forest handle, a lift, a polynomial trend basis, a communicator of more than one rank.  Every failure returns before the first
 * launch; the handle's model, candidates and later sweeps are unaffected.
 * `believer_constrained_last`: of the last call, the time of the producer launches, of the solves, of k_believer and of
 * k_believer_constrained in ms, and the candidate passes behind pass 0; any pointer may be NULL.                             */
int bogp_sweep_believer_constrained(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                                    int believe_plugin, int n_con, const double* lo, const double* hi, const double* pending,
                                    int n_pending, double* best_val, int64_t* best_idx, double* best_x, double* best_mu,
                                    double* pivots, double* plugin_out, double* acq_out, double* pof_out, double* mse_out);
int bogp_believer_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* criterion_ms,
                                   int* n_passes);

/* ---- sweep: Kriging-believer batches for constrained EHVI --------------------------------------------------
 * q proposals per call for a multi-objective run whose simulation also returns constraints (bogp_sweep_ehvi_constrained's model:
 * targets 0 .. m_obj - 1 the objectives, maximised as given, target m_obj + j the constraint feasible in [lo_j, hi_j], constant
 * basis).  The bracket is shared by the m = m_obj + n_con targets, so kappa0, b_i, pivot_i and c_i are those of
 * bogp_sweep_believer (pivot floor 1e-12 -> c_i = 0; the candidate row that is a winner gets variance exactly 0) and step j sees
 * the means unchanged and
 *   MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2),   value_j = EHVI_j * P   as bogp_sweep_ehvi_constrained forms them
 * from these moments: sd_k = sqrt(max(MSE_k, 1e-9)) for the objectives, P the product of bogp_feasibility over the constraints in
 * index order from 1.0, the value exactly +0.0 where P == 0, P alone over no cells, a NaN P propagated.
 * The front: F_0 = the non-dominated rows of `front` (the objective rows of the FEASIBLE observations) strictly above ref_point.
 * A believed mean mu(p) is the full m-vector (beta + r(p).gamma_k for a pending point, the sweep's own means for a winner).
 * With believe_front = 1 its objective part joins the front, F_B = front(F_{B-1} u {mu_{0..m_obj-1}(p_B)}), if and only if the
 * point is feasible by belief -- lo_j <= mu_{m_obj+j}(p) <= hi_j for every constraint, the test bogp_sweep_believer_constrained
 * applies to its plugin; a point infeasible by belief, and believe_front = 0, leave the front and condition the variances only.
 * The cells of step j are bogp_ehvi_grid_cells of the front as it stands.
 * feasibility_only != 0: no feasible observation exists; the criterion is P alone (C = 0, n_cells[j] = 0) in ALL q steps -- the
 * criterion is the caller's, as a BOGP_ACQ_NONE step of bogp_sweep_believer_constrained stays feasibility-only -- and no believed
 * mean starts a front.  It requires n_front = 0.
 * Step j takes the argmax by bogp_sweep's rule over the rows that are not winners yet; the q winners are q distinct rows.
 * Without pending points step 0 IS bogp_sweep_ehvi_constrained called with bogp_ehvi_grid_cells' cells (or C = 0), bit for bit.
 *   front        n_front x m_obj HOST rows, NULL for n_front = 0: one cell [ref_point, +inf) unless feasibility_only
 *   n_con, lo, hi   as bogp_sweep_ehvi_constrained;  pending: n_pending x d HOST rows, NULL for n_pending = 0
 *   1 <= q <= M, q + n_pending <= BOGP_MAX_BELIEVED
 *   best_val, best_idx (q): each step's winner.  Optional HOST buffers (NULL to skip): best_x (q x d), best_mu (q x m: the
 *   believed means), pivots (n_pending + q), n_cells (q: the cells step j used), val_out (q x M), pof_out (q x M),
 *   mse_out (q x M x m).
 * Per believed point: the solve of bogp_sweep_believer, one streaming pass (producer + k_believer for c(x), per chunk) and one
 * launch of k_believer_ehvi_constrained over all rows (8 (3 + 4 m) bytes a row plus the cell loop); the N^2 contraction runs
 * once, in pass 0.  No bit depends on BOGP_CHUNK_MB.
 * BOGP_ERR_INVALID: no committed model, no candidates, m_obj < 2, n_con < 1, m_obj + n_con != n_targets, q < 1, q > M, the limit
 * exceeded, a null required array, feasibility_only with n_front > 0, a non-finite entry of ref_point / front / pending, NaN
 * bounds or lo > hi, more than BOGP_MAX_EHVI_CELLS cells at any step (the message names the step and the count; step 0's count
 * is checked before any device work).  BOGP_ERR_UNSUPPORTED: a forest handle, a lift, a polynomial trend basis, a communicator
 * of more than one rank.  The handle's model, candidates and later sweeps are unaffected.
 * `believer_ehvi_constrained_last`: of the last call, the time of the producer launches, of the solves, of k_believer and of
 * k_believer_ehvi_constrained in ms, and the candidate passes behind pass 0; any pointer may be NULL.                        */
int bogp_sweep_believer_ehvi_constrained(bogp_handle* h, int m_obj, int q, const double* ref_point, const double* front, int n_front,
                                         int feasibility_only, int believe_front, int n_con, const double* lo, const double* hi,
                                         const double* pending, int n_pending, double* best_val, int64_t* best_idx, double* best_x,
                                         double* best_mu, double* pivots, int* n_cells, double* val_out, double* pof_out,
                                         double* mse_out);
int bogp_believer_ehvi_constrained_last(bogp_handle* h, double* corr_ms, double* solve_ms, double* update_ms, double* criterion_ms,
                                        int* n_passes);

/* ---- sweep in a reduced space: box-penalised criteria under a linear lift ---------------------------
 * Replaces PCABO's inner maximisation (extension.py:113-133): the criterion is maximised over a box of the REDUCED
 * space (r = the committed model's d, _compute_bounds :113-119) through penalized_acquisition (:62-86), which maps a
 * candidate z back, x_ = (z A + mean) + center (LinearTransform.inverse_transform, :56-59, in this order), and returns
 *   penalty = -( sum_{x_i < lo_i} (lo_i - x_i) + sum_{x_i > hi_i} (x_i - hi_i) )       INSTEAD of the criterion
 * whenever penalty != 0 (:73); x_ exactly on a bound is feasible.  Typically 95 .. 100 % of a uniform design of the reduced
 * box are such rows, so the device decides feasibility for all M rows first (M r D multiply-adds), compacts the feasible
 * rows in their original order (no atomics: deterministic), runs the sweep of bogp_sweep_topk on them alone and ranks
 * criterion values and penalties together.
 * `lift_set`: A (r x D row-major = pca.components_), mean (D = pca.mean_), center (D = LinearTransform.center; NULL = 0),
 * lo / hi (D, the original box; +-inf allowed).  Persists on the handle until bogp_lift_clear; needs a training set (r is
 * its d; a later bogp_set_train of another d makes the lifted sweep return BOGP_ERR_INVALID until the lift is set again).
 * BOGP_ERR_INVALID: no training set, a null array, D < 1, a non-finite A / mean / center, NaN bounds or lo > hi.
 * BOGP_ERR_UNSUPPORTED: D > BOGP_MAX_DIM, r > BOGP_LIFT_MAX_R (a candidate row is held in registers), r D >
 * BOGP_LIFT_MAX_RD (A is staged in LDS), a forest handle.  The plain calls (bogp_sweep, bogp_sweep_topk, bogp_predict)
 * never look at the lift; bogp_sweep_ehvi refuses a handle with a lift (BOGP_ERR_UNSUPPORTED).
 * `lift_sweep_topk`: q, acq_id, acq_par, plugin, minimize, k, best_val, best_idx (q x k) as bogp_sweep_topk, over
 *   value_c[m] = penalty[m] if penalty[m] != 0, else criterion_c(z_m) -- the value bogp_sweep defines for that row --
 * for ALL M current candidates: first maximum, ties -> lower index, a NaN wins at its first position, slots beyond M are
 * (-inf, -1); indices number the M candidates as uploaded / generated.  Without a feasible row the winner is the least
 * penalised row and no posterior pass runs; with every row feasible the result is bogp_sweep_topk's, bit for bit.  A
 * feasible row's value is what the plain sweep returns for that row among the feasible rows alone.
 *   n_feasible   out, may be NULL: feasible rows M_f
 *   value_out    optional HOST buffer (q x M row-major): value_c[m];  penalty_out  optional HOST buffer (M): penalty[m]
 *                (-0.0 for a feasible row)
 * BOGP_ERR_UNSUPPORTED: a forest handle, a communicator of more than one rank.  bogp_last_timing reports the pass over
 * the survivors (all zero when M_f = 0).
 * `lift_last`: M_f of the last lifted sweep, the time of its filter (penalty + scan + the read-back of M_f + compaction)
 * and of its merge + ranking, in ms; any pointer may be NULL.                                                        */
#define BOGP_LIFT_MAX_R 64    /* reduced dimensions r of a lift */
#define BOGP_LIFT_MAX_RD 4096 /* r x D of a lift: doubles of A one workgroup stages in LDS */
int bogp_lift_set(bogp_handle* h, int D, const double* A, const double* mean, const double* center, const double* lo,
                  const double* hi);
int bogp_lift_clear(bogp_handle* h);
int bogp_lift_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize, int k,
                         double* best_val, int64_t* best_idx, int64_t* n_feasible, double* value_out, double* penalty_out);
int bogp_lift_last(bogp_handle* h, int64_t* n_feasible, double* filter_ms, double* merge_ms);

/* ---- second model kind: a packed regression forest ---------------------------------------------------
 * Replaces RandomForest.predict(X, eval_MSE=True) (surrogate/random_forest.py:124-155): scikit-learn's Tree.predict per
 * tree on the row cast to float32, mu = mean over the T trees, MSE = std(ddof = 1)^2 over the trees -- and, on these
 * moments, the criteria of bogp_sweep (acquisition_fun.py:52-64, 127-135, 153-176, 208-217, 265-290; EI's guard is the
 * one of a model without sigma2, :166-169).  The trees are fitted on the host (scikit-learn); the device evaluates them.
 * A handle carries a Gaussian process (bogp_set_train) OR a forest, never both: each call refuses the other's handle.
 *
 * `forest_set`: T >= 2 trees over d columns as flat arrays in scikit-learn's layout; tree t owns nodes
 * [tree_offset[t], tree_offset[t + 1]) (at most 65535), child indices are relative to the tree, node 0 is its root, a
 * leaf has left == right == -1 and predicts value[node].  test[node] (NULL: all 0) selects the node's rule:
 *   0  x32 <= threshold -> left  (x32 = the row's entry rounded to float32, threshold a double: Tree.predict)
 *   1  x32 != threshold -> left  (a one-hot column of level `threshold`, split at 0.5, rewritten onto the raw column
 *      that holds the level INDEX; threshold must be an integer in [0, 2^24))
 * The call validates on the host -- children inside their tree, every node reached at most once (no cycle), feature in
 * [0, d), finite leaf values, no NaN threshold -- packs (8-byte nodes, thresholds rounded toward -inf to float32, which
 * decides x32 <= threshold identically) and records each tree's depth, which bounds the kernel's walk.  A malformed
 * forest returns BOGP_ERR_INVALID and launches nothing.  It establishes d for the candidate calls; a forest of another
 * d drops the current candidates and transform.  NaN candidates are not supported: a NaN entry goes right under rule 0.
 * `forest_predict`: mu (M), mse (M, may be NULL) of the current candidates, HOST buffers.
 * `forest_leaves`: the T per-tree predictions of rows [first_row, first_row + n), n x T row-major (tests, diagnostics).
 * `forest_sweep_topk`: q criteria (ids / parameters / plugin / minimize as bogp_sweep) over the current candidates and
 * the k best rows of each: best_val / best_idx are q x k (rank 0 the argmax, ties -> lower index, NaN maximal, slots
 * beyond M (-inf, -1)); acq_out (q x M) optional.  The winners stay on the device as those of bogp_sweep (k = 1) and
 * bogp_sweep_topk (k > 1) do, for bogp_exchange_*.  A row's result depends on the row and the forest alone: rows that
 * reach the same leaves get the same bits.  The kernel's time is reported as acquisition_ms by bogp_last_timing.
 * `forest_info`: out[7] = {T, d, nodes, leaves, largest depth, bytes of the packed forest, LDS bytes of a workgroup}. */
int bogp_forest_set(bogp_handle* h, int T, int d, const int64_t* tree_offset, const int32_t* feature, const double* threshold,
                    const int32_t* left, const int32_t* right, const double* value, const int32_t* test);
int bogp_forest_predict(bogp_handle* h, double* mu, double* mse);
int bogp_forest_leaves(bogp_handle* h, int64_t first_row, int n, double* per_tree);
int bogp_forest_sweep_topk(bogp_handle* h, int q, const int* acq_id, const double* acq_par, double plugin, int minimize,
                           int k, double* best_val, int64_t* best_idx, double* acq_out);
int bogp_forest_info(const bogp_handle* h, int64_t* out);
/* Forests with SEVERAL outputs, and the expected hypervolume improvement on their moments.  Replaces, for a RandomForest
 * fitted on y (N, m), RandomForest.predict (surrogate/random_forest.py:141-155: scikit-learn grows one tree structure whose
 * leaves hold m values, tree_.value (n_nodes, m, 1); mu = mean and MSE = std(ddof = 1)^2 over the trees, per output, both
 * (M, m)) and, on these moments, EHVI.forward (multi_objective/analytic.py:223-274) as MOBO maximises it on mixed spaces
 * (mobo.py:168-186) -- one kernel walks the forest and evaluates EHVI per candidate, with the arithmetic of bogp_sweep_ehvi
 * on the moments (sigma_k = sqrt(max(MSE_k, 1e-9)), one product per cell, an upper bound at +inf exact).
 * `forest_set_multi`: bogp_forest_set with `value` nodes x m row-major (tree_.value[:, :, 0]); 2 <= m <= BOGP_MAX_TARGETS,
 * the same validation walk, the same BOGP_ERR_UNSUPPORTED when the largest tree (n_nodes + m n_leaves words, twice) and
 * 256 rows of d features exceed a workgroup's LDS.  It replaces any forest the handle held.
 * `forest_outputs`: m of the handle's forest (1 after bogp_forest_set; 0 without a forest).
 * `forest_predict_multi`: mu (M x m), mse (M x m, may be NULL) of the current candidates, HOST buffers.
 * `forest_leaves_multi`: per-tree, per-output predictions of rows [first_row, first_row + n), n x T x m row-major.
 * `forest_sweep_ehvi`: m, C, lower, upper, k, best_val, best_idx, ehvi_out, mu_out, mse_out as bogp_sweep_ehvi (the same
 * limits BOGP_MAX_EHVI_CELLS / BOGP_MAX_TOPK, first maximum, ties -> lower index, NaN maximal, slots beyond M (-inf, -1));
 * m must equal the forest's outputs.  Rows that reach the same leaves get the same bits.  The kernel's time is reported
 * as acquisition_ms by bogp_last_timing.
 * The one-output calls (bogp_forest_predict / _leaves / _sweep_topk) return BOGP_ERR_UNSUPPORTED on a forest of several
 * outputs, these calls on a forest of one output; bogp_sweep_ehvi refuses every forest handle; a handle with a lift is
 * refused (BOGP_ERR_UNSUPPORTED).  A refused call launches nothing.                                                  */
int bogp_forest_set_multi(bogp_handle* h, int T, int d, int m, const int64_t* tree_offset, const int32_t* feature,
                          const double* threshold, const int32_t* left, const int32_t* right, const double* value,
                          const int32_t* test);
int bogp_forest_outputs(const bogp_handle* h);
int bogp_forest_predict_multi(bogp_handle* h, double* mu, double* mse);
int bogp_forest_leaves_multi(bogp_handle* h, int64_t first_row, int n, double* per_tree);
int bogp_forest_sweep_ehvi(bogp_handle* h, int m, int C, const double* lower, const double* upper, int k, double* best_val,
                           int64_t* best_idx, double* ehvi_out, double* mu_out, double* mse_out);
/* Candidates of a MIXED space drawn on the device (replaces SearchSpace._sample column by column: Real.sample,
 * search_space/variable.py:240-248, and _Discrete.sample, :260-278, whose randint(0, L) every Integer / Ordinal /
 * Discrete / Subset / Bool variable maps through its levels): the Philox stream of bogp_candidates_generate, element
 * (row, k) a pure function of (seed, (first_row + row) * d + k).  Per column k:
 *   BOGP_COLUMN_REAL      x = lo + (hi - lo) u, then the handle's scale / precision transform, as bogp_candidates_generate
 *   BOGP_COLUMN_DISCRETE  index = min(floor(u L), L - 1), L = n_levels[k] > 0; x = lo + index (hi - lo) / (L - 1)
 *                         (lo for L = 1): lo + index for an Integer column [lo, lo + L - 1]; the level index itself
 *                         for lo = 0, hi = L - 1, which the host maps to the level's label
 * as a double in the M x d matrix that bogp_candidates_read hands back.  Not np.random.randint's stream: no parity
 * with the reference's draws is claimed, as for the uniform generator.                                            */
#define BOGP_COLUMN_REAL 0
#define BOGP_COLUMN_DISCRETE 1
int bogp_candidates_generate_mixed(bogp_handle* h, const int* kind, const double* lo, const double* hi, const int* n_levels,
                                   int64_t M, uint64_t seed, int64_t first_row);

/* ---- input-gradient of the posterior at ONE point ---------------------------------------------------
 * Replaces GaussianProcess.gradient(x) (gpr.py:537-576, corr_dx :600-661): dmu (d), dmse (d).            */
int bogp_gradient(bogp_handle* h, const double* x, double* dmu, double* dmse);
/* The same for B points at once (Xb: B x d; dmu, dmse: B x d row-major); constant or (r05) linear trend basis, one target.  r03: k_point_rhs +
 * k_point_tri (csrc/kernels_point.hip) -- ONE pass over L^-1 per point serves all d + 1 right-hand sides.     */
int bogp_gradient_batch(bogp_handle* h, const double* Xb, int B, double* dmu, double* dmse);
/* Hessian of the posterior mean at x (GaussianProcess.Hessian, gpr.py:578-598), d x d row-major.  Squared exponential
 * only, like the reference's corr_Hessian (:663-734); constant / linear trend (their Hessians are zero, trend.py:88-116). */
int bogp_hessian(bogp_handle* h, const double* x, double* H);
/* Correlation matrix of the rows of X1 (n1 x d) at the committed theta: GaussianProcess.prior_cov(X1, corr=True)
 * (gpr.py:318-353).  R is n1 x n1 row-major; the covariance flavour is R scaled on the host (:350-351).               */
int bogp_prior_corr(bogp_handle* h, const double* X1, int n1, double* R);
/* One point, everything at once: what `criterion(x, return_dx=True)` needs (acquisition_fun.py:139-146, 181-188,
 * 220-227, 292-309 call predict, gradient and the closed form) -- mu, mse, dmu (d), dmse (d) and the q criterion values --
 * with a single host synchronisation.  This is the call the reference's DEFAULT inner optimiser (multi-restart
 * L-BFGS-B, base.py:201-243) makes thousands of times per ask().  Constant or (r05) linear trend basis -- the two the
 * reference's `gradient` differentiates (gpr.py:556-575; the quadratic basis has no Jacobian, trend.py:138-139) --, one target;
 * q may be 0.                                                                                                        */
int bogp_point_eval(bogp_handle* h, const double* x, int q, const int* acq_id, const double* acq_par, double plugin,
                    int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq);
/* The same for B points (Xb: B x d, host) in ONE device round trip, plus the criteria's own input-gradients -- the
 * `return_dx` chain rule of acquisition_fun.py:139-146 (UCB), 181-188 (EI), 220-227 (EpsilonPI), 292-309 (MGFI) evaluated
 * on the device, guards (zero gradient) included.  Outputs, row-major, any may be NULL: mu, mse (B), dmu, dmse (B x d),
 * acq (B x q), dacq (B x q x d).  The reference raises for more than one row (gpr.py:548-549); row b here is what its
 * one-row call returns for row b.  Constant trend basis.                                                      */
int bogp_point_eval_batch(bogp_handle* h, const double* Xb, int B, int q, const int* acq_id, const double* acq_par,
                          double plugin, int minimize, double* mu, double* mse, double* dmu, double* dmse, double* acq,
                          double* dacq);
/* Multi-start local maximisation of ONE criterion inside the box [lo, hi] (d each), all B starts in lock step on the
 * device: every iteration is one batched value + gradient evaluation of the B trial points (as bogp_point_eval_batch,
 * records stay on the device) and one optimiser step per start (projected L-BFGS, 8 curvature pairs, Armijo
 * backtracking; a start never moves to a worse point).  Replaces the restart loop of acquisition/optim/__init__.py:74-153
 * when it is started from the sweep's top-k -- the reference runs its restarts one after the other, one
 * point per call.  Stop rules per start as the reference configures scipy's L-BFGS-B (:94-101): projected gradient
 * below pgtol (1e-8), relative improvement below factr (1e6) x machine epsilon, or max_evals evaluations.
 * X0: B x d starting points (clipped into the box); Xout: B x d; fout: B (criterion value at Xout, >= the value at
 * X0); n_evals: B evaluations used, may be NULL.  any d up to BOGP_MAX_DIM (r05; r03-r04: d <= 64); constant or linear trend basis.                              */
int bogp_polish(bogp_handle* h, const double* X0, int B, const double* lo, const double* hi, int acq_id, double acq_par,
                double plugin, int minimize, int max_evals, double pgtol, double factr, double* Xout, double* fout,
                int* n_evals);
/* Expected hypervolume improvement AND its input gradient at B points of the committed m-target model (an extension: the
 * reference's EHVI has no gradient, analytic.py:99-274), and the lock-step polish on it.  k_point_rhs + k_point_tri run as for
 * bogp_point_eval_batch (FP64 VALU flavour for every B); k_point_ehvi_finish (csrc/kernels_point_ehvi.hip) then forms the m means
 * and their gradients from the m columns of gamma, MSE_k = sigma2_k (1 - |V r|^2 + u^2) clipped at 0, sd_k = sqrt(max(MSE_k, 1e-9))
 * (analytic.py:233) and, over the cells, EHVI = sum_c prod_k f_ck with f = sd (G(a) - G(b)), df/dmu = Phi(-a) - Phi(-b),
 * df/dsd = phi(a) - phi(b) (a = (l - mu) / sd, b = (u - mu) / sd, G(z) = phi(z) - z Phi(-z); the b terms are 0 for u = +inf).
 * dsd_k/dx = dMSE_k/dx / (2 sd_k) where MSE_k > 1e-9 and exactly 0 where the clamp or the clip is active.  The value agrees with
 * bogp_sweep_ehvi's to rounding (the summation orders differ); identical inputs give identical bits, and row b of a B-point call
 * equals the one-point call on that row whenever both run the same row-block split (csrc/kernels_point.hip: point_tri_geometry).
 *   m, C, lower, upper   as bogp_sweep_ehvi.  A call whose (m, C, bytes) equal the cells the previous call of these two left on
 *                        the device skips their check and upload (the BFGS loop makes thousands of one-point calls).
 *   `point_eval_ehvi`    Xb: B x d (host).  Outputs, row-major, any but ehvi may be NULL: ehvi (B), dehvi (B x d), mu, mse (B x m),
 *                        dmu, dmse (B x m x d).
 *   `polish_ehvi`        bogp_polish's loop, state, stop rules and read-back on this evaluation: X0, lo, hi, max_evals, pgtol,
 *                        factr, Xout, fout, n_evals as there; fout[b] >= EHVI(clip(X0[b])).
 * BOGP_ERR_INVALID: no committed model; m != n_targets or m < 2; C outside [1, BOGP_MAX_EHVI_CELLS], a non-finite lower bound, a
 * NaN upper bound or one below its lower bound; a null required pointer; B <= 0; lo > hi; max_evals <= 0.
 * BOGP_ERR_UNSUPPORTED: the cubic, generalized-exponential and general-nu kernels (no corr_dx); a polynomial basis;
 * d > BOGP_MAX_DIM; a forest on the handle.  The handle's active target, its candidates and later sweeps are unaffected. */
int bogp_point_eval_ehvi(bogp_handle* h, const double* Xb, int B, int m, int C, const double* lower, const double* upper,
                         double* ehvi, double* dehvi, double* mu, double* mse, double* dmu, double* dmse);
int bogp_polish_ehvi(bogp_handle* h, const double* X0, int B, const double* lo, const double* hi, int m, int C,
                     const double* lower, const double* upper, int max_evals, double pgtol, double factr, double* Xout,
                     double* fout, int* n_evals);
/* The feasibility-weighted criteria of bogp_sweep_constrained AND their input gradients at B points of the committed m-target model,
 * and the lock-step polish on one of them (an extension: the reference drops constraint values, base.py:328).  k_point_rhs +
 * k_point_tri run as for bogp_point_eval_ehvi (FP64 VALU flavour for every B); k_point_constrained_finish
 * (csrc/kernels_point_constrained.hip) then forms the m means and their gradients from the m columns of gamma, MSE_k = sigma2_k
 * (1 - |V r|^2 + u^2) clipped at 0, sd_k = sqrt(MSE_k) without a floor (as bogp_sweep_constrained), and
 *   F_k, dF_k/dmu, dF_k/dsd = bogp_feasibility_grad(mu_k, MSE_k, sigma2_k, lo_k, hi_k);   P = F_1 * ... * F_{m-1} (this order, from 1.0)
 *   value_c = base_c * P   (base_c as bogp_sweep_constrained: EI, EpsilonPI, MGFI on target 0, or 1 for BOGP_ACQ_NONE)
 *   dP/dx   = sum_k (prod_{j != k} F_j) (dF_k/dmu dmu_k/dx + dF_k/dsd dsd_k/dx),   dsd_k/dx = dMSE_k/dx / (2 sd_k)
 *   dvalue_c/dx = P (c_dy (+-dmu_0/dx) + c_dsd dsd_0/dx) + base_c dP/dx   (c_dy, c_dsd: bogp_point_eval_batch's chain-rule coefficients)
 * The products over j != k come from prefix and suffix products, never from a division.  A zero coefficient times anything is 0: P == 0
 * removes the first term, base_c == 0 the second, a guard of the criterion or of the feasibility (sd / sqrt(sigma2) < 1e-6: the
 * indicator) its own; where sd_0 == 0 exactly the criterion's coefficients are 0.  A gradient is never NaN where the value is finite.
 * The values agree with bogp_sweep_constrained's to rounding (the summation orders differ); identical inputs give identical bits, the
 * bits of a criterion do not depend on the other criteria of the call, and row b of a B-point call equals the one-point call on that
 * row whenever both run the same row-block split (csrc/kernels_point.hip: point_tri_geometry).
 *   q, acq_id, acq_par, plugin, minimize, n_con, lo, hi   as bogp_sweep_constrained.
 *   `point_eval_constrained`  Xb: B x d (host).  Outputs, row-major, any but acq may be NULL: acq (B x q), dacq (B x q x d), pof (B),
 *                        dpof (B x d), mu, mse (B x m), dmu, dmse (B x m x d).
 *   `polish_constrained` bogp_polish's loop, state, stop rules and read-back on this evaluation of ONE criterion: X0, box_lo, box_hi
 *                        (the box), max_evals, pgtol, factr, Xout, fout, n_evals as there; a start never moves to a worse point, Xout
 *                        lies in the box and fout[b] >= value(clip(X0[b])).
 * BOGP_ERR_INVALID: no committed model, n_targets < 2, n_con != n_targets - 1, q outside [1, BOGP_MAX_Q], UCB or an id other than EI /
 * EpsilonPI / MGFI / BOGP_ACQ_NONE, a parameter the criterion refuses, a NaN bound, hi < lo, a null required pointer, B <= 0,
 * box_lo > box_hi, max_evals <= 0.  BOGP_ERR_UNSUPPORTED: the cubic, generalized-exponential and general-nu kernels (no corr_dx); a
 * polynomial basis; d > BOGP_MAX_DIM; a forest on the handle.  The handle's active target, its candidates and later sweeps are
 * unaffected.
 *
 * bogp_feasibility_grad (host only, no handle, no device call): out3 = [F, dF/dmu, dF/dsd] with F = bogp_feasibility(...) itself (the
 * same bits) and, with sd = sqrt(mse), za = (lo - mu) / sd, zb = (hi - mu) / sd:  dF/dmu = (phi(za) - phi(zb)) / sd,  dF/dsd =
 * (za phi(za) - zb phi(zb)) / sd.  An infinite side contributes exactly 0 to both; under the guard sd / sqrt(sigma2) < 1e-6 both are
 * exactly 0; lo == hi gives (0, 0, 0), two infinite sides (1, 0, 0).  Returns BOGP_ERR_INVALID for a null out3, else BOGP_OK. */
int bogp_feasibility_grad(double mu, double mse, double sigma2, double lo, double hi, double* out3);
int bogp_point_eval_constrained(bogp_handle* h, const double* Xb, int B, int q, const int* acq_id, const double* acq_par, double plugin,
                                int minimize, int n_con, const double* lo, const double* hi, double* acq, double* dacq, double* pof,
                                double* dpof, double* mu, double* mse, double* dmu, double* dmse);
int bogp_polish_constrained(bogp_handle* h, const double* X0, int B, const double* box_lo, const double* box_hi, int acq_id, double acq_par,
                            double plugin, int minimize, int n_con, const double* lo, const double* hi, int max_evals, double pgtol,
                            double factr, double* Xout, double* fout, int* n_evals);
/* The criterion of bogp_sweep_ehvi_constrained AND its input gradient at B points of the committed (m_obj + n_con)-target model, and the
 * lock-step polish on it (an extension: BaseMOBO.tell leaves constraint values as a TODO, mobo.py:117-118).  k_point_rhs + k_point_tri
 * run as for bogp_point_eval_ehvi (FP64 VALU flavour for every B); k_point_ehvi_constrained_finish
 * (csrc/kernels_point_ehvi_constrained.hip) then forms the moments of all targets as its two siblings do -- mu_k, MSE_k = sigma2_k
 * (1 - |V r|^2 + u^2) clipped at 0, dmu_k/dx = gamma_k . dr/dx, dMSE_k/dx = sigma2_k ds/dx -- and, with targets 0 .. m_obj - 1 the
 * objectives (maximised as given) and target m_obj + j the constraint feasible in [lo_j, hi_j]:
 *   objectives   sd_k = sqrt(max(MSE_k, 1e-9)); dsd_k/dx = dMSE_k/dx / (2 sd_k) where MSE_k > 1e-9 and exactly 0 otherwise
 *   constraints  sd_k = sqrt(MSE_k) without a floor;  F_j, dF_j/dmu, dF_j/dsd = bogp_feasibility_grad(mu, MSE, sigma2, lo_j, hi_j)
 *   P = F_0 * ... * F_{n_con-1} (this order, from 1.0);  dP/dx = sum_j (prod_{l != j} F_l) (dF_j/dmu dmu/dx + dF_j/dsd dsd/dx)
 *   E, dE/dmu_k, dE/dsd_k over the C cells of the objectives as bogp_point_eval_ehvi;  dE/dx = sum_{k < m_obj} (dE/dmu_k dmu_k/dx + dE/dsd_k dsd_k/dx)
 *   P == 0.0:   value = +0.0 exactly, gradient 0 in every component (by definition, as in the sweep; the cells are not read)
 *   C == 0:     value = P,   gradient dP/dx
 *   otherwise:  value = E P, gradient (P != 0 ? P dE/dx : 0) + (E != 0 ? E dP/dx : 0)
 * The products over l != j come from prefix and suffix products, never from a division; a zero coefficient times anything is 0.  A NaN
 * P is not == 0 and propagates; a gradient is never NaN where the value is finite.  The values agree with bogp_sweep_ehvi_constrained's
 * to rounding (the summation orders differ); identical inputs give identical bits, and row b of a B-point call equals the one-point
 * call on that row whenever both run the same row-block split (csrc/kernels_point.hip: point_tri_geometry).
 *   m_obj, C, lower, upper, n_con, lo, hi   as bogp_sweep_ehvi_constrained: 0 <= C <= BOGP_MAX_EHVI_CELLS, lower / upper C x m_obj and
 *                        may be NULL for C == 0.  Cells equal to those this path left on the device -- same m_obj, C and bytes -- are not
 *                        checked or uploaded again (the BFGS loop makes thousands of one-point calls over one front).
 *   `point_eval_ehvi_constrained`  Xb: B x d (host).  Outputs, row-major, any but val may be NULL: val (B), dval (B x d), pof (B),
 *                        dpof (B x d), ehvi (B), dehvi (B x d) -- both 0 where P == 0 or C == 0: the cells were not read --, mu, mse
 *                        (B x m), dmu, dmse (B x m x d), m = m_obj + n_con.
 *   `polish_ehvi_constrained`  bogp_polish's loop, state, stop rules and read-back on this evaluation: X0, box_lo, box_hi (the box),
 *                        max_evals, pgtol, factr, Xout, fout, n_evals as there; a start never moves to a worse point, Xout lies in the
 *                        box and fout[b] >= value(clip(X0[b])).
 * BOGP_ERR_INVALID: no committed model, m_obj < 2, n_con < 1, m_obj + n_con != n_targets, C out of range, a cell bound that is not
 * finite (lower), NaN or below its lower bound (upper), a NaN constraint bound, hi < lo, a null required pointer, B <= 0,
 * box_lo > box_hi, max_evals <= 0.  BOGP_ERR_UNSUPPORTED: the cubic, generalized-exponential and general-nu kernels (no corr_dx); a
 * polynomial basis; d > BOGP_MAX_DIM; a forest on the handle.  The handle's active target, its candidates and later sweeps are
 * unaffected. */
int bogp_point_eval_ehvi_constrained(bogp_handle* h, const double* Xb, int B, int m_obj, int C, const double* lower, const double* upper,
                                     int n_con, const double* lo, const double* hi, double* val, double* dval, double* pof, double* dpof,
                                     double* ehvi, double* dehvi, double* mu, double* mse, double* dmu, double* dmse);
int bogp_polish_ehvi_constrained(bogp_handle* h, const double* X0, int B, const double* box_lo, const double* box_hi, int m_obj, int C,
                                 const double* lower, const double* upper, int n_con, const double* lo, const double* hi,
                                 int max_evals, double pgtol, double factr, double* Xout, double* fout, int* n_evals);

/* ---- multi-GPU: the one exchange step per sweep ------------------------------------------
 * Nothing like it exists in the reference (its only parallelism is joblib over the q criteria, bayes_opt.py:108-111);
 * this is the cross-rank half of the new inner maximiser behind acquisition/optim/__init__.py:55-153.  One process per
 * GPU, each with its own handle and its own contiguous block of the M candidates; the model is replicated by redundant,
 * deterministic factorisation (no broadcast).  After bogp_sweep / bogp_sweep_topk every rank calls bogp_exchange_*: its q
 * (or q x k) winners -- (value, LOCAL index + index_offset, point) -- are packed on the device from the sweep's own result
 * buffers, gathered with ONE ncclAllGather (RCCL over xGMI; q (2 + d) doubles per rank), read back once, and reduced by
 * the same deterministic rule on every rank: np.argmax over the concatenation of all shards (largest value; a NaN beats
 * every number; ties -> lowest global index).  All ranks return identical results.
 *   bogp_comm_unique_id   fills BOGP_COMM_ID_BYTES bytes (ncclGetUniqueId); call on ONE rank, hand the bytes to all
 *                         ranks by any means (MPI_Bcast, a file, torch.distributed's store ...)
 *   bogp_comm_init        ncclCommInitRank on the handle's device; collective over the `world` ranks; world = 1 is fine
 *   bogp_comm_attach      borrow an existing ncclComm_t instead (not destroyed with the handle)
 *   bogp_comm_info        rank / world of the handle's communicator (world = 0: none)
 *   bogp_exchange_argmax  after bogp_sweep:      best_val (q), best_gidx (q), best_x (q x d, may be NULL)
 *   bogp_exchange_topk    after bogp_sweep_topk: best_val, best_gidx (q x k), best_x (q x k x d, may be NULL); global
 *                         k best per criterion in the same order; empty slots (-inf, -1, NaN)
 *   bogp_reduce_pairs / bogp_merge_topk   the reduce itself on HOST records [R][q( x k)][2 + d] = (value, index bit
 *                         pattern, point) for callers that gather by their own transport (MPI, gloo); need no handle. */
int bogp_comm_unique_id(unsigned char* id_out);
int bogp_comm_init(bogp_handle* h, const unsigned char* id, int rank, int world);
int bogp_comm_attach(bogp_handle* h, void* nccl_comm);
int bogp_comm_info(const bogp_handle* h, int* rank, int* world);
int bogp_comm_destroy(bogp_handle* h);
int bogp_exchange_argmax(bogp_handle* h, int64_t index_offset, double* best_val, int64_t* best_gidx, double* best_x);
int bogp_exchange_topk(bogp_handle* h, int64_t index_offset, double* best_val, int64_t* best_gidx, double* best_x);
int bogp_reduce_pairs(int R, int q, int d, const double* gathered, double* val, int64_t* gidx, double* x);
int bogp_merge_topk(int R, int q, int k, int d, const double* gathered, double* val, int64_t* gidx, double* x);

/* ---- measurement ----------------------------------------------------------------------------------
 * HIP-event durations (ms, summed over candidate chunks) of the kernels of the LAST bogp_predict /
 * bogp_sweep call, recorded on the library's own stream: corr (k_corr_chunk, the K* producer), contract
 * (k_contract, the dominant L^-1 MFMA contraction) and acquisition/argmax.  n_chunks = launches of each.
 * Which intervals each field sums on each sweep path (one launch, chunks, pruned chunks, one pass, forest):
 * the table above collect_timing in csrc/bogp_api_sweep.hip.  */
int bogp_last_timing(bogp_handle* h, double* corr_ms, double* contract_ms, double* acquisition_ms, int* n_chunks);

/* ---- pruned sweep -----------------------------------------------------------------------------------
 * A bogp_sweep without acq_out returns only its q winners, so a candidate whose criteria cannot reach the best values found so
 * far even with the most optimistic variance (|L^-1 r|^2 = 0) skips the N^2 contraction (constant basis, chunked path; DESIGN.md
 * section 5.22).  Winners and their values are those of the full sweep, bit for bit.  on = 0 switches the pruning off for this
 * handle: every row is then contracted, as for bogp_predict / bogp_sweep_topk / acq_out, which never prune.  on = 1 (the default)
 * is automatic: a sweep of more than one chunk over fully resident candidates (not a lazy upload), with a squared-distance kernel,
 * bounds all rows behind the pilot in ONE pass -- a producer launch that stores no correlations -- and produces correlation columns
 * for the survivors alone; it waits on the host twice (the pilot's estimate, the survivor count of a segment), also where the sweep
 * itself is queued.  Where that does not apply, or the pilot's own rows show that little can be pruned, it is the per-chunk path,
 * which on = 2 forces.                                                                                                          */
int bogp_set_prune(bogp_handle* h, int on);

/* Which way the LAST sweep pruned: path = BOGP_PRUNE_PATH_*; for the one-pass paths, survivors = the rows behind the pilot that the
 * bound let through and that were contracted in `rounds` rounds of at most one chunk's rows (0 and 0 otherwise).  Any output may
 * be NULL.                                                                                                                      */
#define BOGP_PRUNE_PATH_NONE 0             /* nothing was pruned (option off, value outputs, one launch, ...)      */
#define BOGP_PRUNE_PATH_CHUNKS 1           /* bound, compaction and gather chunk by chunk                          */
#define BOGP_PRUNE_PATH_ONEPASS 2          /* one bounding pass per segment, exact producer for survivors only     */
#define BOGP_PRUNE_PATH_ONEPASS_FALLBACK 3 /* ... of which a segment with too many survivors ran chunk by chunk    */
int bogp_last_prune_path(bogp_handle* h, int* path, int64_t* survivors, int* rounds);

/* The two host decisions of the one-pass flow, no device and no handle (tests/test_prune_decide_host.py): BOGP_PRUNE_PATH_CHUNKS if
 * more than an eighth of the pilot's rows survive the pilot's own thresholds, else BOGP_PRUNE_PATH_ONEPASS_FALLBACK if more than a
 * quarter of the segment's rows survive, else BOGP_PRUNE_PATH_ONEPASS.                                                           */
int bogp_prune_decide(int64_t pilot_rows, int64_t pilot_survivors, int64_t segment_rows, int64_t segment_survivors);

/* Candidates per chunk of a candidate pass, no device and no handle (tests/test_sweep_geometry_host.py): what chunk_bytes (the
 * BOGP_CHUNK_MB switch, 1 GiB by default) hold of columns of `rows` doubles -- the padded training rows -- in whole 64-row tiles, at
 * least 64 and at most M rounded up to 64.  Negative where that exceeds what the kernels' 32-bit row offsets reach (76 695 808): the
 * sweeps then fail with BOGP_ERR_UNSUPPORTED.  rows, M, chunk_bytes > 0.                                                          */
int64_t bogp_sweep_chunk_rows(int64_t rows, int64_t M, int64_t chunk_bytes);

/* Rows that went through the contraction in the LAST bogp_predict / bogp_sweep call (M without pruning; waits for a queued sweep). */
int bogp_last_contracted_rows(bogp_handle* h, int64_t* rows);

/* Candidate tile of the direct variance contraction (DESIGN.md section 5.2'''): a workgroup contracts 64, 32 or 16 candidates with
 * 256 columns of L^-1.  rows = 0 (the default) chooses per launch -- 64 while the 64-row grid fills the device, narrower tiles for
 * launches of few rows --, 16 / 32 / 64 force one tile for this handle (tests and A/B); anything else is BOGP_ERR_INVALID.  No output
 * bit depends on the tile.  The gated launches of the per-chunk pruned path always take 64 rows, and so does every launch under
 * BOGP_CONTRACT_DIRECT=0.  bogp_last_contract_tile: the tile rows of the last contraction launch of this handle (64 before any).   */
int bogp_set_contract_tile(bogp_handle* h, int rows);
int bogp_last_contract_tile(bogp_handle* h, int* rows);

/* The automatic choice, no device and no handle (tests/test_contract_tile_host.py): tile rows for a launch of row_tiles64 64-row
 * tiles x nJ column groups on a device of n_cu compute units; live != 0: a gated launch.                                         */
int bogp_contract_tile_rows(int64_t row_tiles64, int nJ, int n_cu, int live);

/* Host evaluations of the pruned sweep's two rules, no device and no handle (tests/test_prune_bounds_host.py): an upper bound of
 * criterion acq_id over every standard deviation in [0, sd_ub] at the mean behind y_hat (guard branches included; NaN or +inf
 * where no bound exists), and whether a row with that bound is pruned against a value another row attained:
 * bound + 1e-9 (|bound| + |threshold|) + 1e-300 < threshold, threshold finite.                                                  */
double bogp_acq_upper_bound(int acq_id, double acq_par, double y_hat, double sd_ub, double plugin, double sigma2);
int bogp_prune_below(double bound, double threshold);

/* FP32 bounding stage of the one-pass pruned sweep.  For the squared-exponential, Matern-3/2 and Matern-5/2
 * kernels up to 128 dimensions, the bounding pass of a segment first runs in FP32 with a proven error margin per row; only the rows
 * it cannot rule out get the exact FP64 sums and the exact bound, which decides as before: survivors, rounds, paths and every output
 * bit are unchanged.  A segment of which the FP32 stage keeps more than a quarter runs the exact pass over all its rows instead.
 * on = 1 (the default) / 0 for this handle.                                                                                         */
int bogp_set_prune_bound32(bogp_handle* h, int on);

/* What the FP32 stage did in the LAST sweep: rows it bounded, rows it kept (summed over the segments), segments that ran the exact
 * pass over all rows after all.  All zero where the stage did not run.  Any output may be NULL.                                     */
int bogp_last_bound32(bogp_handle* h, int64_t* rows, int64_t* kept, int* fallbacks);

/* Debug read-back of the last segment the FP32 stage bounded (waits for a queued sweep): *rows = its rows (0: none); per row the FP32
 * sums r . gamma and w . r, their margins and the stage's flag.  Arrays of `cap` >= *rows entries, any of them NULL.                 */
int bogp_debug_bound32(bogp_handle* h, int64_t cap, double* mu32, double* e_mu, double* wd32, double* e_w, unsigned char* flags, int64_t* rows);

/* Debug count of what the handles of this process hold on the device right now: live device and mapped pinned allocations, their
 * bytes, live events.  A handle owns every buffer and event through a member that frees it (csrc/bogp_handle.h), so the counts
 * return to their earlier values after bogp_destroy (tests/test_gpu_handle_lifetime.py).  No handle; any output may be NULL.        */
void bogp_debug_live(int64_t* allocations, int64_t* bytes, int64_t* events);

/* Host evaluations of the FP32 stage's two rules, no device and no handle (tests/test_bound32_host.py): the margins of a row whose
 * scaled point has squared norm na (+inf where the stage cannot bound the row), and the largest bogp_acq_upper_bound over y_hat in
 * [y_hat - e, y_hat + e] (+inf where the interval holds a switch point of the criterion, a NaN or an infinity).                     */
int bogp_bound32_margin(int kernel, int d, double na, double nb_max, double gamma_l1, double w_l1, double* e_mu, double* e_w);
double bogp_acq_upper_bound_interval(int acq_id, double acq_par, double y_hat, double e, double sd_ub, double plugin, double sigma2);

/* Algorithmic FP64 flops per candidate of the posterior for the committed model:
 * N^2 + N (3d + 5 + 2p)  (SURVEY.md section 8d).                                                        */
double bogp_flops_per_candidate(const bogp_handle* h);

/* ---- self test -------------------------------------------------------------------------------------
 * The in-tree dense product behind the polynomial-trend, REML and small-batch paths (kernels_gemm.hip; the library links no
 * BLAS), on host buffers: C (m x n, ldc) = alpha op(A) (m x k) op(B) (k x n) + beta C, column-major; ta / tb != 0: the stored
 * matrix is the transpose; tri = 1 / 2: op(A) is square lower / upper triangular with explicit zeros in the other triangle
 * (the kernel then shortens its k range); split != 0: the deterministic split-K path may be taken (small C, long k).
 * What the reference gets from numpy.dot / scipy.linalg (gpr.py:799-808, 850-918); used by tests/test_gpu_gemm.py.        */
int bogp_selftest_gemm(bogp_handle* h, int ta, int tb, int m, int n, int k, double alpha, const double* A, int lda,
                       const double* B, int ldb, double beta, double* C, int ldc, int tri, int split);

/* The radial profile r(s2) of correlation function `kernel` (BOGP_SELFTEST_PROFILE; s2 = the weighted squared distance the producers
 * accumulate, pexp = the exponent p / the order nu where the kernel has one) or one of the special functions behind it, evaluated on the
 * device for n arguments: what the reference gets per pair from kernel.py:186-207, 289-329 (numpy sqrt / exp, scipy.special.kv and
 * scipy.special.gamma).  BESSEL_K: K_pexp(arg); RGAMMA: 1 / Gamma(arg); BESSEL_K_PAIRS: arg holds n pairs (nu, x) -> K_nu(x);
 * MATERN_NU_PAIRS: n pairs (nu, s2) -> the general-nu Matern profile at squared distance s2.
 * Used by tests/test_gpu_special.py to hold them to committed tables argument by argument.                                            */
#define BOGP_SELFTEST_PROFILE 0
#define BOGP_SELFTEST_BESSEL_K 1
#define BOGP_SELFTEST_RGAMMA 2
#define BOGP_SELFTEST_BESSEL_K_PAIRS 3
#define BOGP_SELFTEST_MATERN_NU_PAIRS 4
int bogp_selftest_profile(bogp_handle* h, int what, int kernel, double pexp, const double* arg, int64_t n, double* out);

/* The scalar criterion functions of csrc/bogp_device.h -- what every sweep ends in and what the pruned paths decide with -- evaluated
 * on the device at arguments the caller chooses: `rows` is n x 8 doubles (row-major), one thread per row writes one double to out.
 * Columns per selector (the remaining ones are ignored; ids and parameters travel as doubles):
 *   NDTR (a)   NORM_PDF (x)   EHVI_G (z)
 *   ACQ_VALUE (id, par, y_hat, sd, plugin, sigma2)             FEASIBILITY (mu, mse, sigma2, lo, hi)
 *   ACQ_UPPER_BOUND (id, par, y_hat, sd_ub, plugin, sigma2)    ACQ_UPPER_BOUND_INTERVAL (id, par, y32, e, sd_ub, plugin, sigma2)
 *   PRUNE_BELOW (bound, thr) -> 0.0 / 1.0
 * The kernel calls the functions themselves and holds no copy of any expression.  Used by tests/test_gpu_criteria.py to hold them to
 * the committed table tests/golden/G46_criteria_truth.npz argument by argument.                                                      */
#define BOGP_CRITERIA_NDTR 0
#define BOGP_CRITERIA_NORM_PDF 1
#define BOGP_CRITERIA_EHVI_G 2
#define BOGP_CRITERIA_ACQ_VALUE 3
#define BOGP_CRITERIA_FEASIBILITY 4
#define BOGP_CRITERIA_ACQ_UPPER_BOUND 5
#define BOGP_CRITERIA_ACQ_UPPER_BOUND_INTERVAL 6
#define BOGP_CRITERIA_PRUNE_BELOW 7
#define BOGP_CRITERIA_COLUMNS 8
int bogp_selftest_criteria(bogp_handle* h, int what, const double* rows, int64_t n, double* out);
/* feasibility_grad of csrc/bogp_device.h itself on the device: rows n x 5 (mu, mse, sigma2, lo, hi), out n x 3 (F, dF/dmu, dF/dsd),
 * both HOST arrays; out[:, 0] has the bits of bogp_selftest_criteria(BOGP_CRITERIA_FEASIBILITY).  Used by
 * tests/test_gpu_constrained_grad.py against tests/golden/G47_feasibility_grad_truth.npz.  BOGP_ERR_INVALID: null pointer or n <= 0. */
int bogp_selftest_feasibility_grad(bogp_handle* h, const double* rows, int64_t n, double* out);

/* The optimiser behind bogp_mle_batch (csrc/bogp_lbfgsb.h: L-BFGS-B after Byrd, Lu, Nocedal & Zhu 1995 with the More'-Thuente
 * line search) on a HOST objective: what the reference gets from scipy.optimize.fmin_l_bfgs_b (gpr.py:1136).  No device, no handle;
 * used by tests/test_lbfgsb.py to compare it with scipy on the CPU.  x: in the start, out the minimiser (n); fn fills *f and g (n).
 * m / maxfun / maxiter <= 0: 10 / 15000 / 15000.  status as in bogp_mle_batch.                                                  */
typedef void (*bogp_objective_fn)(const double* x, int n, double* f, double* g, void* user);
int bogp_lbfgsb_minimize(int n, int m, double* x, const double* lo, const double* hi, double factr, double pgtol, int maxfun,
                         int maxiter, bogp_objective_fn fn, void* user, double* f, int* nfev, int* nit, int* status);

/* Which device path a concentrated-likelihood evaluation (bogp_nll) of N points in d dimensions would take with the constant
 * basis (trend) and n_targets columns of y -- no handle, no device call (the decision is made from sizes and the environment
 * switches alone; gpr.py:920-1040 is the function all three evaluate):
 *   BOGP_NLL_PATH_GENERAL   the multi-kernel path (blocked Cholesky, recursive-doubling inverse, U U^T, ...)
 *   BOGP_NLL_PATH_ONE_LAUNCH  the whole evaluation in one launch of one workgroup (k_nll_small; N <= 156 if it fits one CU's LDS)
 *   BOGP_NLL_PATH_ELIM      one launch per 64 columns (k_elim_step; up to N = 3072)
 * DESIGN.md section 5.12; used by tests/test_abi.py.                                                                         */
#define BOGP_NLL_PATH_GENERAL 0
#define BOGP_NLL_PATH_ONE_LAUNCH 1
#define BOGP_NLL_PATH_ELIM 2
int bogp_nll_path(int N, int d, int trend, int n_targets);

/* The schedule of WIDE FIRST PANELS the blocked Cholesky of the general path (gpr.py:795, `cholesky(R, lower=True)`) takes for N training
 * points -- no handle, no device call.  Returns the number of wide panels (0 below N = 6017 and with BOGP_BIG_CHOL=0) and writes up to `cap`
 * widths (64-column blocks per panel) to `widths` (may be NULL).  Inside a wide panel the rank-64 updates touch the panel's own columns
 * only and ONE rank-64w product on 128 x 128 tiles updates the rest of the trailing matrix; every schedule yields the SAME BITS as the
 * one-level chain (the products run over k in the same order from the same starting value).  DESIGN.md section 5.9; tests/test_abi.py,
 * tests/test_gpu_driver.py.                                                                                                         */
int bogp_chol_wide_panels(int N, int* widths, int cap);

#ifdef __cplusplus
}
#endif
#endif /* BOGP_H */
