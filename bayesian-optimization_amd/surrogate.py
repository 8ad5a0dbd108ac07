"""GPU GaussianProcess: drop-in for `bayes_optim.surrogate.GaussianProcess` on one MI355X.

Satisfies the surrogate protocol of SURVEY.md section 8b (who calls what: `base.py:423-446` fit/predict,
`acquisition_fun.py:52-80` predict/gradient, attributes `sigma2`, `y`, `is_fitted`) with the same constructor
keywords as the reference (`surrogate/gaussian_process/gpr.py:211-228`).  All O(N^2)+ arithmetic runs in libbogp
(HIP kernels); the host keeps only what the reference keeps on the host: the L-BFGS-B restart loop of
the MLE (`gpr.py:1058-1197`) and input validation.  There is no CPU fallback.

Differences from the reference, all deliberate and listed in DESIGN.md:
  * `optimizer="CMA"`: NotImplementedError (out of scope) instead of running on the CPU.  Multi-target y is served for a
    fixed constant trend (the only case the reference's own `fit` survives).  The three polynomial trends
    (constant / linear / quadratic) are all on the device.
  * `likelihood="restricted"` (REML, gpr.py:813-918) is evaluated on the device AND `fit` completes with it; the
    reference's own `fit` raises TypeError at gpr.py:405 after the optimisation (sigma2 comes back as a scalar).
  * Matern-5/2 (`corr=functools.partial(matern, nu=2.5)` or `"matern52"`) can be FITTED: the device has its
    theta- and x-derivatives, which the reference leaves as `pass` (gpr.py:647-648, 758-759).
  * `predict(batch_size=...)` works (the reference's branch is dead code on Python 3, gpr.py:513-535); chunking
    is done inside the library anyway.
"""
from __future__ import annotations

import os
import warnings

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

from . import _lib, distributed
from .prior_mean import constant_trend, device_trend_of

_KERNEL_IDS = {
    "squared_exponential": _lib.KERNEL_SE,
    "matern": _lib.KERNEL_MATERN32,  # the reference passes only (theta, d): nu defaults to 1.5 (kernel.py:159)
    "matern12": _lib.KERNEL_MATERN12,
    "matern32": _lib.KERNEL_MATERN32,
    "matern52": _lib.KERNEL_MATERN52,
    "absolute_exponential": _lib.KERNEL_ABSEXP,
    # values only (set_state / predict / sweep): `fit` needs d llf / d theta, which the reference defines for neither
    "cubic": _lib.KERNEL_CUBIC,
    "generalized_exponential": _lib.KERNEL_GENEXP,  # theta = [theta_1 .. theta_d, p]: thetaL / thetaU of length d + 1
}
# "linear" / "pure_nugget" are not in the reference's correlation table at all (gpr.py:198-207)
_UNBUILT_KERNELS = ("linear",)
_NU_IDS = {0.5: _lib.KERNEL_MATERN12, 1.5: _lib.KERNEL_MATERN32, 2.5: _lib.KERNEL_MATERN52}


_ENV_WARNED = set()


def _warn_env_once(name, what):
    """An environment variable switched a non-default fit schedule on from OUTSIDE the code: say so once per process."""
    if name not in _ENV_WARNED:
        _ENV_WARNED.add(name)
        warnings.warn("bogp: %s is set -- %s" % (name, what), stacklevel=3)


def kernel_id_of(corr) -> int:
    """Map the reference's `corr` argument (a name, or a callable such as functools.partial(matern, nu=2.5))."""
    if isinstance(corr, str):
        if corr in _KERNEL_IDS:
            return _KERNEL_IDS[corr]
        if corr in _UNBUILT_KERNELS:
            raise NotImplementedError("correlation %r is not built on the device yet (SURVEY.md 8 f4)" % corr)
        raise ValueError("corr should be one of %s or callable, %s was given." % (list(_KERNEL_IDS), corr))
    func = getattr(corr, "func", corr)
    name = getattr(func, "__name__", "")
    if name == "squared_exponential":
        return _lib.KERNEL_SE
    if name == "absolute_exponential":
        return _lib.KERNEL_ABSEXP
    if name == "cubic":
        return _lib.KERNEL_CUBIC
    if name == "generalized_exponential":
        return _lib.KERNEL_GENEXP
    if name == "matern":
        nu = (getattr(corr, "keywords", None) or {}).get("nu", 1.5)
        if nu in _NU_IDS:
            return _NU_IDS[nu]
        if not (isinstance(nu, (int, float)) and 0.0 < float(nu) <= 60.0):
            raise NotImplementedError("general-nu Matern: nu = %r outside (0, 60]" % (nu,))
        return _lib.KERNEL_MATERN_NU  # kernel.py:201-207 (scipy.special.kv there, a device K_nu here); values only, like the reference
    raise NotImplementedError("callable correlation %r is not built on the device" % (corr,))


class GaussianProcess:
    """The Gaussian Process model class (GPU engine).  Constructor keywords as gpr.py:211-228, plus `device`."""

    _optimizer_types = ["BFGS", "CMA"]
    _likelihood_functions = ["concentrated", "restricted"]

    def __init__(
        self,
        mean=None,
        corr="squared_exponential",
        theta0=None,
        thetaL=None,
        thetaU=None,
        sigma2=None,
        nugget=1e-6,
        noise_estim=False,
        optimizer="BFGS",
        likelihood="concentrated",
        random_start=1,
        wait_iter=5,
        eval_budget=None,
        random_state=None,
        verbose=False,
        device=0,
        distribute_restarts=False,
        restart_streams=None,
        restart_batch=None,
        restart_lookahead=None,
        mle_chain_rule=False,
        mle_prune_reserve=0,
    ):
        self.mean = mean
        self.corr = corr
        self.sigma2 = sigma2
        self.verbose = bool(verbose)
        self.corr_type = corr
        self.kernel_id = kernel_id_of(corr)
        # general-nu Matern: the order is a keyword of the correlation function in the reference (functools.partial(matern, nu=...)),
        # an extra trailing entry of theta at the C ABI (like generalized_exponential's exponent): `_epar` puts it there
        self._nu = float((getattr(corr, "keywords", None) or {}).get("nu", 1.5)) if self.kernel_id == _lib.KERNEL_MATERN_NU else None
        self.is_fitted = False
        self.device = int(device)
        self.distribute_restarts = bool(distribute_restarts)
        # MLE restarts on `restart_streams` engines (= HIP streams) of the SAME GPU at once (opt-in; None: BOGP_RESTART_STREAMS or 1)
        self.restart_streams = int(restart_streams if restart_streams is not None else os.environ.get("BOGP_RESTART_STREAMS", "1"))
        if restart_streams is None and self.restart_streams > 1:
            _warn_env_once("BOGP_RESTART_STREAMS", "the MLE restarts run on %d streams: ALL start points are drawn up front from the global np.random "
                           "stream (the sequential loop draws lazily and stops early), so later draws differ from the reference's trajectory" % self.restart_streams)
        # MLE restarts advanced TOGETHER on the device, `restart_batch` at a time (opt-in; None: BOGP_RESTART_BATCH or 0 = the
        # reference's sequential scipy loop): bogp_mle_batch, one batched likelihood call per round of all active restarts
        self.restart_batch = int(restart_batch if restart_batch is not None else os.environ.get("BOGP_RESTART_BATCH", "0"))
        if restart_batch is None and self.restart_batch > 0:
            _warn_env_once("BOGP_RESTART_BATCH", "the MLE restarts run in lock step, %d at a time, on libbogp's own L-BFGS-B (not scipy's): every restart of a wave "
                           "starts and its start point is drawn, so the fit and the np.random stream differ from the reference's sequential loop" % self.restart_batch)
        # extension, with restart_batch only: hand the optimiser the gradient of the function it minimises (d / d log10 par) instead of
        # the reference's d / d par (which stays the default)
        self.mle_chain_rule = bool(mle_chain_rule)
        # restart_batch only: as the shared evaluation budget runs out (fewer than this many evaluations per active restart left) the worst
        # restart is stopped, so that the budget ends on the leading ones (0: equal shares to the end)
        self.mle_prune_reserve = int(mle_prune_reserve)
        # r05: the reference's SEQUENTIAL restart loop with look-ahead -- restart i + 1 (.. i + L) is run speculatively on a second (..) engine
        # while restart i runs; results, evaluation count and the np.random stream are the sequential loop's, bit for bit
        # (`_restarts_with_lookahead`).  None: BOGP_RESTART_LOOKAHEAD, or by size (two restarts ahead from N = 1500, where the device time of an
        # evaluation dwarfs the interpreter's share, one below); 0: off.
        self.restart_lookahead = int(restart_lookahead if restart_lookahead is not None else os.environ.get("BOGP_RESTART_LOOKAHEAD", "-1"))  # -1: by size
        self._worker_engines = []

        self.theta0 = np.array(theta0, dtype=float).flatten() if theta0 is not None else None
        if thetaL is None or thetaU is None:
            # np.array(None) makes np.isfinite raise TypeError in the reference (gpr.py:238-242): bounds are mandatory
            raise TypeError("thetaL and thetaU are required (finite bounds of the MLE search box)")
        self.thetaL = np.array(thetaL, dtype=float).flatten()
        self.thetaU = np.array(thetaU, dtype=float).flatten()
        if not (np.isfinite(self.thetaL).all() and np.isfinite(self.thetaU).all()):
            raise ValueError("all bounds are required finite.")

        self.optimizer = optimizer
        self.random_start = int(random_start)
        self.random_state = random_state
        self.wait_iter = wait_iter
        self.eval_budget = eval_budget

        self.nugget = nugget
        self.noise_var = np.atleast_1d(nugget) if nugget else 0
        self.noise_estim = noise_estim
        self.noisy = bool(self.noise_var) or bool(self.noise_estim)
        if not self.noisy:
            self.estimation_mode = "noiseless"
        elif self.noise_estim:
            self.estimation_mode = "noise_estim"
        else:
            self.estimation_mode = "noisy"

        assert likelihood in self._likelihood_functions
        self.likelihood = likelihood
        if self.mean is None:
            self.mean = constant_trend(len(self.thetaU), beta=0)  # simple Kriging (gpr.py:269-270)
        self.mean_type = "basis_expansion"
        self.estimate_trend = self.mean.beta is None
        self._engine = None
        self._committed_par = None
        self._check_params()

    # ------------------------------------------------------------------------------------------------
    # engine plumbing (the object stays picklable: base.py:499-540 dills the whole optimiser)
    # ------------------------------------------------------------------------------------------------
    _MODE = {"noiseless": _lib.MODE_NOISELESS, "noisy": _lib.MODE_NOISY, "noise_estim": _lib.MODE_NOISE_ESTIM}

    @property
    def engine(self) -> "_lib.Engine":
        if self._engine is None:
            self._engine = _lib.Engine(self.device)
            if hasattr(self, "X"):
                self._engine.set_train(self.X, self.y)
                if self._committed_par is not None:
                    self._commit(self._committed_par, refresh_attributes=False, restricted=getattr(self, "_committed_restricted", False))
        return self._engine

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_engine"] = None  # device handles never travel; re-created lazily from (X, y, par)
        st["_worker_engines"] = []
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)

    def _trend_args(self):
        tid, _, beta = device_trend_of(self.mean)  # raises for bases the device does not evaluate
        # the estimation mode is fixed at construction (gpr.py:273-275); fit() later fills mean.beta with the GLS value
        return tid, self.estimate_trend, (0.0 if self.estimate_trend else beta)

    @staticmethod
    def _trend_views(st, est):
        """Ft, G, Q, beta of an engine state in the reference's shapes: (N, p), (p, p), (N, p), (p, 1)."""
        if not est:
            return None, None, None, np.atleast_1d(st["beta"]).reshape(-1, 1)
        if np.ndim(st["G"]) == 0:  # constant basis: the C ABI hands back vectors and a scalar
            return st["Ft"].reshape(-1, 1), np.array([[st["G"]]]), st["Q"].reshape(-1, 1), np.array([[st["beta"]]])
        return st["Ft"], st["G"], st["Q"], np.asarray(st["beta"], dtype=float).reshape(-1, 1)

    def _epar(self, par):
        """The parameter vector as the engine takes it: nu inserted behind the theta entries for the general-nu Matern kernel."""
        if self.kernel_id != _lib.KERNEL_MATERN_NU:
            return par
        par = np.asarray(par, dtype=np.float64).ravel()
        n_theta = len(self.thetaL)
        return np.r_[par[:n_theta], self._nu, par[n_theta:]]

    def _nv(self) -> float:
        return float(np.atleast_1d(self.noise_var)[0]) if self.estimation_mode == "noisy" else 0.0

    # ------------------------------------------------------------------------------------------------
    def _check_params(self):
        """gpr.py:1199-1248 (the parts that apply)."""
        if self.thetaL.size != self.thetaU.size:
            raise ValueError("thetaL and thetaU must have the same length.")
        if self.theta0 is not None and self.theta0.size != self.thetaL.size:
            raise ValueError("theta0, thetaL, and thetaU must have the same length.")
        if np.any(self.thetaL <= 0) or np.any(self.thetaU < self.thetaL):
            raise ValueError("The bounds must satisfy O < thetaL <= thetaU.")
        if self.optimizer not in self._optimizer_types:
            raise ValueError("optimizer should be one of %s" % self._optimizer_types)
        if self.optimizer == "CMA":
            raise NotImplementedError("optimizer='CMA' is out of scope (SURVEY.md 2 row 8); use 'BFGS'")

    def _check_data(self, X, y):
        """gpr.py:279-310 without the pair-distance list (never built on the device)."""
        X = np.asarray(X, dtype=np.float64)  # also coerces a `Solution` (object dtype), like check_X_y
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
        if y.ndim == 1:
            y = y.reshape(-1, 1)
        if X.shape[0] == 0:
            raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
        if X.shape[0] != y.shape[0]:
            raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (X.shape[0], y.shape[0]))
        if not (np.isfinite(X).all() and np.isfinite(y).all()):
            raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
        if y.shape[1] > 1 and (self.estimate_trend or type(self.mean).__name__ != "constant_trend" or self.likelihood == "restricted"):  # (REML: single target)
            # the reference gets through the MLE and then raises "Shapes of beta and F do not match." (gpr.py:787 assigns
            # a (p, n_targets) beta); only a fixed constant trend works there with several targets
            raise NotImplementedError("multi-target y needs a fixed constant trend (constant_trend(dim, beta=...)) and the concentrated likelihood")
        if y.shape[1] > _lib.MAX_TARGETS:
            raise NotImplementedError("at most %d targets" % _lib.MAX_TARGETS)
        if self.kernel_id == _lib.KERNEL_GENEXP:  # theta carries the exponent p as its last entry (kernel.py:369-373)
            if self.thetaL.size not in (2, X.shape[1] + 1):
                raise Exception("Length of theta must be 2 or %s" % (X.shape[1] + 1))
            if getattr(self.mean, "n_feature", X.shape[1]) != X.shape[1]:
                # the default trend is built from len(thetaU) = d + 1 (gpr.py:269-270): the reference then rejects X at trend.py:57
                raise Exception("X does not have the right size!")
        elif self.thetaL.size not in (1, X.shape[1]):
            raise ValueError("Length of theta must be 1 or %s" % X.shape[1])
        if self.estimate_trend:
            p = _lib.trend_size_of(self._trend_args()[0], X.shape[1])
            if p > X.shape[0]:  # gpr.py:299-308
                raise Exception("Ordinary least squares problem is undetermined n_samples=%d must be greater than the "
                                "meanession model size p=%d." % (X.shape[0], p))  # fmt: skip
        self.X, self.y = np.ascontiguousarray(X), np.ascontiguousarray(y)
        self._committed_par = None
        self.engine.set_train(self.X, self.y)

    # ------------------------------------------------------------------------------------------------
    # likelihood (gpr.py:920-1040) -- evaluated on the device
    # ------------------------------------------------------------------------------------------------
    def _restore(self, prev):
        """Put the device back into the committed state `prev` = (par, restricted) -- or mark the model as holding none."""
        if prev[0] is None:
            self._committed_par = None
        else:
            self._commit(prev[0], refresh_attributes=False, restricted=prev[1])

    def log_likelihood_concentrated(self, par, env=None, eval_grad=False, _adopt=False):
        """gpr.py:920-1040.  As in the reference, evaluating the likelihood has no side effect on the fitted model: the
        committed state is re-established afterwards, also when `env` is filled or the factorisation fails.  Only the
        MLE's final evaluation (`_adopt=True`, gpr.py:1183-1188) keeps the state it built."""
        par = np.asarray(par, dtype=np.float64).ravel()
        tid, est, beta = self._trend_args()
        mode = self._MODE[self.estimation_mode]
        if not (np.all(np.isfinite(par)) and np.all(par > 0)):
            # L-BFGS-B can step to NaN after an infinite objective; the reference's Cholesky then raises
            # ValueError/LinAlgError on the NaN matrix, which it turns into -inf (gpr.py:946-947, 960-961, 978-979)
            return (-np.inf, np.zeros((len(par), 1))) if eval_grad else -np.inf
        prev = (self._committed_par, getattr(self, "_committed_restricted", False))
        after = prev
        try:
            if env is not None:
                llf = self._commit(par, refresh_attributes=False, restricted=False)
                if llf > 0:  # rejected before env is touched (gpr.py:981-982); bogp_commit itself only builds the state
                    self._restore(prev)
                    return (-np.inf, np.zeros((len(par), 1))) if eval_grad else -np.inf
                st = self.engine.get_state()
                Ft, G, Q, b = self._trend_views(st, est)
                env.update(
                    sigma2=np.atleast_1d(st["sigma2"]), noise_var=st["noise_var"], rho=st["rho"].reshape(len(self.X), -1),
                    Yt=st["Yt"].reshape(len(self.X), -1), C=st["C"], Ft=Ft, G=G, Q=Q,
                    beta=float(b[0, 0]) if b.size == 1 else b, gamma=st["gamma"].reshape(len(self.X), -1),
                )  # fmt: skip
                if _adopt:
                    after = (np.array(par, dtype=float), False)
                if not eval_grad:
                    if not _adopt:
                        self._restore(prev)
                    return llf
            out = self.engine.nll(self.kernel_id, mode, self._epar(par), self._nv(), est, beta, eval_grad=eval_grad, trend=tid)
            # nll overwrote the factor buffers: re-establish the state that is to survive this call
            self._restore(after)
            return out
        except _lib.NotPositiveDefinite:
            # Cholesky failure or llf > 0: the reference's -inf convention (gpr.py:946-947, 981-982)
            self._restore(prev)
            return (-np.inf, np.zeros((len(par), 1))) if eval_grad else -np.inf

    def _split_restricted(self, par):
        """(theta, sigma2, noise_var) of a REML parameter vector (gpr.py:826-834)."""
        par = np.asarray(par, dtype=np.float64).ravel()
        if self.estimation_mode == "noise_estim":
            return par[:-2], float(par[-2]), float(par[-1])
        return par[:-1], float(par[-1]), (self._nv() if self.estimation_mode == "noisy" else 0.0)

    def log_likelihood_restricted(self, par, env=None, eval_grad=False, _adopt=False):
        """The restricted likelihood of gpr.py:813-918 on the device (same return convention as the concentrated one:
        llf or (llf, d llf / d par), -inf where the reference gives -inf).  `env` receives what the reference puts
        there (:902-911) -- the NOISY-mode factorisation at (theta, sigma2, noise_var), which is also the state `fit`
        commits for prediction (`_adopt=True`: the MLE's final evaluation keeps it; any other call leaves the fitted
        model as it was)."""
        par = np.asarray(par, dtype=np.float64).ravel()
        tid, est, beta = self._trend_args()
        if self.y.shape[1] > 1:
            # several targets: the reference's arithmetic yields a VALUE (the scalar terms broadcast over the n_t x n_t matrix rho^T rho,
            # everything summed, gpr.py:861-866) and raises in the gradient (a (1, N n_t) by (N, N) product, :875, :896); `env` would
            # receive one column per target there -- not built, nothing in the reference reads it
            if eval_grad:
                raise ValueError("shapes (1,%d) and (%d,%d) not aligned: the restricted likelihood has no gradient with several targets "
                                 "(gpr.py:875, 896)" % (self.y.size, len(self.y), len(self.y)))
            if env is not None:
                raise NotImplementedError("env of the restricted likelihood with several targets")
        if not (np.all(np.isfinite(par)) and np.all(par > 0)):
            return (-np.inf, np.zeros((len(par), 1))) if eval_grad else -np.inf
        prev = (self._committed_par, getattr(self, "_committed_restricted", False))
        after = prev
        try:
            if env is not None:
                self._commit(par, refresh_attributes=False, restricted=True)
                st = self.engine.get_state()
                Ft, G, Q, b = self._trend_views(st, est)
                env.update(sigma2=np.atleast_1d(st["sigma2"]), noise_var=st["noise_var"], rho=st["rho"].reshape(-1, 1),
                           Yt=st["Yt"].reshape(-1, 1), C=st["C"], Ft=Ft, G=G, Q=Q, gamma=st["gamma"].reshape(-1, 1))  # fmt: skip
                if _adopt:
                    after = (np.array(par, dtype=float), True)
            out = self.engine.nll_restricted(self.kernel_id, self._MODE[self.estimation_mode], self._epar(par), self._nv(), est, beta, eval_grad=eval_grad, trend=tid)
            self._restore(after)
            return out
        except _lib.NotPositiveDefinite:
            self._restore(prev)
            return (-np.inf, np.zeros((len(par), 1))) if eval_grad else -np.inf

    def _commit(self, par, refresh_attributes=True, restricted=None) -> float:
        tid, est, beta = self._trend_args()
        restricted = (self.likelihood == "restricted") if restricted is None else restricted
        self._committed_restricted = restricted  # how `_committed_par` is to be read when the state is rebuilt
        if restricted:  # R = (sigma2 R0 + nv I) / (sigma2 + nv): the NOISY-mode state (gpr.py:836-839)
            theta, s2, nv = self._split_restricted(par)
            llf = self.engine.commit(self.kernel_id, _lib.MODE_NOISY, self._epar(np.r_[theta, s2]), nv, est, beta, trend=tid)
            self._committed_par = np.array(par, dtype=float)
            if refresh_attributes:
                self._pull_state(par)
            return llf
        llf = self.engine.commit(self.kernel_id, self._MODE[self.estimation_mode], self._epar(par), self._nv(), est, beta, trend=tid)
        self._committed_par = np.array(par, dtype=float)
        if refresh_attributes:
            self._pull_state(par)
        return llf

    def _pull_state(self, par):
        """The tail of fit(): gpr.py:402-415 + compute_beta_gamma (:784-788)."""
        st = self.engine.get_state()
        n_theta = len(self.thetaL)
        self.theta_ = np.array(par[:n_theta], dtype=float)
        self.noise_var = st["noise_var"]
        self.sigma2 = np.atleast_1d(st["sigma2"]).astype(float)
        self.rho = st["rho"].reshape(len(self.X), -1)
        self.Yt = st["Yt"].reshape(len(self.X), -1)
        self.C = st["C"]
        self.gamma = st["gamma"].reshape(len(self.X), -1)
        if self.estimate_trend:
            self.Ft, self.G, self.Q, b = self._trend_views(st, True)
            self.mean.beta = float(b[0, 0]) if b.size == 1 else b.ravel()

    # ------------------------------------------------------------------------------------------------
    # MLE (gpr.py:1042-1197): the host loop is the reference's; every objective evaluation is a device call
    # ------------------------------------------------------------------------------------------------
    def _hyperparameter_bound(self, par_list):
        bounds = []
        for name in par_list:
            if name == "theta":
                bounds.append(np.c_[self.thetaL, self.thetaU])
            elif name == "sigma2":
                bounds.append(np.atleast_2d([1e-5, max(1e-3, self.y.std() ** 2)]))
            elif name in ("alpha", "noise_var"):  # noise_var: the reference's "TODO" bound (gpr.py:1052-1054)
                bounds.append(np.atleast_2d([1e-10, 1.0 - 1e-10]))
        return np.concatenate(bounds, axis=0)

    def _optimize_hyperparameter(self):
        restricted = self.likelihood == "restricted"
        llf_fun = self.log_likelihood_restricted if restricted else self.log_likelihood_concentrated
        par_list, par_len = ["theta"], [len(self.thetaL)]
        if restricted or self.estimation_mode == "noisy":  # gpr.py:1075-1078
            par_list.append("sigma2")
            par_len.append(1)
        if self.estimation_mode == "noise_estim":  # :1080-1086
            par_list.append("noise_var" if restricted else "alpha")
            par_len.append(1)
        bounds = self._hyperparameter_bound(par_list)
        log10bounds = np.log10(bounds)
        n_theta = len(self.thetaL)
        # warm start from the previous optimum when refitting (:1095-1107); draws use the GLOBAL np.random, as there
        if hasattr(self, "theta_"):
            log10theta0 = np.log10(self.theta_)
        else:
            log10theta0 = (
                np.log10(self.theta0)
                if self.theta0 is not None
                else np.random.uniform(np.log10(self.thetaL), np.log10(self.thetaU))
            )
        if self.estimation_mode == "noiseless" and not restricted:  # :1104-1107
            log10param = log10theta0
        else:
            log10param = np.r_[log10theta0, np.random.uniform(log10bounds[n_theta:, 0], log10bounds[n_theta:, 1])]
        n_par = len(log10param)
        eval_budget = 200 * n_par if self.eval_budget is None else self.eval_budget
        llf_opt = np.inf
        self.eval_count = 0

        def obj_func(log10param):
            # NB: the gradient handed to L-BFGS-B is d llf / d param, NOT d / d log10 param (SURVEY.md 8a quirk,
            # gpr.py:1113-1123); reproduced so that the optimiser walks the reference's trajectory
            self.eval_count += 1
            param = 10.0 ** np.array(log10param)
            llf, grad = llf_fun(param, eval_grad=True)
            return -1.0 * llf, -1.0 * np.asarray(grad, dtype=float).ravel()

        # Restarts: sequential with a shared budget and stagnation counter, as the reference (gpr.py:1127-1162).
        # With `distribute_restarts=True` under an initialised torch.distributed group, restart i runs
        # on rank i % R with budget / R evaluations; every rank still draws ALL starting points from the (identically
        # seeded) global np.random stream, so the union of starts is the sequential run's; ONE all-gather of
        # (-llf, parameters) then picks the winner on every rank.
        rank, world = (0, 1)
        dist = distributed._dist() if self.distribute_restarts else None
        if dist is not None:
            rank, world = dist.get_rank(), dist.get_world_size()
            eval_budget = max(1, -(-eval_budget // world))
        batch = int(getattr(self, "restart_batch", 0) or 0)
        if batch > 0:
            # (with `distribute_restarts` every rank runs ITS restarts -- i % world == rank, all start points drawn on every rank from the
            # identically seeded global stream -- in lock-step waves on its own GPU with budget / world, then ONE all-gather picks the winner)
            param_opt, llf_opt = self._restarts_in_lock_step(batch, log10param, log10bounds, eval_budget, restricted, rank, world)
            if world > 1:
                param_opt, llf_opt = distributed.exchange_best_parameters(np.asarray(param_opt, float), float(llf_opt))
            optimal_param = 10.0**param_opt
            env = {}
            optimal_llf_value = llf_fun(optimal_param, env, _adopt=True)
            param, i = {}, 0
            for name, len_ in zip(par_list, par_len):
                param[name] = optimal_param[i : i + len_]
                i += len_
            return param, optimal_llf_value, env, optimal_param
        streams = min(int(getattr(self, "restart_streams", 1) or 1), self.random_start)
        if streams > 1 and dist is None and not restricted:
            param_opt, llf_opt = self._restarts_on_streams(streams, log10param, log10bounds, eval_budget)
            optimal_param = 10.0**param_opt
            env = {}
            optimal_llf_value = llf_fun(optimal_param, env, _adopt=True)
            param, i = {}, 0
            for name, len_ in zip(par_list, par_len):
                param[name] = optimal_param[i : i + len_]
                i += len_
            return param, optimal_llf_value, env, optimal_param
        ahead = int(getattr(self, "restart_lookahead", 0) or 0)
        if ahead < 0:
            ahead = 2 if len(self.X) >= 1500 else 1
        ahead = min(ahead, self.random_start - 1, 3)
        looked = None
        if ahead > 0 and dist is None and not restricted:
            # (None: the worker engines could not be set up -- device memory -- and nothing was drawn or evaluated: the plain loop below runs)
            looked = self._restarts_with_lookahead(ahead, log10param, log10bounds, eval_budget)
        if looked is not None:
            param_opt, llf_opt = looked
            optimal_param = 10.0**param_opt
            env = {}
            optimal_llf_value = llf_fun(optimal_param, env, _adopt=True)
            param, i = {}, 0
            for name, len_ in zip(par_list, par_len):
                param[name] = optimal_param[i : i + len_]
                i += len_
            return param, optimal_llf_value, env, optimal_param
        wait_count = 0
        param_opt, llf_opt = np.array(log10param, dtype=float), np.inf
        first = True
        for iteration in range(self.random_start):
            if iteration != 0:
                log10param = np.random.uniform(log10bounds[:, 0], log10bounds[:, 1])
            if iteration % world != rank:
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                param_opt_, llf_opt_, info = fmin_l_bfgs_b(obj_func, log10param, bounds=log10bounds, maxfun=eval_budget)
            if first:
                param_opt, llf_opt, first = param_opt_, llf_opt_, False
            elif llf_opt_ <= llf_opt:
                param_opt, llf_opt = param_opt_, llf_opt_
                wait_count = 0
            else:
                wait_count += 1
            if self.verbose:
                print("MLE restart %d: %d likelihood evaluations, best llf so far %.10g" % (iteration + 1, info["funcalls"], -llf_opt))
            eval_budget -= info["funcalls"]
            if eval_budget <= 0 or wait_count >= self.wait_iter:
                break
        if world > 1:
            for _ in range(iteration + 1, self.random_start):  # (as in _restarts_in_lock_step: every rank consumes random_start - 1 draws)
                np.random.uniform(log10bounds[:, 0], log10bounds[:, 1])
            param_opt, llf_opt = distributed.exchange_best_parameters(np.asarray(param_opt, float), float(llf_opt))

        optimal_param = 10.0**param_opt
        env = {}
        optimal_llf_value = llf_fun(optimal_param, env, _adopt=True)  # :1185-1188; keeps the state it builds
        param, i = {}, 0
        for name, len_ in zip(par_list, par_len):
            param[name] = optimal_param[i : i + len_]
            i += len_
        return param, optimal_llf_value, env, optimal_param

    def _restarts_in_lock_step(self, batch, log10param0, log10bounds, eval_budget, restricted, rank=0, world=1):
        """The MLE restarts of gpr.py:1127-1162 advanced together, `batch` at a time (bogp_mle_batch): every round of the
        lock-step loop evaluates the current trial point of each active restart with ONE batched likelihood call (one workgroup a
        restart for N <= 156, the elimination kernels over `batch` workspaces up to N = 2048), and the optimiser is libbogp's own
        L-BFGS-B -- the published algorithm scipy's fmin_l_bfgs_b implements, with its defaults, as a re-entrant state machine
        (tests/test_lbfgsb.py follows scipy's iterates) -- so no Python runs between evaluations.

        The reference's bookkeeping is kept at WAVE granularity: wave w starts restarts w * batch ... (start points drawn from the
        global np.random in the sequential loop's order, the first being the warm start), its runs share the remaining evaluation
        budget, and after the wave the best value / stagnation counter / budget are updated restart by restart exactly as
        gpr.py:1142-1162 does (`<=`: a later restart wins a tie).  batch = 1 is therefore the reference's loop with libbogp's optimiser;
        batch >= random_start starts every restart, where the sequential loop may stop after `wait_iter` of them bring nothing."""
        tid, est, beta = self._trend_args()
        mode, nv, kid = self._MODE[self.estimation_mode], self._nv(), self.kernel_id
        if restricted:  # the REML objective takes the fixed nugget of the noisy mode as an argument (gpr.py:826-834)
            nv = self._nv() if self.estimation_mode == "noisy" else 0.0
        lo, hi = np.ascontiguousarray(log10bounds[:, 0]), np.ascontiguousarray(log10bounds[:, 1])
        param_opt, llf_opt, first, wait_count = np.array(log10param0, dtype=float), np.inf, True, 0
        self.eval_count, self.mle_rounds = 0, 0
        it = 0
        while it < self.random_start:
            # the next wave: up to `batch` restarts of THIS rank; the start points of the other ranks' restarts are drawn and dropped so
            # that every rank consumes the global stream alike
            starts, idx = [], []
            while it < self.random_start and len(starts) < batch:
                x = np.array(log10param0, dtype=float) if it == 0 else np.random.uniform(lo, hi)
                if it % world == rank:
                    starts.append(x)
                    idx.append(it)
                it += 1
            n_w = len(starts)
            if n_w == 0:
                break
            xopt, fopt, nev, status, rounds = self.engine.mle_batch(kid, mode, np.array(starts), lo, hi, nv, est, beta, trend=tid,
                                                                    restricted=restricted, eval_budget=int(eval_budget),
                                                                    chain_rule=bool(getattr(self, "mle_chain_rule", False)),
                                                                    prune_reserve=int(getattr(self, "mle_prune_reserve", 0)))  # fmt: skip
            self.mle_rounds += rounds
            stop = False
            for r in range(n_w):
                if first:
                    param_opt, llf_opt, first = xopt[r], fopt[r], False
                elif fopt[r] <= llf_opt:
                    param_opt, llf_opt = xopt[r], fopt[r]
                    wait_count = 0
                else:
                    wait_count += 1
                if self.verbose:
                    print("MLE restart %d (lock step): %d likelihood evaluations, status %d, best llf so far %.10g" % (idx[r] + 1, nev[r], status[r], -llf_opt))
                self.eval_count += int(nev[r])
                eval_budget -= int(nev[r])
                if eval_budget <= 0 or wait_count >= self.wait_iter:
                    stop = True  # (the whole wave has already run: its later restarts still count, as above)
            if stop:
                break
        if world > 1:
            # ranks leave the loop on their OWN budget / stagnation counters: the start points of the restarts nobody ran are still drawn,
            # so that every rank has consumed exactly random_start - 1 draws and the identically seeded global streams stay identical for
            # whatever samples next
            while it < self.random_start:
                np.random.uniform(lo, hi)
                it += 1
        self._committed_par = None  # (the batched paths leave the factor buffers alone, the fallback paths do not)
        return np.asarray(param_opt, dtype=float), float(llf_opt)

    def _restarts_with_lookahead(self, ahead, log10param0, log10bounds, eval_budget):
        """The reference's sequential restart loop (gpr.py:1127-1162) -- same restarts, same order, same shared budget, same stagnation stop,
        same draws from the global np.random, same evaluation count, same result BIT FOR BIT -- with the next `ahead` restarts run
        SPECULATIVELY on further engines of the same GPU (own HIP stream, own factor buffers, one host thread each; ctypes releases the GIL)
        while the current one runs.  A likelihood evaluation up to N ~ 4000 is a chain of small launches that leaves most of the GPU idle,
        and two independent chains interleave (profiles/r05_nll_two_handles.txt); a default BO loop is 95 % such evaluations.

        Why this is exact.  A restart is a deterministic function of (start point, maxfun): the engines run the same kernels with the same
        launch geometry, and nothing in an evaluation touches np.random.  What restart i + 1 inherits from restart i is only (a) whether it
        runs at all (budget left, stagnation counter), (b) its maxfun = the budget left.  So it is launched with the budget known at launch
        time -- an upper bound of (b) -- and its start point is drawn early, with the generator's state saved before the draw:
          * if the loop stops before it, it is cancelled and the generator is put back (the draw never happened);
          * if it used no more evaluations than the budget it really had, scipy's `evaluations > maxfun` test (made at every new iterate)
            could not have fired either way: the result IS the sequential one;
          * otherwise (it ran into the end of the budget) it is re-run with the true maxfun -- which is what the sequential loop does.
        `restart_lookahead=0` (or BOGP_RESTART_LOOKAHEAD=0) runs the plain loop."""
        import threading
        from concurrent.futures import ThreadPoolExecutor

        lo, hi = log10bounds[:, 0], log10bounds[:, 1]
        make = type(self.engine)  # (the oracle-backed stand-in of the CPU tests speculates on stand-ins)
        # A worker engine holds its own factor buffers (4 to 6 N^2 doubles).  If one cannot be created or loaded -- another process on the
        # GPU, a very large N -- the fit must not fail where the sequential loop would have run: the workers that did come up are kept, the
        # broken one is destroyed, and with none at all the caller runs the plain loop (nothing has been drawn or evaluated yet).
        ready = []
        for k in range(ahead):
            eng = None
            try:
                if k < len(self._worker_engines):
                    eng = self._worker_engines[k]
                else:
                    eng = make(self.device)
                eng.set_train(self.X, self.y)
                ready.append(eng)
            except Exception as exc:  # noqa: BLE001 -- HIP out-of-memory surfaces as the library's RuntimeError
                if eng is not None:
                    try:
                        eng.close()
                    except Exception:  # noqa: BLE001
                        pass
                if self.verbose:
                    print("MLE look-ahead: worker engine %d unavailable (%s); %d in use" % (k + 1, exc, len(ready)))
                break
        for eng in self._worker_engines:
            if not any(eng is r for r in ready):
                try:
                    eng.close()
                except Exception:  # noqa: BLE001
                    pass
        self._worker_engines = list(ready)
        if not ready:
            self.lookahead_stats = dict(restarts=0, speculated=0, rerun=0, cancelled=0, fallback=1)
            return None
        ahead = len(ready)
        W = ahead + 1
        engines = [self.engine] + ready
        tid, est, beta = self._trend_args()
        mode, nv, kid = self._MODE[self.estimation_mode], self._nv(), self.kernel_id

        class _Cancelled(Exception):
            pass

        def run(eng, start, maxfun, cancel):
            calls = [0]

            def obj(log10param):  # what obj_func of the sequential loop returns, value for value
                if cancel is not None and cancel.is_set():
                    raise _Cancelled()
                calls[0] += 1
                par = 10.0 ** np.array(log10param)
                if not (np.all(np.isfinite(par)) and np.all(par > 0)):
                    return -1.0 * -np.inf, -1.0 * np.zeros(len(par))
                try:
                    llf, grad = eng.nll(kid, mode, self._epar(par), nv, est, beta, eval_grad=True, trend=tid)
                except _lib.NotPositiveDefinite:
                    return -1.0 * -np.inf, -1.0 * np.zeros(len(par))
                return -1.0 * llf, -1.0 * np.asarray(grad, dtype=float).ravel()

            try:
                p_, l_, info = fmin_l_bfgs_b(obj, start, bounds=log10bounds, maxfun=maxfun)
            except _Cancelled:
                return None
            return p_, l_, info, calls[0]

        from concurrent.futures import FIRST_COMPLETED, wait

        depth = max(ahead, 4)  # restarts that may be in flight or finished-and-waiting beyond the current one: an engine that finishes a short
        #                        restart early takes the next one instead of idling behind a long restart i
        inflight = {}  # restart index -> (future, engine index, maxfun it was given, generator state before its draw, cancel event, start point)
        busy = [None] * W  # the future each engine is working on
        stats = dict(restarts=0, speculated=0, rerun=0, cancelled=0)  # (kept in self.lookahead_stats: tests, `verbose`)
        next_it, budget, wait_count, first, most = 0, int(eval_budget), 0, True, 0
        param_opt, llf_opt = np.array(log10param0, dtype=float), np.inf
        self.eval_count = 0

        def launch_what_fits(it):
            nonlocal next_it
            while next_it < self.random_start and next_it <= it + depth:
                free = [e for e in range(W) if busy[e] is None or busy[e].done()]
                if not free:
                    return
                # speculate only while the budget is roomy: a restart that runs into the end of the budget it was GUESSED to have must be
                # re-run with the real one, and near the end of the budget that is the common case (twice the largest restart so far, per
                # restart between here and there)
                if next_it > it and budget < 2 * max(most, 1) * (next_it - it + 1):
                    return
                state = np.random.get_state() if next_it != 0 else None
                start = np.array(log10param0, dtype=float) if next_it == 0 else np.random.uniform(lo, hi)
                e = free[0]
                cancel = threading.Event()
                busy[e] = pool.submit(run, engines[e], start, budget, cancel)
                inflight[next_it] = (busy[e], e, budget, state, cancel, start)
                stats["speculated"] += int(next_it > it)
                next_it += 1

        with warnings.catch_warnings():  # (ONE context around the pool: catch_warnings is not thread-safe)
            warnings.simplefilter("ignore")
            with ThreadPoolExecutor(max_workers=W) as pool:
              it = 0
              try:
                while it < self.random_start:
                    launch_what_fits(it)
                    fut = inflight[it][0]
                    while not fut.done():  # whenever ANY restart finishes, its engine may take the next speculative one
                        wait([f for f in busy if f is not None and not f.done()], return_when=FIRST_COMPLETED)
                        launch_what_fits(it)
                    fut, e, spec_budget, _, _, start = inflight.pop(it)
                    p_, l_, info, calls = fut.result()
                    if spec_budget != budget and info["funcalls"] > budget:
                        # it ran into a budget it did not have: the sequential call, on an engine that is idle NOW (its own may have moved on)
                        idle = [k for k in range(W) if busy[k] is None or busy[k].done()]
                        if not idle:
                            wait([f for f in busy if f is not None], return_when=FIRST_COMPLETED)
                            idle = [k for k in range(W) if busy[k] is None or busy[k].done()]
                        busy[idle[0]] = pool.submit(run, engines[idle[0]], start, budget, None)
                        p_, l_, info, calls = busy[idle[0]].result()
                        stats["rerun"] += 1
                    stats["restarts"] += 1
                    if first:
                        param_opt, llf_opt, first = p_, l_, False
                    elif l_ <= llf_opt:
                        param_opt, llf_opt = p_, l_
                        wait_count = 0
                    else:
                        wait_count += 1
                    if self.verbose:
                        print("MLE restart %d: %d likelihood evaluations, best llf so far %.10g" % (it + 1, info["funcalls"], -llf_opt))
                    self.eval_count += calls
                    budget -= info["funcalls"]
                    most = max(most, int(info["funcalls"]))
                    it += 1
                    if budget <= 0 or wait_count >= self.wait_iter:
                        break
              finally:
                # restarts launched beyond the loop's end -- or beyond an exception of the current one (a HIP error, an unsupported
                # configuration) -- never happened: stop them, wait for their threads, and un-draw their start points, so that the global
                # generator is where the sequential loop would have left it on this path too
                rest = sorted(inflight)
                for j in rest:
                    inflight[j][4].set()
                for j in rest:
                    try:
                        inflight[j][0].result()
                    except Exception:  # noqa: BLE001 -- a speculative restart's own failure dies with it
                        pass
                states = [inflight[j][3] for j in rest if inflight[j][3] is not None]
                if states:
                    np.random.set_state(states[0])
                stats["cancelled"] = len(rest)
        self.lookahead_stats = stats
        self._committed_par = None
        if len(self.X) >= 4096:  # the workers' factor buffers (>= 0.5 GB each from here on) go back to the device between fits
            for eng in self._worker_engines:
                try:
                    eng.close()
                except Exception:  # noqa: BLE001
                    pass
            self._worker_engines = []
        return np.asarray(param_opt, dtype=float), float(llf_opt)

    def _restarts_on_streams(self, streams, log10param0, log10bounds, eval_budget):
        """The MLE restarts of gpr.py:1127-1162 on `streams` engines of ONE GPU at once (the single-device flavour of
        `distribute_restarts`): at the training-set sizes of an ordinary BO run a likelihood evaluation is a chain of ~15 small
        launches (0.1-0.3 ms) that leaves the GPU idle, and `tell()` is several hundred of them -- 98 % of a 200-evaluation run's wall
        time (profiles/r03_bo_loop.txt).  Restart i runs on worker i % streams (its own engine = its own HIP stream and factor buffers;
        ctypes releases the GIL during every call) with 1 / streams of the budget and its own stagnation counter; ALL starting points
        come from the global np.random stream in the sequential loop's order, so the union of starts is the sequential run's; the best
        (-llf, parameters) wins, ties to the lowest worker.  Opt-in: it relaxes the shared budget exactly as `distribute_restarts` does."""
        from concurrent.futures import ThreadPoolExecutor

        starts = [np.array(log10param0, dtype=float)]
        for _ in range(1, self.random_start):
            starts.append(np.random.uniform(log10bounds[:, 0], log10bounds[:, 1]))
        budget = max(1, -(-int(eval_budget) // streams))
        tid, est, beta = self._trend_args()
        mode, nv, kid = self._MODE[self.estimation_mode], self._nv(), self.kernel_id
        while len(self._worker_engines) < streams:
            self._worker_engines.append(_lib.Engine(self.device))
        for eng in self._worker_engines[:streams]:
            eng.set_train(self.X, self.y)

        def worker(w):
            eng = self._worker_engines[w]
            calls = [0]

            def obj(log10param):
                calls[0] += 1
                par = 10.0 ** np.array(log10param)
                if not (np.all(np.isfinite(par)) and np.all(par > 0)):
                    return np.inf, np.zeros(len(par))
                try:
                    llf, grad = eng.nll(kid, mode, par, nv, est, beta, eval_grad=True, trend=tid)
                except _lib.NotPositiveDefinite:
                    return np.inf, np.zeros(len(par))
                return -1.0 * llf, -1.0 * np.asarray(grad, dtype=float).ravel()

            best_p, best_l, first, wait, left = None, np.inf, True, 0, budget
            for it in range(w, self.random_start, streams):
                p_, l_, info = fmin_l_bfgs_b(obj, starts[it], bounds=log10bounds, maxfun=left)
                if first:
                    best_p, best_l, first = p_, l_, False
                elif l_ <= best_l:
                    best_p, best_l, wait = p_, l_, 0
                else:
                    wait += 1
                left -= info["funcalls"]
                if left <= 0 or wait >= self.wait_iter:
                    break
            return best_p, float(best_l), calls[0]

        # (ONE warnings context, entered by the calling thread around the pool: catch_warnings saves / restores the process-global
        # filter list and is not thread-safe, so the workers must not enter their own)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with ThreadPoolExecutor(max_workers=streams) as pool:
                results = list(pool.map(worker, range(streams)))
        self.eval_count = sum(r[2] for r in results)
        best = min(range(streams), key=lambda w: (results[w][1], w))
        if self.verbose:
            print("MLE on %d streams: %d likelihood evaluations, best llf %.10g (worker %d)" % (streams, self.eval_count, -results[best][1], best))
        return np.asarray(results[best][0], dtype=float), results[best][1]

    def fit(self, X, y):
        """gpr.py:355-417.  Returns self; sets `is_fitted`."""
        if self.kernel_id in (_lib.KERNEL_CUBIC, _lib.KERNEL_GENEXP, _lib.KERNEL_MATERN_NU):
            # the MLE needs d llf / d theta; for these two the reference's own fit raises UnboundLocalError at gpr.py:1001
            # (corr_grad_theta :763-766 defines nothing).  Pinned hyper-parameters work: set_state / predict / sweep.
            raise NotImplementedError("corr=%r has no theta-derivative (neither here nor in the reference): use set_state(par, X, y)" % (self.corr,))
        self._check_data(X, y)
        n_retry = 0
        while True:
            self._committed_par = None  # nothing of an earlier (or rejected) state survives into this optimisation
            self.par, self.log_likelihood_, env, optimal_param = self._optimize_hyperparameter()
            if np.isinf(self.log_likelihood_):
                print("Invalid likelihood value. Increasing nugget...")  # gpr.py:384-399
                if self.estimation_mode == "noiseless":
                    self.estimation_mode = "noisy"
                    self.noise_var = 1e-5
                else:
                    self.noise_var = np.atleast_1d(self.noise_var) * 10
                n_retry += 1
                if n_retry > 12:  # the reference loops forever; bound it (noise_var would exceed 1e7)
                    raise np.linalg.LinAlgError("likelihood stays -inf after %d nugget increases" % n_retry)
            else:
                break
        # `log_likelihood_concentrated(par, env)` committed the model at the optimum: pull the attributes
        self._pull_state(optimal_param)
        self.is_fitted = True
        return self

    def update(self, X, y):
        self.fit(X, y)
        return self

    def set_state(self, par, X=None, y=None):
        """Pin a fitted state at given hyper-parameters without running the MLE (what SURVEY.md Appendix A does to
        the reference with `_check_data` + one likelihood call + attribute copy).  Returns the log-likelihood."""
        if X is not None:
            self._check_data(X, y)
        par = np.asarray(par, dtype=float).ravel()
        llf = self._commit(par)
        self.log_likelihood_ = llf
        self.is_fitted = True
        return llf

    # ------------------------------------------------------------------------------------------------
    # posterior (gpr.py:424-535) and its input-gradient (gpr.py:537-576)
    # ------------------------------------------------------------------------------------------------
    def _check_X(self, X):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        if X.ndim != 2:
            raise ValueError("Expected 2D array, got %dD array instead" % X.ndim)
        if X.shape[0] == 0:  # sklearn's check_array, which the reference calls first (gpr.py:460)
            raise ValueError("Found array with 0 sample(s) (shape=%s) while a minimum of 1 is required." % (X.shape,))
        if X.shape[1] != self.X.shape[1]:
            raise ValueError(
                "The number of features in X (X.shape[1] = %d) should match the number of features used for fit() which is %d."
                % (X.shape[1], self.X.shape[1])
            )
        if not np.isfinite(X).all():
            raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
        return np.ascontiguousarray(X)

    def predict(self, X, eval_MSE=False, batch_size=None):
        assert hasattr(self, "X")
        if self._committed_par is None:
            raise Exception("The model is not fitted yet!")
        X = self._check_X(X)
        if batch_size is not None and (type(batch_size) is not int or batch_size <= 0):
            raise Exception("batch_size must be a positive integer")
        eng = self.engine
        eng.upload_candidates(X)
        n_t = self.y.shape[1]
        if n_t > 1:  # (M, n_targets) like gpr.py:490, 502-505; the factorisation is shared by the targets
            # MSE = (1 - sum rt^2 + sum u^2) sigma2_t: when the targets share sigma2 (always in the noisy mode, gpr.py:970) the
            # variance of target 0 IS the variance of every target, so the others take the mean-only path (no contraction)
            same_var = bool(np.all(np.asarray(self.sigma2) == np.asarray(self.sigma2).ravel()[0]))
            cols = []
            for t in range(n_t):
                eng.select_target(t)
                cols.append(eng.predict(eval_MSE=eval_MSE and (t == 0 or not same_var)))
            eng.select_target(0)
            mu = np.column_stack([c[0] for c in cols])
            if not eval_MSE:
                return mu
            return mu, np.column_stack([cols[0][1] if c[1] is None else c[1] for c in cols])
        mu, mse = eng.predict(eval_MSE=eval_MSE)
        if eval_MSE:
            return mu.reshape(-1, 1), mse.reshape(-1, 1)
        return mu.reshape(-1, 1)

    def gradient(self, x):
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        if x.shape[1] != self.X.shape[1]:
            raise Exception("x does not have the right size!")
        if x.shape[0] != 1:
            raise Exception("x must be a vector!")
        if type(self.mean).__name__ == "quadratic_trend":
            raise NotImplementedError  # quadratic_trend.Jacobian raises in the reference (trend.py:138-139)
        if self.y.shape[1] > 1:  # the reference's gradient raises ValueError (a broadcast of (n_targets,) with (1, d))
            raise NotImplementedError("gradient of a multi-target model")
        dmu, dmse = self.engine.gradient(x[0])
        return dmu.reshape(-1, 1), dmse.reshape(-1, 1)

    def sampling_prior(self, X, n_samples=1, n_features=1024, seed=None):
        """`n_samples` prior paths beta + z(x) at the rows of X: (len(X), n_samples).  A stub in the reference (gpr.py:312-313)."""
        from . import thompson

        return thompson.sample(self, X, n_samples, n_features, seed, conditioned=False)

    def sampling_posterior(self, X, n_samples=1, n_features=1024, seed=None):
        """`n_samples` posterior sample paths at the rows of X: (len(X), n_samples), mean `predict`'s mu and variance its MSE.  A
        stub in the reference (gpr.py:315-316); `bogp.thompson` has the construction and what it refuses."""
        from . import thompson

        return thompson.sample(self, X, n_samples, n_features, seed, conditioned=True)

    def Hessian(self, x):
        """Hessian of the posterior mean at one row (gpr.py:578-598): (d, d).  As in the reference it exists for the
        squared-exponential kernel (corr_Hessian, :663-734, defines no other) and the constant / linear trends."""
        if self._committed_par is None:
            raise Exception("The model is not fitted yet!")
        x = np.atleast_2d(np.asarray(x, dtype=np.float64))
        if x.shape[1] != self.X.shape[1]:
            raise Exception("x does not have the right size!")
        if x.shape[0] != 1:
            raise Exception("x must be a vector!")
        if self.kernel_id != _lib.KERNEL_SE or type(self.mean).__name__ == "quadratic_trend" or self.y.shape[1] != 1:
            raise NotImplementedError("Hessian: squared_exponential kernel, constant or linear trend, one target")
        return self.engine.hessian(x[0])

    def prior_cov(self, X1, X2=None, corr=False):
        """Prior correlation / covariance between the rows of X1 (gpr.py:318-353).  `X2` is accepted as None only: the
        reference's `if X2` raises for any array."""
        if X2 is not None:
            raise ValueError("The truth value of an array with more than one element is ambiguous. Use a.any() or a.all()")
        if self._committed_par is None:
            raise Exception("The model is not fitted yet!")
        X1 = self._check_X(np.atleast_2d(X1))
        R = self.engine.prior_corr(X1)
        if corr:
            return R
        n_t = self.y.shape[1]
        C_prior = np.array([self.sigma2[i] * R for i in range(n_t)])  # :350-351
        return np.sqrt((C_prior**2.0).sum(axis=0) / n_t)

    def _fused_point_ok(self) -> bool:
        """bogp_point_eval serves the constant and (r05) the linear trend basis -- the two the reference's `gradient` can differentiate
        (gpr.py:556-575; quadratic_trend.Jacobian raises, trend.py:138-139) -- with a single target."""
        return self._trend_args()[0] in (_lib.TREND_CONSTANT, _lib.TREND_LINEAR) and self.y.shape[1] == 1

    def gradient_batch(self, X):
        """`gradient` at B rows in one device call: (d mu / dx (B, d), d MSE / dx (B, d)).  Not in the reference
        (its gradient takes one row, gpr.py:548-549); SURVEY.md 8 f2."""
        if self._committed_par is None:
            raise Exception("The model is not fitted yet!")
        X = self._check_X(X)
        if not self._fused_point_ok():  # the quadratic basis / several targets: row by row (and the reference's errors)
            rows = [self.gradient(x.reshape(1, -1)) for x in X]
            return np.array([r[0].ravel() for r in rows]), np.array([r[1].ravel() for r in rows])
        return self.engine.gradient_batch(X)
