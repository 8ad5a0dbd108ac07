"""Acquisition functions on the GPU engine: drop-in for `bayes_optim.acquisition.acquisition_fun`.

Protocol mirrored: classes are looked up BY NAME (`base.py:485-488`), built with keywords
`model, minimize, [plugin], [t | alpha | epsilon]`, `hasattr(cls, "plugin")` decides plugin injection
(`bayes_opt.py:21-23`), `ParallelBO` reads the default `t` / `alpha` / `epsilon` off an instance
(`bayes_opt.py:96-98`), and the object is called as `criterion(X, return_dx=bool)` (`utils.py:184-195`).

Implementation is table-driven rather than a copy of the reference's class bodies:
  * values come from libbogp's acquisition kernel -- ONE device launch for any number of rows
    (closed forms + guards of `acquisition_fun.py:127-135, 153-176, 208-217, 265-290` live in csrc/kernels_acq.hip);
  * the `return_dx` chain rule (rows a12: `:139-146, 181-188, 220-227, 292-309`) is evaluated on the host from
    `model.gradient`, one row per call like the reference, through the shared `_Moments` helper.

Batched semantics (the reference raises ValueError for EI / EpsilonPI / MGFI on more than one row): row i of the
result is what the reference's single-row call returns for row i, guards included; with `return_dx=True` and several
rows the chain rule itself runs on the device (`bogp_point_eval_batch`) and the answer is (values (M, 1), dx (M, d)).
Return shapes follow the reference: one row -> shape (1,) for EI / MGFI / UCB (its Python `sum` over a (1,1) array)
and (1,1) for EpsilonPI; M rows -> (M, 1).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
from scipy.special import ndtr

from . import _lib
from . import forest as _forest


class norm:  # noqa: N801 -- the two members of scipy.stats.norm the chain rules use, without its argument-checking machinery
    """`scipy.stats.norm.pdf / cdf` at loc = 0, scale = 1 are exactly `exp(-x**2 / 2) / sqrt(2 pi)` and `special.ndtr(x)`
    (scipy/stats/_continuous_distns.py: `_norm_pdf`, `_norm_cdf`); calling those directly gives the same bits at a tenth
    of the host time -- the reference's BFGS loop evaluates them once per point."""

    _C = np.sqrt(2 * np.pi)

    @staticmethod
    def pdf(x):
        return np.exp(-np.asarray(x) ** 2 / 2.0) / norm._C

    @staticmethod
    def cdf(x):
        return ndtr(x)


class _PositiveParameter:
    """Data descriptor for a strictly positive criterion parameter (the reference asserts `> 0` in every setter:
    alpha `:123-125`, epsilon `:204-206`, t `:259-263`), with an optional transform (MGFI clamps t at 22.36)."""

    def __init__(self, transform: Optional[Callable[[float], float]] = None, zero_ok_attr: Optional[str] = None):
        self.transform = transform
        self.zero_ok_attr = zero_ok_attr

    def __set_name__(self, owner, name):
        self.slot = "_" + name

    def __get__(self, obj, objtype=None):
        return self if obj is None else getattr(obj, self.slot)

    def __set__(self, obj, value):
        zero_ok = bool(self.zero_ok_attr and getattr(obj, self.zero_ok_attr, False))
        assert value > 0 or (zero_ok and value == 0)
        setattr(obj, self.slot, self.transform(value) if self.transform else value)


class _Moments:
    """Posterior moments and their input-gradients at ONE row, in the orientation the criteria use:
    y (sign-flipped when maximising, `:52-64`), sd = sqrt(MSE), dy and dsd as (1, d) rows (`:66-80`)."""

    def __init__(self, criterion: "AcquisitionFunction", X: np.ndarray, moments=None):
        model, sign = criterion.model, (1.0 if criterion.minimize else -1.0)
        if moments is None:
            mu, mse = model.predict(X, eval_MSE=True)
            dmu, dmse = model.gradient(np.array(X, dtype=float))
        else:  # already computed by the fused one-point device call
            mu, mse, dmu, dmse = moments
        self.y = sign * mu
        self.sd = np.sqrt(mse)
        self.dy = sign * dmu.T
        with np.errstate(all="ignore"):
            self.dsd = dmse.T / (2.0 * self.sd)
        self.d = X.shape[1]

    def zeros(self):
        return np.zeros((self.d, 1))  # the shape of the reference's guard / exception fall-backs


class AcquisitionFunction:
    """Common machinery; concrete criteria set `acq_id` and override `_par` / `_dx`."""

    acq_id: int = -1

    def __init__(self, model=None, minimize: bool = True):
        self.model = model
        self.minimize = minimize

    @property
    def model(self):
        return self._model

    @model.setter
    def model(self, model):
        if model is None:
            raise ValueError("model cannot be None")
        assert hasattr(model, "predict")
        self._model = model

    # -- what the sweep needs from a criterion ----------------------------------------------------------
    def acq_par(self) -> float:
        return 0.0

    def effective_plugin(self) -> float:
        return 0.0

    def check_X(self, X) -> np.ndarray:
        return np.atleast_2d(np.asarray(X, dtype=float))

    # -- evaluation ---------------------------------------------------------------------------------------
    def _values(self, X: np.ndarray) -> np.ndarray:
        """Posterior + this criterion for all rows of X in one device call (bogp_sweep with acq_out)."""
        if getattr(self._model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        eng = self._model.engine
        eng.upload_candidates(self._model._check_X(X))
        _, _, vals = eng.sweep([(self.acq_id, self.acq_par())], self.effective_plugin(), self.minimize, return_values=True)
        return vals[0]

    _single_row_shape = (1,)

    def _fused_point(self, X: np.ndarray):
        """value + moments + their gradients at one row in ONE device call (bogp_point_eval), or None when the model
        needs the separate predict / gradient entry points (polynomial trend basis, several targets, foreign model)."""
        model = self._model
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        eng = getattr(model, "engine", None)
        fused = getattr(model, "_fused_point_ok", None)
        if eng is None or fused is None or not hasattr(eng, "point_eval") or not fused():
            return None
        x = model._check_X(X)
        mu, mse, dmu, dmse, vals = eng.point_eval(x[0], [(self.acq_id, self.acq_par())], self.effective_plugin(), self.minimize)
        mom = (np.array([[mu]]), np.array([[mse]]), dmu.reshape(-1, 1), dmse.reshape(-1, 1))
        return vals, mom

    def __call__(self, X, return_dx: bool = False):
        if _forest.is_forest_model(self._model):  # moments of the packed forest (bogp_forest_sweep_topk); rows keep their level labels
            if return_dx:
                raise NotImplementedError("a forest has no input gradient (the reference's RandomForest has none either): return_dx=True is not served")
            v = _forest.criterion_values(self, X)
            return v.reshape(self._single_row_shape) if len(v) == 1 else v.reshape(-1, 1)
        X = self.check_X(X)
        if X.shape[0] == 1:  # the one-point call of the reference's inner optimisers: one device round trip
            fused = self._fused_point(X)
            if fused is not None:
                value = fused[0].reshape(self._single_row_shape)
                return self._dx(_Moments(self, X, fused[1]), value) if return_dx else value
        if return_dx and X.shape[0] != 1:
            # the reference stops here ("x must be a vector!", gpr.py:548-549).  Row i of the answer below is what its
            # one-row call returns for row i: (values (M, 1), gradients (M, d)), one device round trip for all rows
            # (bogp_point_eval_batch evaluates the chain rule of `_dx` on the device)
            model, eng = self._model, getattr(self._model, "engine", None)
            fused = getattr(model, "_fused_point_ok", None)
            if eng is None or fused is None or not hasattr(eng, "point_eval_batch") or not fused():
                raise Exception("x must be a vector!")
            if getattr(model, "_committed_par", None) is None:
                raise Exception("The model is not fitted yet!")
            _, _, _, _, vals, dvals = eng.point_eval_batch(model._check_X(X), [(self.acq_id, self.acq_par())], self.effective_plugin(), self.minimize)
            return vals.reshape(-1, 1), dvals[:, 0, :]
        v = self._values(X)
        value = v.reshape(self._single_row_shape) if X.shape[0] == 1 else v.reshape(-1, 1)
        if not return_dx:
            return value
        return self._dx(_Moments(self, X), value)

    def _dx(self, m: _Moments, value):
        raise NotImplementedError


class ImprovementBased(AcquisitionFunction):
    """Criteria measured against a plug-in value: best observed fitness unless given (`:87-104`).
    The stored value is already oriented for minimisation (negated when maximising)."""

    def __init__(self, plugin: float = None, **kwargs):
        super().__init__(**kwargs)
        self.plugin = plugin

    @property
    def plugin(self):
        return self._plugin

    @plugin.setter
    def plugin(self, value):
        sign = 1.0 if self.minimize else -1.0
        if value is not None:
            self._plugin = sign * value
        elif hasattr(self._model, "y"):
            y = self._model.y
            self._plugin = np.min(y) if self.minimize else sign * np.max(y)
        else:
            self._plugin = None

    def effective_plugin(self) -> float:
        if self._plugin is None:  # the model had no data when the criterion was built: resolve now
            self.plugin = None
        return float(self._plugin)


class UCB(AcquisitionFunction):
    """y + alpha sd, maximised as-is even when minimising (`:107-147`)."""

    acq_id = _lib.ACQ_UCB
    alpha = _PositiveParameter()

    def __init__(self, alpha: float = 0.5, **kwargs):
        super().__init__(**kwargs)
        self.alpha = alpha

    def acq_par(self):
        return float(self.alpha)

    def _dx(self, m, value):
        return value, m.dy + self.alpha * m.dsd


class EI(ImprovementBased):
    """Expected improvement (`:150-189`)."""

    acq_id = _lib.ACQ_EI

    def _dx(self, m, value):
        if m.sd / np.sqrt(self._model.sigma2) < 1e-6:  # the small-variance guard returns (0, zeros)
            return 0, m.zeros()
        z = (self.plugin - m.y) / m.sd
        return value, norm.pdf(z) * m.dsd - norm.cdf(z) * m.dy


class EpsilonPI(ImprovementBased):
    """epsilon-probability of improvement (`:192-228`)."""

    acq_id = _lib.ACQ_EPSILON_PI
    _allow_zero = False
    _single_row_shape = (1, 1)
    epsilon = _PositiveParameter(zero_ok_attr="_allow_zero")

    def __init__(self, epsilon=1e-10, **kwargs):
        super().__init__(**kwargs)
        self.epsilon = epsilon

    def acq_par(self):
        return float(self.epsilon)

    def _dx(self, m, value):
        shrink = (1 - self.epsilon) if m.y > 0 else (1 + self.epsilon)
        with np.errstate(all="ignore"):
            z = (self._plugin - shrink * m.y) / m.sd
            slope = -(shrink * m.dy + z * m.dsd) * norm.pdf(z) / m.sd
        return value, slope


class PI(EpsilonPI):
    """Probability of improvement = EpsilonPI with epsilon = 0.

    The reference's PI cannot be constructed: it forwards epsilon=0 into a setter that asserts eps > 0
    (`:204-206, 232-235`).  Here epsilon = 0 is admitted for this subclass only."""

    _allow_zero = True

    def __init__(self, **kwargs):
        kwargs["epsilon"] = 0
        super().__init__(**kwargs)


class MGFI(ImprovementBased):
    """Moment-generating function of the improvement (`:238-310`); t is clamped at 22.36 against overflow."""

    acq_id = _lib.ACQ_MGFI
    t = _PositiveParameter(transform=lambda t: min(t, 22.36))

    def __init__(self, t: float = 1, **kwargs):
        super().__init__(**kwargs)
        self.t = t

    def acq_par(self):
        return float(self.t)

    def _dx(self, m, value):
        if np.isclose(m.sd, 0):
            return np.array([0.0]), m.zeros()
        t, plugin, var = self.t, self._plugin, m.sd**2.0
        with np.errstate(all="raise"):
            try:
                z = (plugin - (m.y - t * var)) / m.sd
                scale = np.exp(t * (plugin + t * var / 2 - m.y - 1))
                dz = -((m.dy - 2.0 * t * m.sd * m.dsd) + z * m.dsd) / m.sd
                slope = scale * (norm.pdf(z) * dz + norm.cdf(z) * (t**2 * m.sd * m.dsd - t * m.dy))
            except FloatingPointError:  # the reference turns warnings into a zero gradient
                slope = m.zeros()
        return value, slope


class EHVI:
    """Expected hypervolume improvement of a multi-target device model: drop-in for the reference's
    `bayes_optim.multi_objective.analytic.EHVI` (analytic.py:99-274), which MOBO maximises (mobo.py:177-186).

    The targets are maximised as given (MOBO passes `y * (-1) ** minimize`, mobo.py:66-76).  The cells of the region the
    front does not dominate come from exactly one of
      Y            the observed objective values (n x m), decomposed by `bogp.pareto.hypercell_bounds`;
      partitioning the reference's partitioning object, read through `.pareto_Y` and `.get_hypercell_bounds()`;
      cells        (lower, upper), each C x m (upper may hold +inf).
    `criterion(X)` returns one value per row, shape (M,): row i is what the reference's one-row call returns for row i
    (computed in float64 -- the reference casts mu / MSE to float32, analytic.py:228-233).  All rows are evaluated in one
    device pass (`bogp_sweep_ehvi`); by default there is no input gradient, as in the reference.

    `input_gradient=True` (an extension, Gaussian-process models only): `criterion(X, return_dx=True)` returns (values, dx)
    in the shapes of the single-objective criteria -- one row: ((1,), (1, d)); M rows: ((M, 1), (M, d)) -- through
    `bogp_point_eval_ehvi` (the closed-form gradient in (mu_k, sd_k) chained with the posterior's input gradients on the
    device), `criterion(X)` for at most 64 rows takes the same call, and `argmax_restart` serves "BFGS", "sweep-BFGS" and
    "sweep-device-BFGS" for it.

    The model may also be a `RandomForest` fitted on y (N, m) -- this package's or the reference's, as MOBO fits it on mixed
    spaces: rows then come in the reference's format (level labels in the categorical columns), and the forest walk and the
    criterion are one device pass (`bogp_forest_sweep_ehvi`).  A forest whose outputs differ from `n_obj` is refused."""

    is_ehvi = True
    minimize = False  # (the sweep helpers read it off every criterion)

    def __init__(self, model=None, ref_point=None, partitioning=None, Y=None, cells=None, input_gradient: bool = False):
        if model is None:
            raise ValueError("model cannot be None")
        if input_gradient and _forest.is_forest_model(model):
            raise NotImplementedError("a forest has no input gradient (the reference's RandomForest has none either): "
                                      "EHVI(input_gradient=True) takes a Gaussian process model")  # fmt: skip
        self.input_gradient = bool(input_gradient)
        if sum(s is not None for s in (partitioning, Y, cells)) != 1:
            raise ValueError("EHVI takes exactly one of partitioning=, Y= and cells=")
        if ref_point is None:
            raise ValueError("EHVI needs a ref_point")
        self.model = model
        self.ref_point = np.asarray(ref_point, dtype=float).ravel()
        m = len(self.ref_point)
        pareto_Y = None
        if partitioning is not None:
            pareto_Y = np.atleast_2d(np.asarray(partitioning.pareto_Y, dtype=float))
            n_out = getattr(partitioning, "num_outcomes", pareto_Y.shape[1])
            if n_out != m:
                raise ValueError("The length of the reference point must match the number of outcomes. Got ref_point with "
                                 "%d elements, but expected %d." % (m, n_out))  # fmt: skip
            b = partitioning.get_hypercell_bounds()
            lower, upper = np.asarray(b[0], dtype=float), np.asarray(b[1], dtype=float)
        elif Y is not None:
            Y = np.atleast_2d(np.asarray(Y, dtype=float))
            if Y.shape[1] != m:
                raise ValueError("The length of the reference point must match the number of outcomes. Got ref_point with "
                                 "%d elements, but expected %d." % (m, Y.shape[1]))  # fmt: skip
            from .pareto import hypercell_bounds, pareto_front

            pareto_Y = pareto_front(Y, self.ref_point)  # (as the reference's partitioning keeps only points above the reference point)
            lower, upper = hypercell_bounds(Y, self.ref_point)
        else:
            lower, upper = (np.asarray(c, dtype=float) for c in cells)
        if pareto_Y is not None and len(pareto_Y) and not np.any(np.all(pareto_Y > self.ref_point, axis=1)):
            raise ValueError("At least one pareto point must be better than the reference point.")
        lower, upper = np.atleast_2d(lower), np.atleast_2d(upper)
        if lower.shape != upper.shape or lower.shape[1] != m:
            raise ValueError("cell bounds must be two C x %d arrays, got %s and %s" % (m, lower.shape, upper.shape))
        if len(lower) > _lib.MAX_EHVI_CELLS:
            raise ValueError("%d cells: at most %d per sweep" % (len(lower), _lib.MAX_EHVI_CELLS))
        self.pareto_Y = pareto_Y
        self.cell_lower_bounds = np.ascontiguousarray(lower)
        self.cell_upper_bounds = np.ascontiguousarray(upper)

    @property
    def n_obj(self) -> int:
        return len(self.ref_point)

    def effective_plugin(self) -> float:
        return 0.0

    def sweep(self, k: int = 1, return_values: bool = False):
        """The EHVI sweep over the engine's current candidates: (best (k,), idx (k,)[, values (M,)])."""
        model = self.model
        if _forest.is_forest_model(model):
            return _forest.ehvi_sweep(self, k=k, return_values=return_values)
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        return model.engine.sweep_ehvi(self.cell_lower_bounds, self.cell_upper_bounds, k=k, return_values=return_values)

    def __call__(self, X, return_dx: bool = False):
        if return_dx and not self.input_gradient:
            raise NotImplementedError("EHVI has no input gradient (the reference's EHVI has none either)")
        if _forest.is_forest_model(self.model):  # rows keep their level labels
            if return_dx:
                raise NotImplementedError("a forest has no input gradient: return_dx=True is not served")
            return _forest.criterion_values(self, X)
        if getattr(self.model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        eng = self.model.engine
        if self.input_gradient:
            rows = self.model._check_X(np.atleast_2d(np.asarray(X, dtype=float)))
            if return_dx or len(rows) <= 64:  # value and gradient in one device round trip (bogp_point_eval_ehvi)
                if not hasattr(eng, "point_eval_ehvi"):
                    raise NotImplementedError("the model's engine has no point_eval_ehvi: no input gradient of EHVI")
                vals, dx = eng.point_eval_ehvi(rows, self.cell_lower_bounds, self.cell_upper_bounds)[:2]
                if not return_dx:
                    return vals
                return (vals.reshape(1), dx.reshape(1, -1)) if len(rows) == 1 else (vals.reshape(-1, 1), dx)
        eng.upload_candidates(self.model._check_X(X))
        return self.sweep(return_values=True)[2]


class Constrained:
    """A single-objective criterion weighted by the probability that modelled constraints hold (`bogp_sweep_constrained`): what the
    reference accepts as `h_vals` / `g_vals` and leaves open (`BaseBO.tell`, base.py:328).  `model` is a device GaussianProcess
    fitted on y (N, m), m >= 2: column 0 the objective, column k the constraint feasible when lo[k - 1] <= c_k(x) <= hi[k - 1]
    (default (-inf, 0] each: g <= 0; an equality |h| <= tol is [-tol, tol]).  Per row

        value = fun(x on column 0) * prod_k P(lo_k <= c_k(x) <= hi_k)

    with `fun` one of "EI" | "PI" | "EpsilonPI" | "MGFI" (the non-negative criteria; `par`: `epsilon` or `t`, defaults as in the
    single-objective classes) or None: the probability of feasibility alone (Gelbart, Snoek, Adams 2014).  "UCB" changes sign
    -- its product with a probability orders nothing -- and raises ValueError.  `plugin=None` takes the best column-0 value among
    the training rows whose constraint columns all lie inside their bounds; with no such row the criterion is feasibility-only
    whatever `fun` says.  The stored plugin is oriented for minimisation, as `ImprovementBased` stores it.

    `criterion(X)` returns one value per row, shape (M,), in one device pass; `criterion.sweep(k, return_values)` sweeps the
    engine's current candidates as `EHVI.sweep` does.  By default there is no input gradient (`return_dx=True` raises).

    `input_gradient=True` (an extension): `criterion(X, return_dx=True)` returns (values, dx) in the shapes
    `EHVI(input_gradient=True)` returns -- one row: ((1,), (1, d)); M rows: ((M, 1), (M, d)) -- through `bogp_point_eval_constrained`
    (the derivative of the probability of feasibility and the criterion's chain rule on the device), `criterion(X)` for at most 64
    rows takes the same call, and `argmax_restart` serves "BFGS", "sweep-BFGS" and "sweep-device-BFGS" for it."""

    is_constrained = True
    _IDS = {"EI": _lib.ACQ_EI, "PI": _lib.ACQ_EPSILON_PI, "EpsilonPI": _lib.ACQ_EPSILON_PI, "MGFI": _lib.ACQ_MGFI, None: _lib.ACQ_NONE}

    def __init__(self, model=None, fun="EI", minimize: bool = True, plugin: float = None, lo=None, hi=None, input_gradient: bool = False,
                 **par):
        if model is None:
            raise ValueError("model cannot be None")
        if _forest.is_forest_model(model):
            raise NotImplementedError("modelled constraints take a multi-target Gaussian process: a forest model is not served")
        self.input_gradient = bool(input_gradient)
        if fun == "UCB":
            raise ValueError("UCB changes sign, so its product with a probability of feasibility orders nothing: use EI, PI, "
                             "EpsilonPI, MGFI or fun=None (feasibility only)")  # fmt: skip
        if fun not in self._IDS:
            raise ValueError("fun must be 'EI', 'PI', 'EpsilonPI', 'MGFI' or None, not %r" % (fun,))
        y = np.asarray(getattr(model, "y", np.zeros((0, 0))), dtype=float)
        if y.ndim != 2 or y.shape[1] < 2:
            raise ValueError("modelled constraints need a model fitted on y (N, m) with m >= 2 columns (objective, constraints)")
        if y.shape[1] > _lib.MAX_TARGETS:
            raise ValueError("%d columns: at most %d targets (one objective and %d constraints)" % (y.shape[1], _lib.MAX_TARGETS, _lib.MAX_TARGETS - 1))
        n_con = y.shape[1] - 1
        lo = np.full(n_con, -np.inf) if lo is None else np.asarray(lo, dtype=float).ravel()
        hi = np.zeros(n_con) if hi is None else np.asarray(hi, dtype=float).ravel()
        if len(lo) != n_con or len(hi) != n_con:
            raise ValueError("lo and hi must hold one bound for each of the %d constraint columns of model.y" % n_con)
        if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(hi < lo):
            raise ValueError("constraint bounds must not be NaN, and hi >= lo")
        allowed = {"EI": (), "PI": (), "EpsilonPI": ("epsilon",), "MGFI": ("t",), None: ()}[fun]
        for name in par:
            if name not in allowed:
                raise TypeError("fun=%r takes no parameter %r" % (fun, name))
        self.model, self.fun, self.minimize = model, fun, bool(minimize)
        self.lo, self.hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
        self._par = 0.0
        if fun == "EpsilonPI":
            self._par = float(par.get("epsilon", 1e-10))
            assert self._par > 0
        elif fun == "MGFI":
            assert par.get("t", 1) > 0
            self._par = float(min(par.get("t", 1), 22.36))
        sign = 1.0 if self.minimize else -1.0
        feasible = np.all((y[:, 1:] >= self.lo) & (y[:, 1:] <= self.hi), axis=1)
        self.n_feasible = int(feasible.sum())
        if plugin is not None:
            self._plugin = sign * float(plugin)
        elif self.n_feasible:
            self._plugin = float(np.min(sign * y[feasible, 0]))
        else:
            self._plugin = None
        # without a feasible observation there is nothing to improve on: the probability of feasibility alone
        self.acq_id = self._IDS[fun] if self._plugin is not None else _lib.ACQ_NONE

    @property
    def plugin(self):
        return self._plugin

    @property
    def feasibility_only(self) -> bool:
        return self.acq_id == _lib.ACQ_NONE

    def acq_par(self) -> float:
        return 0.0 if self.feasibility_only else self._par

    def effective_plugin(self) -> float:
        return 0.0 if self._plugin is None else float(self._plugin)

    def sweep(self, k: int = 1, return_values: bool = False):
        """The sweep over the engine's current candidates: (best (k,), idx (k,)[, values (M,)])."""
        if getattr(self.model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        out = self.model.engine.sweep_constrained([(self.acq_id, self.acq_par())], self.effective_plugin(), self.minimize, self.lo, self.hi,
                                                  k=int(k), return_values=return_values)  # fmt: skip
        return tuple(a[0] for a in out)

    def __call__(self, X, return_dx: bool = False):
        if return_dx and not self.input_gradient:
            raise NotImplementedError("the feasibility-weighted criterion has no input gradient yet (the gradient of the probability of "
                                      "feasibility is not implemented): use 'sweep' or 'sweep-device[-lhs|-sobol]'")  # fmt: skip
        if getattr(self.model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        if self.input_gradient:
            rows = self.model._check_X(np.atleast_2d(np.asarray(X, dtype=float)))
            if return_dx or len(rows) <= 64:  # value and gradient in one device round trip (bogp_point_eval_constrained)
                eng = self.model.engine
                if not hasattr(eng, "point_eval_constrained"):
                    raise NotImplementedError("the model's engine has no point_eval_constrained: no input gradient of the "
                                              "feasibility-weighted criterion")  # fmt: skip
                vals, dx = eng.point_eval_constrained(rows, [(self.acq_id, self.acq_par())], self.effective_plugin(), self.minimize,
                                                      self.lo, self.hi)[:2]  # fmt: skip
                vals, dx = vals[:, 0], dx[:, 0, :]
                if not return_dx:
                    return vals
                return (vals.reshape(1), dx.reshape(1, -1)) if len(rows) == 1 else (vals.reshape(-1, 1), dx)
        self.model.engine.upload_candidates(self.model._check_X(np.atleast_2d(np.asarray(X, dtype=float))))
        return self.sweep(return_values=True)[2]


class ConstrainedEHVI:
    """Expected hypervolume improvement weighted by the probability that modelled constraints hold (`bogp_sweep_ehvi_constrained`): what
    the reference's multi-objective `tell` names and leaves open (`BaseMOBO.tell`, mobo.py:117-118).  `model` is a device
    GaussianProcess fitted on y (N, m + c), m = len(ref_point) >= 2, c >= 1: columns 0 .. m - 1 are the objectives, maximised as
    given (as `EHVI` takes them), column m + j the constraint feasible when lo[j] <= c_j(x) <= hi[j] (default (-inf, 0] each).  Per row

        value = EHVI(x on the objective columns) * prod_j P(lo_j <= c_j(x) <= hi_j),   and exactly +0.0 where that probability is 0

    over the cells of the FEASIBLE front: `pareto.hypercell_bounds(Y[feasible], ref_point)`, `Y` (N, m) defaulting to
    `model.y[:, :m]`, the feasible rows those whose constraint columns of `model.y` lie inside their bounds (`n_feasible` of them).  A
    feasible set with no row above the reference point has the one cell [ref, +inf); with no feasible row at all the criterion
    is the probability of feasibility alone (`feasibility_only`; Gelbart, Snoek, Adams 2014).  `cells=(lower, upper)` replaces the
    decomposition; such a criterion carries no front (`from_cells` is True and `pareto_Y` None -- `pareto_Y` is also None when no
    row is feasible, which `from_cells` tells apart).

    `criterion(X)` returns one value per row, shape (M,), in one device pass; `criterion.sweep(k, return_values)` sweeps the engine's
    current candidates as `EHVI.sweep` does.  By default there is no input gradient (`return_dx=True` raises); the sweep helpers
    serve it where they serve `EHVI`: alone in its sweep, on one rank.  Its one batch strategy is the Kriging believer of
    `optim.constrained_ehvi_believer_batch` (`bogp_sweep_believer_ehvi_constrained`); every other batch entry refuses it by name.

    `input_gradient=True` (an extension): `criterion(X, return_dx=True)` returns (values, dx) in the shapes
    `EHVI(input_gradient=True)` returns -- one row: ((1,), (1, d)); M rows: ((M, 1), (M, d)) -- through
    `bogp_point_eval_ehvi_constrained` (EHVI's gradient and the gradient of the probability of feasibility multiplied on the device;
    a feasibility-only criterion has the gradient of that probability), `criterion(X)` for at most 64 rows takes the same call, and
    `argmax_restart` serves "BFGS", "sweep-BFGS" and "sweep-device-BFGS" for it."""

    is_ehvi = True  # (the sweep helpers serve it through `.sweep()`, as they serve EHVI)
    is_constrained_ehvi = True  # ... and everything that does more than call `.sweep()` asks for this flag first
    is_constrained = False
    input_gradient = False
    minimize = False  # (the sweep helpers read it off every criterion)

    def __init__(self, model=None, ref_point=None, lo=None, hi=None, Y=None, cells=None, input_gradient: bool = False):
        if model is None:
            raise ValueError("model cannot be None")
        self.input_gradient = bool(input_gradient)
        if _forest.is_forest_model(model):
            raise NotImplementedError("constrained EHVI (bogp.ConstrainedEHVI) takes a multi-target Gaussian process: a forest model is not served")
        if ref_point is None:
            raise ValueError("ConstrainedEHVI needs a ref_point")
        if Y is not None and cells is not None:
            raise ValueError("ConstrainedEHVI takes at most one of Y= and cells=")
        self.model = model
        self.ref_point = np.asarray(ref_point, dtype=float).ravel()
        m = len(self.ref_point)
        y = np.asarray(getattr(model, "y", np.zeros((0, 0))), dtype=float)
        if m < 2 or y.ndim != 2 or y.shape[1] < m + 1:
            raise ValueError("constrained EHVI needs a ref_point of m >= 2 objectives and a model fitted on y (N, m + c) with c >= 1 constraint "
                             "columns: got ref_point %s and model.y %s" % (self.ref_point.shape, y.shape))  # fmt: skip
        if y.shape[1] > _lib.MAX_TARGETS:
            raise ValueError("model.y %s: at most %d targets (objectives and constraints together)" % (y.shape, _lib.MAX_TARGETS))
        n_con = y.shape[1] - m
        lo = np.full(n_con, -np.inf) if lo is None else np.asarray(lo, dtype=float).ravel()
        hi = np.zeros(n_con) if hi is None else np.asarray(hi, dtype=float).ravel()
        if len(lo) != n_con or len(hi) != n_con:
            raise ValueError("lo and hi must hold one bound for each of the %d constraint columns of model.y %s (ref_point %s)"
                             % (n_con, y.shape, self.ref_point.shape))  # fmt: skip
        if np.any(np.isnan(lo)) or np.any(np.isnan(hi)) or np.any(hi < lo):
            raise ValueError("constraint bounds must not be NaN, and hi >= lo")
        self.lo, self.hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
        feasible = np.all((y[:, m:] >= self.lo) & (y[:, m:] <= self.hi), axis=1)
        self.n_feasible = int(feasible.sum())
        self.pareto_Y = None
        self.from_cells = cells is not None  # (pareto_Y is None both for cells= and for "no feasible row": this tells them apart)
        if cells is not None:
            lower, upper = (np.atleast_2d(np.asarray(c, dtype=float)) for c in cells)
        else:
            Y = y[:, :m] if Y is None else np.atleast_2d(np.asarray(Y, dtype=float))
            if Y.shape != (len(y), m):
                raise ValueError("Y must hold the %d objectives of the model's %d rows, got %s" % (m, len(y), Y.shape))
            if self.n_feasible:
                from .pareto import hypercell_bounds, pareto_front

                self.pareto_Y = pareto_front(Y[feasible], self.ref_point)
                lower, upper = (np.atleast_2d(b) for b in hypercell_bounds(Y[feasible], self.ref_point))
            else:  # nothing to improve on yet: the probability of feasibility alone
                lower = upper = np.zeros((0, m))
        if lower.shape != upper.shape or lower.shape[1] != m:
            raise ValueError("cell bounds must be two C x %d arrays, got %s and %s" % (m, lower.shape, upper.shape))
        if len(lower) > _lib.MAX_EHVI_CELLS:
            raise ValueError("%d cells: at most %d per sweep" % (len(lower), _lib.MAX_EHVI_CELLS))
        self.cell_lower_bounds = np.ascontiguousarray(lower)
        self.cell_upper_bounds = np.ascontiguousarray(upper)

    @property
    def n_obj(self) -> int:
        return len(self.ref_point)

    @property
    def feasibility_only(self) -> bool:
        return len(self.cell_lower_bounds) == 0

    def effective_plugin(self) -> float:
        return 0.0

    def sweep(self, k: int = 1, return_values: bool = False):
        """The sweep over the engine's current candidates: (best (k,), idx (k,)[, values (M,)])."""
        if getattr(self.model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        return self.model.engine.sweep_ehvi_constrained(self.cell_lower_bounds, self.cell_upper_bounds, self.lo, self.hi, k=int(k),
                                                        return_values=return_values)  # fmt: skip

    def __call__(self, X, return_dx: bool = False):
        if return_dx and not self.input_gradient:
            raise NotImplementedError("constrained EHVI (bogp.ConstrainedEHVI) has no input gradient: use 'sweep' or "
                                      "'sweep-device[-lhs|-sobol]'")  # fmt: skip
        if getattr(self.model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        if self.input_gradient:
            rows = self.model._check_X(np.atleast_2d(np.asarray(X, dtype=float)))
            if return_dx or len(rows) <= 64:  # value and gradient in one device round trip (bogp_point_eval_ehvi_constrained)
                eng = self.model.engine
                if not hasattr(eng, "point_eval_ehvi_constrained"):
                    raise NotImplementedError("the model's engine has no point_eval_ehvi_constrained: no input gradient of constrained EHVI")
                vals, dx = eng.point_eval_ehvi_constrained(rows, self.cell_lower_bounds, self.cell_upper_bounds, self.lo, self.hi)[:2]
                if not return_dx:
                    return vals
                return (vals.reshape(1), dx.reshape(1, -1)) if len(rows) == 1 else (vals.reshape(-1, 1), dx)
        self.model.engine.upload_candidates(self.model._check_X(np.atleast_2d(np.asarray(X, dtype=float))))
        return self.sweep(return_values=True)[2]
