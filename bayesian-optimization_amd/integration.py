"""`bogp.install(bayes_optim)`: route the reference's own drivers through the device engine, without editing them.

What is re-pointed (INTEGRATION.md sections 3-4; all undone by the returned callable):

  bayes_optim.base.argmax_restart               -> routed_argmax_restart    (same signature; serves the sweep family,
                                                                             hands everything else to the original)
  bayes_optim.{base,bayes_opt,extension}.AcquisitionFunction -> a per-MODEL dispatching namespace (below)
  ParallelBO._batch_arg_max_acquisition         -> fused_batch_arg_max_acquisition
  BaseBO._create_acquisition                    -> constrained_create_acquisition -> forest_create_acquisition (this package's criteria
                                                   for a RandomForest model under "sweep" / "sweep-device"; the original otherwise,
                                                   "MIES" included; under install(expensive_constraints=True) and with stored
                                                   constraint values: bogp.Constrained)
  BaseBO.tell, BaseBO.update_model              -> constrained_tell, constrained_update_model (the originals unless
                                                   install(expensive_constraints=True) AND the tell carries h_vals / g_vals)
  MOBO._create_acquisition                      -> mobo_create_acquisition (this package's EHVI for a device model
                                                   under the sweep family; the reference's EHVI otherwise; with constraint
                                                   values stored under install(constrained_mobo=True): bogp.ConstrainedEHVI)
  MOBO._batch_arg_max_acquisition (inherited)   -> mobo_batch_arg_max_acquisition (raises as the inherited method unless
                                                   install(batch_strategy="believer"): optim.ehvi_believer_batch; with constraint
                                                   values stored, unless install(constrained_mobo_batches="believer"):
                                                   optim.constrained_ehvi_believer_batch)
  BaseMOBO.tell, BaseMOBO.update_model          -> refusing_mobo_tell, constrained_mobo_update_model (the originals unless
                                                   install(expensive_constraints=True) AND the tell carries h_vals / g_vals)
  bayes_optim.GaussianProcess, bayes_optim.surrogate.GaussianProcess, bayes_optim.extension.GaussianProcess
                                                -> a dispatching class that builds
                                                   `bogp.GaussianProcess` (so `bayes_optim.fmin` -- which resolves the
                                                   name at call time, `__init__.py:147-160` -- and `PCABO.update_model`,
                                                   extension.py:178-203, run on the device)

The contract of install() is that NOTHING the reference could do before stops working afterwards:

  * the acquisition namespace decides per model: `EI(model=<a bogp GaussianProcess>)` builds this package's criterion,
    any other model (the reference's CPU GaussianProcess, RandomForest, ...) gets the reference's own class
    (`acquisition_fun.py:107-310`); every other attribute of the namespace is the reference module's;
  * `routed_argmax_restart` serves optimizer = "sweep", "sweep-device[-lhs|-sobol]", "sweep-BFGS" (and a rerouted
    default "BFGS", see `install(reroute_bfgs=...)`) for this package's criteria; "BFGS" on a real space, constraints
    under BFGS / "OnePlusOne_Cholesky_CMA" / "MIES", non-real spaces and criteria that are not this package's all go
    to the saved original (`acquisition/optim/__init__.py:55-153`) -- our criteria are plain callables to it;
  * PCA-BO's penalising wrapper (`functools.partial(penalized_acquisition, ...)`, extension.py:121-133) around one of this
    package's criteria is served under the sweep family by the LIFTED sweep (`optim.unwrap_lift`); under
    "BFGS" the reference's loop and its `penalized_acquisition` run unchanged on this package's one-point criterion;
  * the GaussianProcess name builds the reference's own class for configurations the device does not serve
    (`optimizer="CMA"`, a callable correlation it does not know), with a warning.

Row f1: the reference maximises its q criteria one after the other (`bayes_opt.py:100-115`: q calls of
`_argmax_restart`, i.e. q host samplings, q uploads and q posterior passes although the criteria differ only in
t / alpha), de-duplicates afterwards (`BO.pre_eval_check`, `:27-55`) and pads what is left with random points
(`base.py:282-289`).  The fused method draws the q parameters with the reference's own sampler IN THE SAME ORDER (so
the global np.random stream advances exactly as in the reference), then makes ONE call of `optim.batch_argmax`: one
candidate design, one posterior pass, q criteria, top-k per criterion; a criterion whose best candidate is already
taken by an earlier criterion, or `np.isclose` to an evaluated point, falls back through its own top-k.  With any
other inner optimiser ("BFGS", ...) the reference's method runs unchanged.
"""
from __future__ import annotations

import functools
import types
import warnings
from copy import copy

import numpy as np

from . import acquisition, optim
from . import forest as _forest
from .surrogate import GaussianProcess as _DeviceGP

_SWEEPS = ("sweep",) + tuple(optim.DEVICE_DESIGNS)
_OURS = _SWEEPS + ("sweep-BFGS", "sweep-device-BFGS")  # inner optimisers only this package knows


def is_device_model(model) -> bool:
    """True for a surrogate whose posterior lives in a libbogp engine (this package's GaussianProcess or a subclass)."""
    return isinstance(model, _DeviceGP)


def _history_of(bo):
    """Evaluated points as a float (n, dim) array in the search space's variable order (what pre_eval_check compares
    with np.isclose, bayes_opt.py:41-48), or None before the first tell()."""
    data = getattr(bo, "data", None)
    if data is None or len(data) == 0:
        return None
    return np.asarray(np.asarray(data)[:, : bo.dim], dtype=float)


def fused_batch_arg_max_acquisition(self, n_point: int, return_dx: bool, fixed=None):
    """Drop-in body for `ParallelBO._batch_arg_max_acquisition` (bayes_opt.py:100-115): same arguments, same
    `(candidates, values)` return (two q-tuples)."""
    optimizer, budget = _effective(getattr(self, "_optimizer", None), None)
    kw = getattr(getattr(self, "_argmax_restart", None), "keywords", None) or {}  # bound by BaseBO.__set_argmax (base.py:231-243)
    if optimizer not in _SWEEPS or not is_device_model(getattr(self, "model", None)) or not optim.is_continuous(kw.get("search_space")):
        return _ORIGINAL["batch"](self, n_point, return_dx, fixed)
    if optimizer in optim.DEVICE_DESIGNS and (kw.get("h") is not None or kw.get("g") is not None or fixed):
        return _ORIGINAL["batch"](self, n_point, return_dx, fixed)  # one criterion at a time through routed_argmax_restart
    wrapped = []
    for _ in range(n_point):  # bayes_opt.py:101-106 verbatim in effect: same draws, same order
        _par = self._sampler(self._acquisition_par)
        _acquisition_par = copy(self._acquisition_par)
        _acquisition_par.update({self._par_name: _par})
        wrapped.append(self._create_acquisition(par=_acquisition_par, return_dx=return_dx, fixed=fixed))
    crits, masks, values = [], None, None
    for w in wrapped:
        c, m, v = optim.unwrap_criterion(w)
        if c is None:  # not one of this package's criteria: nothing to fuse
            return tuple(zip(*[list(self._argmax_restart(w, logger=self.logger)) for w in wrapped]))
        crits.append(c)
        masks, values = m, v
    design = optim.DEVICE_DESIGNS.get(optimizer)
    if (_CONSTRAINTS.get("batches") == "believer" and all(optim.is_constrained(c) for c in crits) and masks is None and not fixed
            and kw.get("h") is None and kw.get("g") is None):  # fmt: skip
        # install(constraint_batches="believer"): the q feasibility-weighted criteria condition each other (every other case: below)
        xs, fs = optim.constrained_believer_batch(crits, kw["search_space"], int(budget or kw["eval_budget"]), design=design)
        return tuple(xs), tuple(fs)
    if (_CONSTRAINTS.get("batches") == "thompson" and all(optim.is_constrained(c) for c in crits) and masks is None and not fixed
            and kw.get("h") is None and kw.get("g") is None):  # fmt: skip
        # install(constraint_thompson=True): one joint draw of objective and constraints per point; the criteria supply model, bounds
        # and direction only
        xs, fs = optim.constrained_thompson_batch(crits[0], kw["search_space"], int(budget or kw["eval_budget"]), n_point, design=design,
                                                  history=_history_of(self))  # fmt: skip
        return tuple(xs), tuple(fs)
    k = int(min(32, n_point + 8))  # fall-backs: at most n_point - 1 taken by earlier criteria + a few history hits
    xs, fs = optim.batch_argmax(crits, kw["search_space"], int(budget or kw["eval_budget"]), history=_history_of(self), k=k,
                                design=design, masks=masks, values=values, h=kw.get("h"), g=kw.get("g"), **_strategy_of(masks, kw, crits))  # fmt: skip
    return tuple(xs), tuple(fs)


def _strategy_of(masks, kw, crits=()) -> dict:
    """The `strategy` keyword of the fused step's `batch_argmax` call: none under the default, and none for what the believer does
    not serve -- fixed variables, constraints and modelled constraints (`bogp.Constrained`) stay on the top-k strategy, which serves them."""
    if _BATCH.get("strategy", "topk") == "topk" or masks is not None or kw.get("h") is not None or kw.get("g") is not None:
        return {}
    if any(optim.is_constrained(c) for c in crits):
        return {}
    return {"strategy": _BATCH["strategy"]}


_ORIGINAL: dict = {}
_REROUTE: dict = {}
_BATCH: dict = {}  # install(batch_strategy=...): how the fused ParallelBO step makes its q points differ ("topk" when empty)
_EHVI: dict = {}  # install(ehvi_gradient=True): MOBO's polish optimisers run on bogp.EHVI(input_gradient=True) (empty: the original)
_SURROGATE_DEFAULTS: dict = {}  # keyword defaults install() gives the device GaussianProcess (e.g. restart_batch)
_CONSTRAINTS: dict = {}  # install(expensive_constraints=True): {"tol": equality_tol}; empty: tell() drops h_vals / g_vals as the reference does


def _effective(optimizer, eval_budget):
    """(optimizer, eval_budget) after `install(reroute_bfgs=...)`: the reference's DEFAULT inner optimiser for a GP on a real
    space is "BFGS" with a budget of 100 dim point evaluations (base.py:200-214, default_AQ_max_FEs) -- thousands of one-point
    device round trips per ask().  With a reroute installed those calls become one sweep of `sweep_budget` candidates."""
    if optimizer == "BFGS" and _REROUTE:
        return _REROUTE["optimizer"], _REROUTE["budget"]
    return optimizer, eval_budget


def mobo_create_acquisition(self, fixed=None, **kwargv):
    """Drop-in body for `bayes_optim.mobo.MOBO._create_acquisition` (mobo.py:177-186): with a device model, an inner
    optimiser of the sweep family ("sweep", "sweep-device[-lhs|-sobol]") and a continuous space the criterion is this
    package's `EHVI` (float64, cells from `bogp.pareto`), wrapped exactly as the original wraps the reference's; so it is with
    a forest model (`is_forest_model`: this package's `RandomForest` or the reference's) under "sweep" / "sweep-device" on any
    space a forest sweep serves.  Under `install(ehvi_gradient=True)` a device model on a continuous space is served under "BFGS",
    "sweep-BFGS" and "sweep-device-BFGS" as well: the criterion is built with `input_gradient=True` and `return_dx` is bound as
    `BO._create_acquisition` binds it (base.py:463, 489-494: true for "BFGS" only), so that the reference's `argmax_restart`
    accepts the wrapper.  Every other configuration -- "MIES", the reference's default on mixed spaces, CMA, BFGS without that
    switch -- runs the original unchanged."""
    if _CONSTRAINTS.get("mobo") and getattr(self, "_bogp_constraints", None) is not None:
        # install(expensive_constraints=True, constrained_mobo=True) and a tell() that carried h_vals / g_vals: EHVI of the feasible front
        # times the probability of feasibility, or an error -- never the plain criterion, which would drop the constraints
        optimizer, _ = _effective(getattr(self, "_optimizer", None), None)
        if not is_device_model(getattr(self, "model", None)) or not optim.is_continuous(getattr(self, "search_space", None)):
            raise NotImplementedError("expensive constraints of a multi-objective run (bogp.ConstrainedEHVI) take a device GaussianProcess on "
                                      "a continuous search space; the constraint values are not dropped silently")  # fmt: skip
        lo, hi = _constraint_bounds(self)
        if _CONSTRAINTS.get("mobo_gradient") and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
            # install(constrained_mobo_gradient=True): the criterion with its input gradient; return_dx bound as the ehvi_gradient branch binds it
            criterion = acquisition.ConstrainedEHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), lo=lo, hi=hi,
                                                    input_gradient=True)  # fmt: skip
            return_dx = optimizer == "BFGS"
            return _ORIGINAL["partial_argument"](functools.partial(criterion, return_dx=return_dx), self.search_space.var_name, fixed,
                                                 reduce_output=return_dx)  # fmt: skip
        if optimizer not in _SWEEPS:
            raise NotImplementedError("optimizer=%r under expensive constraints of a multi-objective run: constrained EHVI "
                                      "(bogp.ConstrainedEHVI) is served by the sweep family only %s; the constraint values are not dropped "
                                      "silently" % (optimizer, _SWEEPS))  # fmt: skip
        criterion = acquisition.ConstrainedEHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), lo=lo, hi=hi)
        return _ORIGINAL["partial_argument"](functools.partial(criterion), self.search_space.var_name, fixed, reduce_output=False)
    if getattr(self, "_optimizer", None) in ("sweep", "sweep-device") and _forest.is_forest_model(getattr(self, "model", None)):
        # a RandomForest fitted on y (N, n_obj) (this package's or the reference's), on any space a forest sweep serves: the
        # forest walk and EHVI are one device pass; what a forest sweep does not take is refused by optim.argmax_restart by name
        criterion = acquisition.EHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), Y=np.asarray(self.y, dtype=float))
        return _ORIGINAL["partial_argument"](functools.partial(criterion), self.search_space.var_name, fixed, reduce_output=False)
    optimizer, _ = _effective(getattr(self, "_optimizer", None), None)
    served = is_device_model(getattr(self, "model", None)) and optim.is_continuous(getattr(self, "search_space", None))
    if served and _EHVI.get("gradient") and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        criterion = acquisition.EHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), Y=np.asarray(self.y, dtype=float),
                                     input_gradient=True)  # fmt: skip
        return_dx = optimizer == "BFGS"
        return _ORIGINAL["partial_argument"](functools.partial(criterion, return_dx=return_dx), self.search_space.var_name, fixed,
                                             reduce_output=return_dx)  # fmt: skip
    if optimizer not in _SWEEPS or not served:
        return _ORIGINAL["mobo"](self, fixed=fixed, **kwargv)
    criterion = acquisition.EHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), Y=np.asarray(self.y, dtype=float))
    return _ORIGINAL["partial_argument"](functools.partial(criterion), self.search_space.var_name, fixed, reduce_output=False)


def mobo_batch_arg_max_acquisition(self, n_point: int, return_dx: bool, fixed=None):
    """`MOBO._batch_arg_max_acquisition` under `install(batch_strategy="believer")`: the Kriging believer the reference's MOBO names
    and leaves open (mobo.py:168-178; the inherited BaseBO method raises NotImplementedError, base.py:496-497).  Taken for a device
    GP, an inner optimiser of the sweep family, a continuous space, nothing fixed and no constraints: `optim.ehvi_believer_batch` on
    the criterion `mobo_create_acquisition` builds.  Everything else -- the default `install()` above all -- calls the inherited
    method, which raises as it does without this package.
    After a tell() that carried constraint values (`install(constrained_mobo=True)`) the batch is
    `optim.constrained_ehvi_believer_batch` on `bogp.ConstrainedEHVI` under `install(constrained_mobo_batches="believer")` and the
    same conditions (no cheap h / g); without that switch, and in every other configuration, it raises NotImplementedError."""
    optimizer, budget = _effective(getattr(self, "_optimizer", None), None)
    kw = getattr(getattr(self, "_argmax_restart", None), "keywords", None) or {}
    if getattr(self, "_bogp_constraints", None) is not None:
        # install(..., constrained_mobo_batches="believer"): the believer under constrained EHVI, where everything it needs holds;
        # every other configuration -- the default above all -- raises instead of dropping the constraints
        if (_CONSTRAINTS.get("mobo_batches") == "believer" and _CONSTRAINTS.get("mobo") and not fixed and optimizer in _SWEEPS
                and is_device_model(getattr(self, "model", None)) and optim.is_continuous(kw.get("search_space"))
                and kw.get("h") is None and kw.get("g") is None):  # fmt: skip
            lo, hi = _constraint_bounds(self)
            criterion = acquisition.ConstrainedEHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), lo=lo, hi=hi)
            xs, fs = optim.constrained_ehvi_believer_batch(criterion, kw["search_space"], int(budget or kw["eval_budget"]), int(n_point),
                                                           design=optim.DEVICE_DESIGNS.get(optimizer))  # fmt: skip
            return tuple(xs), tuple(fs)
        raise NotImplementedError("MOBO(n_point=q) under expensive constraints: constrained EHVI (bogp.ConstrainedEHVI) has no batch "
                                  "strategy; ask for one point at a time")  # fmt: skip
    inherited = super(_ORIGINAL["mobo_cls"], self)._batch_arg_max_acquisition
    if (_BATCH.get("strategy") != "believer" or fixed or optimizer not in _SWEEPS or not is_device_model(getattr(self, "model", None))
            or not optim.is_continuous(kw.get("search_space")) or kw.get("h") is not None or kw.get("g") is not None):  # fmt: skip
        return inherited(n_point, return_dx, fixed)
    criterion = acquisition.EHVI(model=self.model, ref_point=np.asarray(self.ref_point, dtype=float), Y=np.asarray(self.y, dtype=float))
    xs, fs = optim.ehvi_believer_batch(criterion, kw["search_space"], int(budget or kw["eval_budget"]), int(n_point),
                                       design=optim.DEVICE_DESIGNS.get(optimizer))  # fmt: skip
    return tuple(xs), tuple(fs)


def forest_create_acquisition(self, fun=None, par=None, return_dx=False, fixed=None):
    """Drop-in body for `BaseBO._create_acquisition` (base.py:482-494): a `RandomForest` model (this package's or the reference's)
    under "sweep" / "sweep-device" gets this package's criterion, which evaluates the packed forest on the device, wrapped exactly as
    the original wraps the reference's.  Every other configuration -- "MIES" above all, the reference's default on mixed spaces --
    runs the original unchanged."""
    optimizer = getattr(self, "_optimizer", None)
    name = fun if fun is not None else getattr(self, "_acquisition_fun", None)
    if optimizer not in ("sweep", "sweep-device") or not _forest.is_forest_model(getattr(self, "model", None)) or not hasattr(acquisition, str(name)):
        return _ORIGINAL["create"](self, fun=fun, par=par, return_dx=return_dx, fixed=fixed)
    par = par if par is not None else copy(self._acquisition_par)
    par.update({"model": self.model, "minimize": self.minimize})
    criterion = getattr(acquisition, name)(**par)
    return _ORIGINAL["base_partial_argument"](func=functools.partial(criterion, return_dx=return_dx), var_name=self.search_space.var_name,
                                              fixed=fixed, reduce_output=return_dx)  # fmt: skip


# ----------------------------------------------------------------------------------------------------------------------
# install(expensive_constraints=True): the h_vals / g_vals of tell() become columns of the surrogate
# ----------------------------------------------------------------------------------------------------------------------
_CONSTRAINED_FUNS = ("EI", "PI", "EpsilonPI", "MGFI")


def _constraint_columns(vals, n, what):
    """`vals` of a tell() of n points as an (n, k) float array: a flat list of n numbers is one constraint."""
    a = np.asarray(vals, dtype=float)
    if a.ndim == 1 and len(a) == n:
        return a.reshape(n, 1)
    if a.ndim == 2 and a.shape[0] == n and a.shape[1] >= 1:
        return a
    raise ValueError("%s must hold one value, or one list of values, for each of the %d points told (got shape %s)" % (what, n, a.shape))


def constrained_tell(self, X, func_vals, h_vals=None, g_vals=None, index=None, warm_start=False):
    """`BaseBO.tell` under `install(expensive_constraints=True)` (the reference drops `h_vals` / `g_vals`, base.py:328): for a `BO` /
    `ParallelBO` (or a subclass) with a device GP the values are kept, row for row with `self.data`, in `self._bogp_constraints` (the
    g columns first, then the h columns), and the original `tell` -- whose `update_model` then fits objective and constraints
    together -- runs.  ValueError: values missing after a tell() that had them, or given after one that had none; a changed number
    of constraints; a non-finite value.  Another model (a forest) is refused by name."""
    given = h_vals is not None or g_vals is not None
    if not _CONSTRAINTS or (not given and getattr(self, "_bogp_constraints", None) is None):
        return _ORIGINAL["tell"](self, X, func_vals, h_vals=h_vals, g_vals=g_vals, index=index, warm_start=warm_start)
    if not is_device_model(getattr(self, "model", None)):
        raise NotImplementedError("expensive constraints (h_vals / g_vals) are modelled by a device GaussianProcess: the %s model of this "
                                  "driver is not served" % type(getattr(self, "model", None)).__name__)  # fmt: skip
    if getattr(self, "n_obj", 1) != 1:
        raise NotImplementedError("expensive constraints (h_vals / g_vals) are served for single-objective drivers (BO, ParallelBO), not for %d objectives" % self.n_obj)
    return _tell_storing_constraints(self, _ORIGINAL["tell"], X, func_vals, h_vals, g_vals, index, warm_start)


def _tell_storing_constraints(self, original_tell, X, func_vals, h_vals, g_vals, index, warm_start):
    """What `constrained_tell` and the multi-objective tell share: the rules and error cases of storing the constraint values of a
    tell() row for row with `self.data`, around `original_tell` (a row is kept where `post_eval_check` keeps it: all of its
    fitness values finite)."""
    given = h_vals is not None or g_vals is not None
    stored = getattr(self, "_bogp_constraints", None)
    if not given:
        raise ValueError("this tell() carries no h_vals / g_vals, but earlier ones did: every point needs its constraint values")
    if stored is None and hasattr(self, "data") and len(self.data) > 0:
        raise ValueError("this tell() carries h_vals / g_vals, but %d points were told without them: every point needs its constraint values" % len(self.data))
    n = len(X)
    g = np.zeros((n, 0)) if g_vals is None else _constraint_columns(g_vals, n, "g_vals")
    h = np.zeros((n, 0)) if h_vals is None else _constraint_columns(h_vals, n, "h_vals")
    counts = (g.shape[1], h.shape[1])
    if stored is not None and counts != self._bogp_constraint_counts:
        raise ValueError("this tell() carries %d g and %d h values a point, earlier ones %d and %d" % (counts + tuple(self._bogp_constraint_counts)))
    fitness = np.asarray(func_vals, dtype=float).reshape(n, -1)
    keep = ~np.any(np.isnan(fitness) | np.isinf(fitness), axis=1)  # the rows post_eval_check keeps (base.py:413-421)
    rows = np.hstack([g, h])[keep]
    if not np.all(np.isfinite(rows)):
        raise ValueError("h_vals / g_vals hold a non-finite value: a modelled constraint needs a number for every evaluated point")
    before = (stored, getattr(self, "_bogp_constraint_counts", None))
    self._bogp_constraints = rows if stored is None else np.vstack([stored, rows])
    self._bogp_constraint_counts = counts
    try:
        return original_tell(self, X, func_vals, h_vals=h_vals, g_vals=g_vals, index=index, warm_start=warm_start)
    except BaseException:
        if not hasattr(self, "data") or len(self.data) != len(self._bogp_constraints):  # the points did not arrive: nor do their values
            self._bogp_constraints, self._bogp_constraint_counts = before
        raise


def refusing_mobo_tell(self, X, func_vals, h_vals=None, g_vals=None, index=None, warm_start=False):
    """`BaseMOBO.tell` under `install(expensive_constraints=True)`: constraint values are refused by name, everything else is the
    original.  With `constrained_mobo=True` as well they are kept instead (the TODO of mobo.py:117-118): row for row with `self.data`
    in `self._bogp_constraints`, by `constrained_tell`'s rules and with its error cases, for a device GP; `constrained_mobo_update_model`
    then fits objectives and constraints together."""
    given = h_vals is not None or g_vals is not None
    if _CONSTRAINTS.get("mobo") and (given or getattr(self, "_bogp_constraints", None) is not None):
        if not is_device_model(getattr(self, "model", None)):
            raise NotImplementedError("expensive constraints (h_vals / g_vals) are modelled by a device GaussianProcess: the %s model of this "
                                      "driver is not served" % type(getattr(self, "model", None)).__name__)  # fmt: skip
        return _tell_storing_constraints(self, _ORIGINAL["mobo_tell"], X, func_vals, h_vals, g_vals, index, warm_start)
    if _CONSTRAINTS and given:
        raise NotImplementedError("expensive constraints (h_vals / g_vals) are served for single-objective drivers (BO, ParallelBO), "
                                  "not for the multi-objective MOBO")  # fmt: skip
    return _ORIGINAL["mobo_tell"](self, X, func_vals, h_vals=h_vals, g_vals=g_vals, index=index, warm_start=warm_start)


def constrained_update_model(self):
    """`BaseBO.update_model` (base.py:423-446) with stored constraint values: column 0 is the reference's standardised fitness (fmin,
    fmax, frange as there), each constraint column is divided by its standard deviation (left as is where that is 0) and never
    shifted -- its boundary stays at 0, and the fixed trend beta = 0 is the prior "undecided" --, and the model is fitted on
    Y (N, 1 + n_g + n_h).  Without stored values: the original."""
    C = getattr(self, "_bogp_constraints", None)
    if not _CONSTRAINTS or C is None:
        return _ORIGINAL["update_model"](self)
    rbase = _ORIGINAL["mods"][1]
    data = self.data
    fitness = np.asarray(data.fitness, dtype=float)
    if len(C) != len(fitness):
        raise ValueError("%d points hold constraint values, %d are stored in data" % (len(C), len(fitness)))
    _std = np.std(fitness)
    if len(fitness) > 5 and np.isclose(_std, 0):
        raise rbase.FlatFitnessError()
    fitness_ = fitness if np.isclose(_std, 0) else (fitness - np.mean(fitness)) / np.std(fitness)
    self.fmin, self.fmax = np.min(fitness_), np.max(fitness_)
    self.frange = self.fmax - self.fmin
    std = np.std(C, axis=0)
    self._bogp_constraint_scale = np.where(np.isclose(std, 0), 1.0, std)
    Y = np.column_stack([fitness_.reshape(-1, 1), C / self._bogp_constraint_scale])
    self.model.fit(data, Y)
    fitness_hat = np.asarray(self.model.predict(data)).reshape(len(fitness_), -1)[:, 0]
    r2 = rbase.r2_score(fitness_, fitness_hat)
    MAPE = rbase.mean_absolute_percentage_error(fitness_, fitness_hat)
    self.logger.info(f"model r2: {r2}, MAPE: {MAPE}")


def constrained_mobo_update_model(self):
    """`BaseMOBO.update_model` (mobo.py:155-165) with stored constraint values: the model is fitted on
    column_stack([self.y, C / scale]) -- the objectives as the reference transforms them (min-max scaled, maximised), each constraint
    column divided by its standard deviation (1 where that is 0) and never shifted, as `constrained_update_model` scales them -- and
    r2 / MSE are logged for the objective columns only.  Without stored values: the original."""
    C = getattr(self, "_bogp_constraints", None)
    if not _CONSTRAINTS.get("mobo") or C is None:
        return _ORIGINAL["mobo_update_model"](self)
    rmobo = _ORIGINAL["mobo_mod"]
    X, y = self.data, np.asarray(self.y, dtype=float)
    if len(C) != len(y):
        raise ValueError("%d points hold constraint values, %d are stored in data" % (len(C), len(y)))
    std = np.std(C, axis=0)
    self._bogp_constraint_scale = np.where(np.isclose(std, 0), 1.0, std)
    self.model.fit(X, np.column_stack([y, C / self._bogp_constraint_scale]))
    y_ = np.asarray(self.model.predict(X)).reshape(len(y), -1)[:, : y.shape[1]]
    r2 = rmobo.r2_score(y, y_, multioutput="raw_values")
    MSE = rmobo.mean_squared_error(y, y_, multioutput="raw_values")
    for i in range(self.n_obj):
        self.logger.info(f"model of f{i + 1} r2: {r2[i]}, MSE: {MSE[i]}")


def _constraint_bounds(self):
    """(lo, hi) of the stored constraint columns as the model sees them: (-inf, 0] for the g columns, [-tol, tol] / std for the h columns
    (tol = `install(equality_tol=)`)."""
    n_g, _ = self._bogp_constraint_counts
    tol = _CONSTRAINTS["tol"] / np.asarray(self._bogp_constraint_scale, dtype=float)[n_g:]
    return np.r_[np.full(n_g, -np.inf), -tol], np.r_[np.zeros(n_g), tol]


def constrained_create_acquisition(self, fun=None, par=None, return_dx=False, fixed=None):
    """`BaseBO._create_acquisition` in front of `forest_create_acquisition`: with stored constraint values the criterion is
    `bogp.Constrained` -- (-inf, 0] for the g columns, [-tol, tol] / std for the h columns (tol = `install(equality_tol=)`), the plugin
    the best FEASIBLE observation instead of the fmin / fmax `BO._create_acquisition` passes.  UCB raises ValueError; an inner optimiser
    outside the sweep family raises NotImplementedError instead of dropping the constraints -- except, under
    `install(constraint_gradient=True)`, "BFGS", "sweep-BFGS" and "sweep-device-BFGS", which get the criterion with `input_gradient=True`."""
    C = getattr(self, "_bogp_constraints", None)
    if not _CONSTRAINTS or C is None or not is_device_model(getattr(self, "model", None)):
        return forest_create_acquisition(self, fun=fun, par=par, return_dx=return_dx, fixed=fixed)
    name = fun if fun is not None else getattr(self, "_acquisition_fun", None)
    if name not in _CONSTRAINED_FUNS:
        raise ValueError("acquisition_fun=%r under expensive constraints: the feasibility-weighted criterion takes EI, PI, EpsilonPI or "
                         "MGFI (UCB changes sign, so its product with a probability orders nothing)" % (name,))  # fmt: skip
    optimizer, _ = _effective(getattr(self, "_optimizer", None), None)
    gradient = bool(_CONSTRAINTS.get("gradient")) and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS")
    if optimizer not in _SWEEPS and not gradient:
        raise NotImplementedError("optimizer=%r under expensive constraints: the feasibility-weighted criterion is served by the sweep "
                                  "family only %s; the constraint values are not dropped silently" % (optimizer, _SWEEPS))  # fmt: skip
    par = dict(par if par is not None else self._acquisition_par)
    for k in ("plugin", "model", "minimize"):
        par.pop(k, None)
    lo, hi = _constraint_bounds(self)
    criterion = acquisition.Constrained(model=self.model, fun=name, minimize=self.minimize, lo=lo, hi=hi, input_gradient=gradient, **par)
    return _ORIGINAL["base_partial_argument"](func=functools.partial(criterion, return_dx=return_dx), var_name=self.search_space.var_name,
                                              fixed=fixed, reduce_output=return_dx)  # fmt: skip


def feasible_xopt(bo):
    """The best observed point of `bo` whose stored constraint values are all feasible (g <= 0, |h| <= `install(equality_tol=)`), as a row
    of `bo.data`, or None when there is none (or nothing stored).  The reference's `xopt` ignores constraint values and is untouched."""
    C = getattr(bo, "_bogp_constraints", None)
    if C is None or not hasattr(bo, "data") or len(C) != len(bo.data):
        return None
    n_g, _ = bo._bogp_constraint_counts
    tol = _CONSTRAINTS.get("tol", 0.1)
    ok = np.all(C[:, :n_g] <= 0, axis=1) & np.all(np.abs(C[:, n_g:]) <= tol, axis=1)
    if not ok.any():
        return None
    f = np.asarray(bo.data.fitness, dtype=float)
    rows = np.flatnonzero(ok)
    return bo.data[int(rows[np.argmin(f[rows]) if bo.minimize else np.argmax(f[rows])])]


def feasible_front(bo):
    """The non-dominated rows of `bo.data` among those whose stored constraint values are all feasible (g <= 0, |h| <=
    `install(equality_tol=)`) -- the multi-objective counterpart of `feasible_xopt` --, an empty selection when no row is feasible, or
    None when nothing is stored.  The reference's `xopt` ignores constraint values and is untouched."""
    C = getattr(bo, "_bogp_constraints", None)
    if C is None or not hasattr(bo, "data") or len(C) != len(bo.data):
        return None
    from .pareto import is_non_dominated

    n_g, _ = bo._bogp_constraint_counts
    tol = _CONSTRAINTS.get("tol", 0.1)
    rows = np.flatnonzero(np.all(C[:, :n_g] <= 0, axis=1) & np.all(np.abs(C[:, n_g:]) <= tol, axis=1))
    if len(rows):
        rows = rows[is_non_dominated(np.asarray(bo.y, dtype=float)[rows])]
    mask = np.zeros(len(C), dtype=bool)
    mask[rows] = True
    return bo.data[mask, :]  # (selected as the reference's xopt selects, mobo.py:56-57)


def routed_argmax_restart(obj_func, search_space, h=None, g=None, eval_budget=100, n_restart=10, wait_iter=3,
                          optimizer="BFGS", logger=None):
    """`bayes_optim.base.argmax_restart` after `install()`.

    This package's inner optimisers (the sweep family) are served by `optim.argmax_restart` when `obj_func` wraps one
    of this package's criteria over a continuous space; every other call -- the reference's "BFGS" /
    "OnePlusOne_Cholesky_CMA" / "MIES", constraints under them, mixed / integer / discrete spaces, foreign criteria or
    models -- goes to the reference's own function with the arguments untouched (optim/__init__.py:55-153), for which a
    bogp criterion is an ordinary callable.  A reroute (`install(reroute_bfgs=...)`) only ever applies to an
    unconstrained "BFGS" call on a continuous space whose criterion is this package's."""
    original = _ORIGINAL["argmax"]
    lifted = optim._lift_wrapper_parts(obj_func)
    if optimizer in _OURS and lifted is not None and optim.unwrap_criterion(lifted[0])[0] is not None and optim.is_continuous(search_space):
        # PCA-BO's penalising wrapper around one of this package's criteria: the lifted sweep over the reduced box
        return optim.argmax_restart(obj_func, search_space, h=h, g=g, eval_budget=eval_budget, n_restart=n_restart,
                                    wait_iter=wait_iter, optimizer=optimizer, logger=logger)  # fmt: skip
    crit = optim.unwrap_criterion(obj_func)[0]
    if crit is not None and optimizer in _OURS and _forest.is_forest_model(getattr(crit, "model", None)):
        # this package's criterion on a forest model (forest_create_acquisition): any space of Real / Integer / Ordinal / Discrete /
        # Subset / Bool variables; what a forest sweep does not take is refused there by name
        return optim.argmax_restart(obj_func, search_space, h=h, g=g, eval_budget=eval_budget, n_restart=n_restart,
                                    wait_iter=wait_iter, optimizer=optimizer, logger=logger)  # fmt: skip
    mine = crit is not None and optim.is_continuous(search_space)
    opt2, budget2 = optimizer, eval_budget
    if mine and optimizer == "BFGS" and h is None and g is None:
        opt2, budget2 = _effective(optimizer, eval_budget)
    if mine and opt2 in _OURS:
        return optim.argmax_restart(obj_func, search_space, h=h, g=g, eval_budget=budget2, n_restart=n_restart,
                                    wait_iter=wait_iter, optimizer=opt2, logger=logger)  # fmt: skip
    if mine and optimizer == "BFGS" and optim.is_constrained(crit) and getattr(crit, "input_gradient", False):
        # Constrained(input_gradient=True): the reference-style loop on bogp_point_eval_constrained; cheap callables h / g are refused by name
        return optim.argmax_restart(obj_func, search_space, h=h, g=g, eval_budget=eval_budget, n_restart=n_restart,
                                    wait_iter=wait_iter, optimizer=optimizer, logger=logger)  # fmt: skip
    if optimizer in _OURS:  # asked for by name, but not servable: say why instead of a KeyError deep in the reference
        raise TypeError("optimizer=%r needs one of this package's criteria (a bogp.GaussianProcess as model=) on a "
                        "continuous search space" % optimizer)  # fmt: skip
    return original(obj_func, search_space, h=h, g=g, eval_budget=eval_budget, n_restart=n_restart, wait_iter=wait_iter,
                    optimizer=optimizer, logger=logger)  # fmt: skip


# ----------------------------------------------------------------------------------------------------------------------
# per-model dispatch: one name, two implementations
# ----------------------------------------------------------------------------------------------------------------------
class _Dispatch(type):
    """Metaclass of the names install() re-points: calling the class builds `_device` or `_host` (decided by
    `_pick(args, kwargs)`), `isinstance` / `issubclass` accept instances of either, attribute look-ups that the
    dispatching class does not define fall through to the device class and then the host class (so that
    `hasattr(cls, "plugin")`, bayes_opt.py:21-23, answers as both originals do)."""

    def __call__(cls, *args, **kwargs):
        if "_pick" not in cls.__dict__:
            # a user's `class My(bayes_optim.GaussianProcess)` inherits this metaclass: its overrides were written against the
            # reference's class, so it is realised on the HOST class with the subclass's own namespace on top (never silently
            # replaced by a plain device object); see _realise
            return _realise(cls)(*args, **kwargs)
        return cls._pick(args, kwargs)(*args, **kwargs)

    def __instancecheck__(cls, obj):
        if "_pick" not in cls.__dict__:  # a user's subclass: its instances are instances of its realisation (and of the realisations of ITS subclasses)
            return isinstance(obj, _realise(cls))
        return isinstance(obj, tuple(t for t in (cls._device, cls._host) if t is not None))

    def __subclasscheck__(cls, sub):
        if "_pick" not in cls.__dict__:
            return sub is cls or (isinstance(sub, _Dispatch) and cls in sub.__mro__) or issubclass(sub, _realise(cls))
        return sub is cls or issubclass(sub, tuple(t for t in (cls._device, cls._host) if t is not None))

    def __getattr__(cls, name):
        if name.startswith("__") and name.endswith("__"):
            raise AttributeError(name)
        for t in (cls.__dict__.get("_device"), cls.__dict__.get("_host")):
            if t is not None and hasattr(t, name):
                return getattr(t, name)
        raise AttributeError("%s has no attribute %r" % (cls.__name__, name))


_REALISED = {}


def _rebind_class_cell(v, cell):
    """`v` with the `__class__` cell of zero-argument super() re-pointed at `cell` (functions, and the functions inside static / class
    methods and properties); anything else unchanged."""
    if isinstance(v, types.FunctionType):
        if "__class__" not in v.__code__.co_freevars:
            return v
        closure = tuple(cell if n == "__class__" else c for n, c in zip(v.__code__.co_freevars, v.__closure__))
        f = types.FunctionType(v.__code__, v.__globals__, v.__name__, v.__defaults__, closure)
        f.__kwdefaults__, f.__qualname__, f.__doc__, f.__module__ = v.__kwdefaults__, v.__qualname__, v.__doc__, v.__module__
        f.__dict__.update(v.__dict__)
        f.__annotations__ = dict(getattr(v, "__annotations__", {}) or {})
        return f
    if isinstance(v, staticmethod):
        return staticmethod(_rebind_class_cell(v.__func__, cell))
    if isinstance(v, classmethod):
        return classmethod(_rebind_class_cell(v.__func__, cell))
    if isinstance(v, property):
        return property(*(None if f is None else _rebind_class_cell(f, cell) for f in (v.fget, v.fset, v.fdel)), v.__doc__)
    return v


def _bare_instance(cls):
    r = _realise(cls)
    return r.__new__(r)


def _realise(cls):
    """The ordinary class behind a user's subclass of a dispatching name: built ONCE per subclass -- so type(a) is type(b) and
    isinstance works --, on the host class (or on the realisations of the user's own intermediate subclasses), with the subclass's
    namespace on top and the `__class__` cell of its methods re-pointed at the realisation, so that zero-argument `super()` resolves
    (`super().__init__(...)`, an overriding `fit` that calls `super().fit`).  Instances pickle through the dispatching name the user's
    module holds (`__reduce_ex__`), which is the only name pickle / dill can look up."""
    r = _REALISED.get(cls)
    if r is not None:
        return r
    bases = []
    for b in cls.__bases__:
        if isinstance(b, _Dispatch):
            if "_pick" in b.__dict__:
                host = b.__dict__.get("_host")
                if host is None:
                    raise TypeError("%s derives from a dispatching bogp class that has no host class to fall back to" % cls.__name__)
                bases.append(host)
            else:
                bases.append(_realise(b))
        else:
            bases.append(b)
    cell = types.CellType()
    ns = {k: _rebind_class_cell(v, cell) for k, v in cls.__dict__.items() if k not in ("__dict__", "__weakref__")}

    def __reduce_ex__(self, protocol, _cls=cls):
        state = self.__getstate__() if hasattr(self, "__getstate__") and type(self).__getstate__ is not getattr(object, "__getstate__", None) else self.__dict__
        return (_bare_instance, (_cls,), state)

    ns.setdefault("__reduce_ex__", __reduce_ex__)
    r = type(cls.__name__, tuple(bases), ns)
    cell.cell_contents = r
    _REALISED[cls] = r
    return r


def _dispatching_criterion(name, device_cls, host_cls):
    def _pick(args, kwargs):
        model = kwargs.get("model", next((a for a in args if hasattr(a, "predict")), None))
        if device_cls is not None and (is_device_model(model) or host_cls is None):
            return device_cls
        return host_cls

    return _Dispatch(name, (), {"_device": device_cls, "_host": host_cls, "_pick": staticmethod(_pick),
                                "__doc__": "dispatches on `model`: %s on a bogp.GaussianProcess, the reference's otherwise" % name})  # fmt: skip


class _AcquisitionNamespace:
    """Stands in for the module `bayes_optim.acquisition.acquisition_fun` under the name `AcquisitionFunction`
    (`base.py:14,250,488`, `bayes_opt.py:8,21,96,187`, `extension.py:13,327`): criteria this package implements dispatch
    per model, every other attribute is the reference module's own."""

    def __init__(self, reference_module):
        self._ref = reference_module
        self._classes = {}
        for name in ("EI", "PI", "EpsilonPI", "UCB", "MGFI"):
            ours, theirs = getattr(acquisition, name, None), getattr(reference_module, name, None)
            if ours is not None:
                self._classes[name] = _dispatching_criterion(name, ours, theirs)

    def __getattr__(self, name):
        classes = self.__dict__.get("_classes", {})
        if name in classes:
            return classes[name]
        return getattr(self.__dict__["_ref"], name)

    def __dir__(self):
        return sorted(set(dir(self._ref)) | set(self._classes))


def _dispatching_surrogate(host_cls):
    def _pick(args, kwargs):
        # install(restart_batch=...): defaults of the device models the drivers build themselves (taken back if the host class is picked)
        added = [k for k in _SURROGATE_DEFAULTS if k not in kwargs]
        for k in added:
            kwargs[k] = _SURROGATE_DEFAULTS[k]
        try:  # validate on a throw-away instance: the constructor touches no device
            probe = _DeviceGP(*args, **kwargs)
            probe._trend_args()  # a trend basis the device does not evaluate is found NOW, not at fit() (it raises NotImplementedError)
            return _DeviceGP
        except NotImplementedError as e:
            for k in added:
                kwargs.pop(k, None)
            warnings.warn("bogp: this GaussianProcess configuration stays on the reference's CPU class (%s)" % e, stacklevel=3)
            return host_cls

    return _Dispatch("GaussianProcess", (), {"_device": _DeviceGP, "_host": host_cls, "_pick": staticmethod(_pick),
                                             "__doc__": "bogp.GaussianProcess where the device serves the configuration, "
                                                        "else bayes_optim's CPU class"})  # fmt: skip


def install(bayes_optim=None, fuse_batch: bool = True, reroute_bfgs: str = None, sweep_budget: int = 1_000_000, surrogate: bool = True,
            restart_batch: int = None, batch_strategy: str = "topk", ehvi_gradient: bool = False, expensive_constraints: bool = False,
            equality_tol: float = 0.1, constraint_gradient: bool = False, constraint_batches: str = "topk", constrained_mobo: bool = False,
            constrained_mobo_gradient: bool = False, constrained_mobo_batches: str = "topk", constraint_thompson: bool = False):
    """Re-point the reference's extension points at this package (see the module docstring).  `bayes_optim` is the
    imported reference package (default: `import bayes_optim`).  Returns `uninstall()`.  Idempotent.

    `surrogate=True`: `bayes_optim.GaussianProcess` and `bayes_optim.surrogate.GaussianProcess` build
    `bogp.GaussianProcess`, hence `bayes_optim.fmin(...)` fits, predicts and maximises on the device (the defining module
    `bayes_optim.surrogate.gaussian_process` keeps the CPU class; names imported BEFORE install() keep what they had).

    `reroute_bfgs` = "sweep" | "sweep-device" | "sweep-device-lhs" | "sweep-device-sobol" | "sweep-BFGS" | "sweep-device-BFGS": drivers constructed
    WITHOUT `acquisition_optimization` fall to the reference's default "BFGS" (one device round trip per point); with a
    reroute their inner maximisation becomes one sweep of `sweep_budget` candidates instead -- no change to the driver's
    constructor call.  Constrained problems, foreign models and non-real spaces are never rerouted.

    `restart_batch` = R: device models built through the re-pointed name get `restart_batch=R` unless the call names its own.

    `batch_strategy` = "topk" | "believer" | "thompson": how the fused `ParallelBO` step keeps its q points apart.  "topk" (default): each
    criterion falls back through its top-k; "believer": `optim.believer_batch` -- criterion j sees the variance conditioned on
    the winners before it (a step with fixed variables or constraints, which the believer does not serve, keeps "topk").  The q
    parameters are drawn with the reference's sampler in the reference's order either way.  Under "believer" the reference's
    `MOBO(n_point=q)` proposes q points as well (`optim.ehvi_believer_batch`: EHVI on the variance conditioned on the winners before
    and on the front their believed means extend); under "topk" its `ask(q)` raises NotImplementedError as in the reference.
    "thompson": `optim.thompson_batch` -- one posterior sample path per point, each optimised over the candidates; the criteria
    supply model and direction only.  Fixed variables and constraints keep "topk" as under the believer; a model Thompson
    sampling refuses (a nugget or noise estimate, a polynomial trend, ...) raises NotImplementedError naming it.

    `ehvi_gradient=True` (an extension: the reference's EHVI has no gradient): the reference's `MOBO` with a device GP on a
    continuous space runs "BFGS", "sweep-BFGS" and "sweep-device-BFGS" on `bogp.EHVI(input_gradient=True)` -- the closed-form
    input gradient of `bogp_point_eval_ehvi` and the lock-step polish `bogp_polish_ehvi`.  Without it `MOBO` with those
    optimisers runs the original.

    `expensive_constraints=True` (an extension: the reference's `tell` accepts `h_vals` / `g_vals` and drops them, base.py:328): a `BO` /
    `ParallelBO` with a device GP keeps them (`constrained_tell`), fits objective and constraints as one multi-target model
    (`constrained_update_model`) and maximises `bogp.Constrained` -- EI / PI / EpsilonPI / MGFI times the probability that g <= 0 and
    |h| <= `equality_tol` (the reference's own equality threshold, `dynamic_penalty`, utils.py:280) -- under the sweep family
    (`constrained_create_acquisition`); `bogp.feasible_xopt(bo)` is the best feasible observation.  Off (the default): nothing of
    this is patched in effect and `tell` drops the values as before.

    `constraint_gradient=True` (with `expensive_constraints=True`; alone it raises ValueError): such a driver also accepts "BFGS",
    "sweep-BFGS" and "sweep-device-BFGS" and maximises `bogp.Constrained(input_gradient=True)` -- the input gradient of
    `bogp_point_eval_constrained` and the lock-step polish `bogp_polish_constrained`.  Without it those optimisers raise as before.

    `constraint_batches` = "topk" | "believer" ("believer" with `expensive_constraints=True`; alone it raises ValueError): how the fused
    `ParallelBO` step keeps the q points of a driver with modelled constraints apart.  "topk" (default): as before, whatever
    `batch_strategy` says.  "believer": `optim.constrained_believer_batch` -- criterion j sees the m variances conditioned on the
    winners before it, and a believed point that is feasible by belief lowers the plugin -- when every criterion of the step is a
    `bogp.Constrained`, the inner optimiser is of the sweep family, nothing is fixed and no cheap h / g is given; every other step
    takes the route it took before.

    `constraint_thompson=True` (with `expensive_constraints=True`; alone, or together with `constraint_batches="believer"`, it raises
    ValueError): the same steps go to `optim.constrained_thompson_batch` instead -- per point one joint draw of the objective and
    the constraints, the best drawn objective where the drawn constraints hold, the least violating row where they hold nowhere
    (Eriksson & Poloczek 2021) -- with the run's history; the criteria supply model, bounds and direction only.  A model that
    Thompson sampling refuses (a nugget or noise estimate, ...) raises NotImplementedError naming it.

    `constrained_mobo=True` (with `expensive_constraints=True`; alone it raises ValueError; an extension: `BaseMOBO.tell` leaves the
    values as a TODO, mobo.py:117-118): the reference's `MOBO` with a device GP keeps the `h_vals` / `g_vals` of its tell()
    (`refusing_mobo_tell`, by `constrained_tell`'s rules), fits objectives and constraints as one multi-target model
    (`constrained_mobo_update_model`) and maximises `bogp.ConstrainedEHVI` -- EHVI over the cells of the feasible front times the
    probability that g <= 0 and |h| <= `equality_tol` -- under the sweep family on a continuous space; any other inner optimiser and
    `MOBO(n_point=q)` (without `constrained_mobo_batches="believer"`) raise instead of dropping the constraints.  `bogp.feasible_front(bo)` is the feasible non-dominated set.  Without
    it a MOBO tell() with constraint values is refused by name as before.

    `constrained_mobo_gradient=True` (with `constrained_mobo=True`; without it ValueError): such a MOBO also accepts "BFGS", "sweep-BFGS"
    and "sweep-device-BFGS" after a tell() that carried constraint values and maximises `bogp.ConstrainedEHVI(input_gradient=True)` --
    the input gradient of `bogp_point_eval_ehvi_constrained` and the lock-step polish `bogp_polish_ehvi_constrained`.  Without it
    those optimisers raise as before.

    `constrained_mobo_batches` = "topk" | "believer" ("believer" with `constrained_mobo=True`; alone it raises ValueError; any other
    value raises ValueError): what `MOBO(n_point=q)` does after a tell() that carried constraint values.  "topk" (default): it raises
    NotImplementedError as before (top-k batches of constrained EHVI crowd into one pocket of the feasibility boundary and are
    not offered).  "believer": `optim.constrained_ehvi_believer_batch` -- step j sees the m + c variances conditioned on the
    winners before it, and a believed point that is feasible by belief joins the feasible front -- for a device GP, an inner
    optimiser of the sweep family, a continuous space, nothing fixed and no cheap h / g; every other configuration raises as
    before."""
    if constrained_mobo_batches not in ("topk", "believer"):
        raise ValueError("constrained_mobo_batches must be 'topk' or 'believer', not %r" % (constrained_mobo_batches,))
    if constrained_mobo_batches == "believer" and not constrained_mobo:
        raise ValueError("constrained_mobo_batches='believer' needs constrained_mobo=True (it batches constrained EHVI)")
    if constrained_mobo and not expensive_constraints:
        raise ValueError("constrained_mobo=True needs expensive_constraints=True (it keeps the h_vals / g_vals of a multi-objective tell())")
    if constrained_mobo_gradient and not constrained_mobo:
        raise ValueError("constrained_mobo_gradient=True needs constrained_mobo=True (it is the input gradient of constrained EHVI)")
    if constraint_batches not in ("topk", "believer"):
        raise ValueError("constraint_batches must be 'topk' or 'believer', not %r" % (constraint_batches,))
    if constraint_batches == "believer" and not expensive_constraints:
        raise ValueError("constraint_batches='believer' needs expensive_constraints=True (it batches the feasibility-weighted criterion)")
    if constraint_thompson and not expensive_constraints:
        raise ValueError("constraint_thompson=True needs expensive_constraints=True (it draws the objective and the modelled constraints jointly)")
    if constraint_thompson and constraint_batches == "believer":
        raise ValueError("constraint_thompson=True and constraint_batches='believer' name two batch strategies for one step: choose one")
    if constraint_gradient and not expensive_constraints:
        raise ValueError("constraint_gradient=True needs expensive_constraints=True (it is the input gradient of the feasibility-weighted criterion)")
    _CONSTRAINTS.clear()
    if expensive_constraints:
        if not (float(equality_tol) >= 0):
            raise ValueError("equality_tol must be >= 0")
        _CONSTRAINTS["tol"] = float(equality_tol)
        if constraint_gradient:
            _CONSTRAINTS["gradient"] = True
        if constraint_batches == "believer":
            _CONSTRAINTS["batches"] = "believer"
        if constraint_thompson:
            _CONSTRAINTS["batches"] = "thompson"
        if constrained_mobo:
            _CONSTRAINTS["mobo"] = True
        if constrained_mobo_gradient:
            _CONSTRAINTS["mobo_gradient"] = True
        if constrained_mobo_batches == "believer":
            _CONSTRAINTS["mobo_batches"] = "believer"
    if batch_strategy not in ("topk", "believer", "thompson"):
        raise ValueError("batch_strategy must be 'topk', 'believer' or 'thompson', not %r" % (batch_strategy,))
    _EHVI.clear()
    if ehvi_gradient:
        _EHVI["gradient"] = True
    _BATCH.clear()
    if batch_strategy != "topk":
        _BATCH["strategy"] = batch_strategy
    if restart_batch is not None:
        # the models `fmin` / the drivers build through the re-pointed GaussianProcess name fit with their MLE restarts in lock step
        # (surrogate.GaussianProcess(restart_batch=R)): `tell()` is most of a BO loop's wall time.  Opt-in: the
        # sequential loop with scipy's optimiser stays the default, as in the reference.
        _SURROGATE_DEFAULTS["restart_batch"] = int(restart_batch)
    if reroute_bfgs is not None:
        if reroute_bfgs not in _OURS:
            raise ValueError("reroute_bfgs must be one of %s" % (_OURS,))
        _REROUTE.update(optimizer=reroute_bfgs, budget=int(sweep_budget))
    if bayes_optim is None:
        import bayes_optim  # noqa: PLC0415
    import importlib

    rbase = importlib.import_module(bayes_optim.__name__ + ".base")
    ropt = importlib.import_module(bayes_optim.__name__ + ".bayes_opt")
    racq = importlib.import_module(bayes_optim.__name__ + ".acquisition.acquisition_fun")
    rsur = importlib.import_module(bayes_optim.__name__ + ".surrogate")
    try:
        rext = importlib.import_module(bayes_optim.__name__ + ".extension")
    except Exception:  # optional module with heavier dependencies
        rext = None
    try:
        rmobo = importlib.import_module(bayes_optim.__name__ + ".mobo")
    except Exception:  # (the multi-objective driver needs torch)
        rmobo = None

    if _ORIGINAL:
        return uninstall
    holders = [m for m in (rbase, ropt, rext) if m is not None and getattr(m, "AcquisitionFunction", None) is racq]
    _ORIGINAL.update(argmax=rbase.argmax_restart, acq_holders=holders, acq=racq, batch=ropt.ParallelBO._batch_arg_max_acquisition,
                     mods=(bayes_optim, rbase, ropt, rsur), gp=(getattr(bayes_optim, "GaussianProcess", None), rsur.GaussianProcess),
                     surrogate=bool(surrogate), mobo_cls=None, ext=None)  # fmt: skip
    rbase.argmax_restart = routed_argmax_restart
    _ORIGINAL.update(create=rbase.BaseBO.__dict__["_create_acquisition"], base_cls=rbase.BaseBO, base_partial_argument=rbase.partial_argument)
    rbase.BaseBO._create_acquisition = constrained_create_acquisition  # (hands on to forest_create_acquisition)
    _ORIGINAL.update(tell=rbase.BaseBO.__dict__["tell"], update_model=rbase.BaseBO.__dict__["update_model"])
    rbase.BaseBO.tell, rbase.BaseBO.update_model = constrained_tell, constrained_update_model
    if rmobo is not None and "tell" in getattr(rmobo, "BaseMOBO", type("", (), {})).__dict__:
        _ORIGINAL.update(mobo_tell_cls=rmobo.BaseMOBO, mobo_tell=rmobo.BaseMOBO.__dict__["tell"])
        rmobo.BaseMOBO.tell = refusing_mobo_tell
        if "update_model" in rmobo.BaseMOBO.__dict__:
            _ORIGINAL.update(mobo_mod=rmobo, mobo_update_model=rmobo.BaseMOBO.__dict__["update_model"])
            rmobo.BaseMOBO.update_model = constrained_mobo_update_model
    if rmobo is not None and hasattr(rmobo, "MOBO"):
        _ORIGINAL.update(mobo_cls=rmobo.MOBO, mobo=rmobo.MOBO.__dict__["_create_acquisition"], partial_argument=rmobo.partial_argument)
        rmobo.MOBO._create_acquisition = mobo_create_acquisition
        if "_batch_arg_max_acquisition" not in rmobo.MOBO.__dict__:  # inherited from BaseBO (raises): given, not replaced
            rmobo.MOBO._batch_arg_max_acquisition = mobo_batch_arg_max_acquisition
            _ORIGINAL["mobo_batch"] = True
    ns = _AcquisitionNamespace(racq)
    for m in holders:
        m.AcquisitionFunction = ns
    if fuse_batch:
        ropt.ParallelBO._batch_arg_max_acquisition = fused_batch_arg_max_acquisition
    if surrogate:
        gp = _dispatching_surrogate(rsur.GaussianProcess)
        bayes_optim.GaussianProcess = rsur.GaussianProcess = gp
        if rext is not None and hasattr(rext, "GaussianProcess"):  # PCABO.update_model builds its surrogate through this name (extension.py:17,183)
            _ORIGINAL["ext"] = (rext, rext.GaussianProcess)
            rext.GaussianProcess = gp
    return uninstall


def uninstall():
    if not _ORIGINAL:
        return
    pkg, rbase, ropt, rsur = _ORIGINAL["mods"]
    rbase.argmax_restart = _ORIGINAL["argmax"]
    _ORIGINAL["base_cls"]._create_acquisition = _ORIGINAL["create"]
    _ORIGINAL["base_cls"].tell, _ORIGINAL["base_cls"].update_model = _ORIGINAL["tell"], _ORIGINAL["update_model"]
    if _ORIGINAL.get("mobo_tell_cls") is not None:
        _ORIGINAL["mobo_tell_cls"].tell = _ORIGINAL["mobo_tell"]
        if _ORIGINAL.get("mobo_update_model") is not None:
            _ORIGINAL["mobo_tell_cls"].update_model = _ORIGINAL["mobo_update_model"]
    for m in _ORIGINAL["acq_holders"]:
        m.AcquisitionFunction = _ORIGINAL["acq"]
    ropt.ParallelBO._batch_arg_max_acquisition = _ORIGINAL["batch"]
    if _ORIGINAL["mobo_cls"] is not None:
        _ORIGINAL["mobo_cls"]._create_acquisition = _ORIGINAL["mobo"]
        if _ORIGINAL.get("mobo_batch"):
            del _ORIGINAL["mobo_cls"]._batch_arg_max_acquisition  # inherited again
    if _ORIGINAL["surrogate"]:
        pkg.GaussianProcess, rsur.GaussianProcess = _ORIGINAL["gp"]
        if _ORIGINAL.get("ext") is not None:
            rext, ext_gp = _ORIGINAL["ext"]
            rext.GaussianProcess = ext_gp
    _ORIGINAL.clear()
    _REROUTE.clear()
    _BATCH.clear()
    _EHVI.clear()
    _CONSTRAINTS.clear()
    _SURROGATE_DEFAULTS.clear()
