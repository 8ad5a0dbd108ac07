"""Inner maximiser of the acquisition function: the M-candidate GPU sweep behind `argmax_restart`'s signature.

The reference maximises one criterion with multi-restart L-BFGS-B / (1+1)-CMA-ES / MIES, ONE point per call
(`bayes_optim/acquisition/optim/__init__.py:55-153`; <= 100 d points per `ask()`).  The sweep is a new option
behind the same signature (`optimizer="sweep"`): sample `eval_budget` candidates in the box, evaluate posterior +
criterion for all of them in one device pass, return the argmax as `(xopt: list, fopt: float)`.
q criteria that differ only in their parameter (ParallelBO's t / alpha draws, `bayes_opt.py:100-115`) share one
posterior pass: `sweep_argmax(criteria=[...])`.

Candidates shard across ranks (one process per GPU): every rank sweeps its own block and ONE exchange of
q x (value, global index) decides the winner (`distributed.exchange_argmax`).
"""
from __future__ import annotations

import functools
import inspect
import warnings
from typing import Callable, List, Optional, Sequence

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

from . import _lib
from . import distributed
from . import forest as _forest
from .lift import Lift


_TRANS = {  # Real.scale -> (forward, inverse) (variable.py:22-55)
    "linear": (lambda v: v, lambda v: v),
    "log": (np.log, np.exp),
    "log10": (np.log10, lambda v: np.power(10, v)),
    "logit": (lambda v: np.log(v / (1 - v)), lambda v: 1 / (1 + np.exp(-v))),
    "bilog": (lambda v: np.sign(v) * np.log(1 + np.abs(v)), lambda v: np.sign(v) * (np.exp(np.abs(v)) - 1)),
}


class Box:
    """Minimal continuous search space with the members of `RealSpace` the maximiser touches
    (`search_space.py:724-769`: `bounds`, `dim`, `sample(N, method)`), incl. the per-variable `scale` and `precision` of
    `Real` (variable.py:165-257): sampling is uniform on the transformed scale, then mapped back, rounded and clipped."""

    def __init__(self, bounds, random_seed=None, precision=None, scale=None):
        self.bounds = [tuple(map(float, b)) for b in bounds]
        self.dim = len(self.bounds)
        self._rng = np.random.default_rng(random_seed)
        self.precision = list(precision) if np.ndim(precision) else [precision] * self.dim
        self.scale = [(s or "linear") for s in (list(scale) if np.ndim(scale) else [scale] * self.dim)]

    def sample(self, N=1, method="uniform"):
        lo_t, hi_t, scales, precs, lo, hi = design_of(self)
        X = self._rng.uniform(lo_t, hi_t, size=(int(N), self.dim))
        for k in range(self.dim):
            X[:, k] = _TRANS[scales[k]][1](X[:, k])
            if precs[k] is not None:
                X[:, k] = np.clip(np.round(X[:, k], precs[k]), lo[k], hi[k])
        return X


def design_of(space):
    """(lo_t, hi_t, scales, precisions, lo, hi) of a continuous search space: the box the design is DRAWN in (transformed
    bounds, `Real._bounds_transformed`), the per-variable scale names and precisions, and the variables' own bounds.
    Accepts a plain list of (lo, hi) pairs, a `Box`, or the reference's `RealSpace` (its `data` list of `Real`)."""
    if isinstance(space, Box):
        lo = np.array([b[0] for b in space.bounds], dtype=float)
        hi = np.array([b[1] for b in space.bounds], dtype=float)
        scales, precs = list(space.scale), list(space.precision)
    elif hasattr(space, "data") and hasattr(space, "bounds"):  # bayes_optim.RealSpace
        lo = np.array([v.bounds[0] for v in space.data], dtype=float)
        hi = np.array([v.bounds[1] for v in space.data], dtype=float)
        scales = [getattr(v, "scale", "linear") or "linear" for v in space.data]
        precs = [getattr(v, "precision", None) for v in space.data]
    else:
        b = list(getattr(space, "bounds", space))
        lo = np.array([x[0] for x in b], dtype=float)
        hi = np.array([x[1] for x in b], dtype=float)
        scales, precs = ["linear"] * len(b), [None] * len(b)
    lo_t = np.array([_TRANS[s][0](np.float64(a)) for s, a in zip(scales, lo)], dtype=float)
    hi_t = np.array([_TRANS[s][0](np.float64(a)) for s, a in zip(scales, hi)], dtype=float)
    return lo_t, hi_t, scales, precs, lo, hi


def _generate(eng, space, count, seed, first_row, method, n_total):
    """Draw `count` rows of the design of `space` on the device, with RealSpace._sample's post-processing
    (search_space.py:754: to_linear_scale, then round) applied there too."""
    lo_t, hi_t, scales, precs, lo, hi = design_of(space)
    plain = all(s == "linear" for s in scales) and all(p is None for p in precs)
    eng.set_candidate_transform(None if plain else scales, None if plain else precs, lo, hi)
    eng.generate_candidates(lo_t, hi_t, count, seed, first_row=first_row, method=method, n_total=n_total)


def device_sample(engine, space, N: int, method: str = "LHS-maximin", seed: int = 0, maximin: int = 5) -> np.ndarray:
    """`space.sample(N, method)` of the reference (search_space.py:742-754) drawn on the device and read back: (N, d).
    `method`: "uniform" | "LHS" | "LHS-maximin" | "sobol" -- the reference's own "LHS" is pyDOE's maximin criterion over
    five hypercubes, i.e. "LHS-maximin" here (the plain "LHS" is one hypercube, the only flavour that can be drawn in
    row shards).  The engine must know d (a training set has been set); its candidate buffer is overwritten."""
    lo_t, hi_t, scales, precs, lo, hi = design_of(space)
    plain = all(s == "linear" for s in scales) and all(p is None for p in precs)
    engine.set_candidate_transform(None if plain else scales, None if plain else precs, lo, hi)
    engine.generate_candidates(lo_t, hi_t, int(N), seed, method=method, maximin=maximin)
    return engine.read_candidates(np.arange(int(N)))


def shard_bounds(M: int, rank: int, world: int):
    """Contiguous block of rank r: rows [r M / R, (r+1) M / R)."""
    return (rank * M) // world, ((rank + 1) * M) // world


def is_continuous(space) -> bool:
    """True for the spaces the sweep and L-BFGS-B serve: a `Box`, the reference's `RealSpace` (recognised by class name
    through the MRO -- `isinstance(search_space, RealSpace)` is the reference's own test, optim/__init__.py:71), or a
    plain sequence of (lo, hi) pairs."""
    if space is None:
        return False
    if isinstance(space, Box) or "RealSpace" in [c.__name__ for c in type(space).__mro__]:
        return True
    if any(c.__name__ == "SearchSpace" for c in type(space).__mro__):
        return False
    try:
        return all(len(b) == 2 for b in space)
    except TypeError:
        return False


def engine_rank_world(eng, group=None):
    """(rank, world) a sweep shards by: the engine's own communicator when it has one (`bogp_comm_init` with an id that
    travelled out of band, or `bogp_comm_attach`: no torch process group need exist), else the torch process group."""
    if getattr(eng, "comm_world", 0):
        return int(eng.comm_rank), int(eng.comm_world)
    return distributed.rank_world(group)


def feasible_rows(X: np.ndarray, h: Optional[Callable], g: Optional[Callable]) -> np.ndarray:
    """Boolean mask of the rows of X the reference would ACCEPT as the outcome of a restart (optim/__init__.py:125-127):
    |h(x)| within 1e-1 of zero for every equality constraint and g(x) <= 0 for every inequality constraint.  `h` / `g`
    take one point as a list, like the wrappers `BaseBO` binds (base.py:224-229, 236-237)."""
    keep = np.ones(len(X), dtype=bool)
    if len(X) > 100_000 and (h is not None or g is not None):  #  one Python call per candidate and constraint
        warnings.warn("a constrained sweep calls the constraint functions once per candidate (%d Python calls): lower eval_budget "
                      "or keep the problem on the reference's optimiser" % len(X), RuntimeWarning, stacklevel=3)
    for i in range(len(X)):
        x = X[i].tolist()
        if h is not None:
            keep[i] = bool(np.all(np.isclose(np.abs(h(x)), 0, atol=1e-1)))
        if keep[i] and g is not None:
            keep[i] = bool(np.all(np.asarray(g(x)) <= 0))
    return keep


def candidate_block(bounds, M: int, seed: int, rank: int = 0, world: int = 1) -> np.ndarray:
    """This rank's block of M uniform candidates in the box: a deterministic function of (seed, rank, world)."""
    lo = np.array([b[0] for b in bounds], dtype=float)
    hi = np.array([b[1] for b in bounds], dtype=float)
    a, b_ = shard_bounds(M, rank, world)
    rng = np.random.default_rng([int(seed), int(rank), int(world)])
    return rng.uniform(lo, hi, size=(b_ - a, len(lo)))


def is_ehvi(criterion) -> bool:
    """True for `acquisition.EHVI` (the multi-objective criterion: its sweep is `bogp_sweep_ehvi`, not `bogp_sweep`)."""
    return bool(getattr(criterion, "is_ehvi", False))


def is_constrained_ehvi(criterion) -> bool:
    """True for `acquisition.ConstrainedEHVI` (EHVI weighted by the probability that modelled constraints hold: its sweep is
    `bogp_sweep_ehvi_constrained`).  It is `is_ehvi` as well -- the sweep helpers call its `.sweep()` as they call EHVI's -- and not
    `is_constrained`; whatever does more with an EHVI than call `.sweep()` (the polish, the believer) asks for this flag first."""
    return bool(getattr(criterion, "is_constrained_ehvi", False))


_CEHVI = "constrained EHVI (bogp.ConstrainedEHVI)"


def _ehvi_of(criteria: Sequence, eng, group=None):
    """The EHVI criterion a sweep serves (`EHVI` or `ConstrainedEHVI`), or None when every criterion is single-objective.  It sweeps
    alone, on one rank."""
    flags = [is_ehvi(c) for c in criteria]
    if not any(flags):
        return None
    if len(criteria) != 1:
        raise ValueError("an EHVI criterion sweeps alone: it cannot share a sweep with other criteria")
    if is_constrained_ehvi(criteria[0]) and engine_rank_world(eng, group)[1] > 1:
        raise NotImplementedError("the sweep of %s runs on one rank (no multi-rank exchange of its winners)" % _CEHVI)
    if engine_rank_world(eng, group)[1] > 1:
        raise NotImplementedError("the EHVI sweep runs on one rank (no multi-rank exchange of its winners)")
    return criteria[0]


def is_constrained(criterion) -> bool:
    """True for `acquisition.Constrained` (a criterion weighted by the probability that modelled constraints hold: its sweep is
    `bogp_sweep_constrained` on a multi-target model, not `bogp_sweep`)."""
    return bool(getattr(criterion, "is_constrained", False))


def _constrained_of(criteria: Sequence, eng, group=None):
    """The first of the `Constrained` criteria a sweep serves together, or None when none of them is one.  They share one call of
    `bogp_sweep_constrained`, hence model, bounds, plugin and direction; a list that mixes them with other criteria is refused."""
    flags = [is_constrained(c) for c in criteria]
    if not any(flags):
        return None
    if not all(flags):
        raise ValueError("feasibility-weighted criteria (bogp.Constrained) cannot share a sweep with other criteria")
    c0 = criteria[0]
    for c in criteria[1:]:
        if (c.model is not c0.model or c.minimize != c0.minimize or c.effective_plugin() != c0.effective_plugin()
                or not np.array_equal(c.lo, c0.lo) or not np.array_equal(c.hi, c0.hi)):  # fmt: skip
            raise ValueError("Constrained criteria sharing one sweep must share model, bounds, plugin and minimize")
    if engine_rank_world(eng, group)[1] > 1:
        raise NotImplementedError("the constrained sweep (bogp.Constrained) runs on one rank (no multi-rank exchange of its winners)")
    return c0


def _constrained_topk(criteria: Sequence, k: int):
    """(values (q, k), local indices (q, k)) of q `Constrained` criteria over the engine's current candidates, in one call."""
    c0 = criteria[0]
    return c0.model.engine.sweep_constrained([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize, c0.lo, c0.hi,
                                             k=int(k))[:2]  # fmt: skip


def _lifted_topk(criteria: Sequence, eng, lift: Lift, k: int, group=None):
    """The k best rows per criterion of the engine's current candidates under `lift` (`bogp_lift_sweep_topk`): rows whose
    lifted point leaves the original box compete with their penalty (extension.py:62-86).  The lift is taken off the engine
    again before this returns, whatever happens: a later plain sweep never sees it."""
    if any(is_constrained_ehvi(c) for c in criteria):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not %s" % _CEHVI)
    if any(is_ehvi(c) for c in criteria):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not EHVI")
    if any(is_constrained(c) for c in criteria):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not modelled constraints (bogp.Constrained)")
    if any(_forest.is_forest_model(c.model) for c in criteria):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves a Gaussian process model, not a forest")
    if engine_rank_world(eng, group)[1] > 1:
        raise NotImplementedError("a lifted sweep (PCA-BO) runs on one rank (no multi-rank exchange of penalised winners)")
    c0 = criteria[0]
    for c in criteria[1:]:
        if c.model is not c0.model or c.minimize != c0.minimize or c.effective_plugin() != c0.effective_plugin():
            raise ValueError("criteria sharing one sweep must share model, minimize and plugin")
    if lift.r != eng.d:
        raise ValueError("the lift maps %d reduced dimensions, the model has %d" % (lift.r, eng.d))
    eng.set_lift(lift.A, lift.mean, lift.center, lift.lo, lift.hi)
    try:
        return eng.lift_sweep_topk([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize, int(k))[:2]
    finally:
        eng.clear_lift()


def sweep_argmax(criteria: Sequence, Xs: np.ndarray, index_offset: int = 0, group=None, return_points: bool = True,
                 lift: Optional[Lift] = None):
    """Evaluate q criteria (same model, same minimize / plugin) on this rank's candidates `Xs` and reduce across
    ranks.  Returns (best_val (q,), best_global_idx (q,), best_x (q, d) or None).  `lift` (a `Lift`, PCA-BO): `Xs` are rows
    of the reduced space; a row whose lifted point leaves the original box competes with its penalty instead of its
    criterion value; one rank only."""
    c0 = criteria[0]
    model = c0.model
    eng = model.engine
    if lift is not None:
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        Xs = model._check_X(Xs)
        eng.upload_candidates(Xs, lazy=True)
        best, idx = _lifted_topk(criteria, eng, lift, 1, group)
        return best[:, 0], idx[:, 0] + int(index_offset), (Xs[idx[:, 0]] if return_points else None)
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    ehvi = _ehvi_of(criteria, eng, group)
    con = _constrained_of(criteria, eng, group)
    for c in criteria[1:]:
        if c.model is not model or c.minimize != c0.minimize or c.effective_plugin() != c0.effective_plugin():
            raise ValueError("criteria sharing one sweep must share model, minimize and plugin")
    Xs = model._check_X(Xs)
    eng.upload_candidates(Xs, lazy=True)  # (the sweep right below overlaps the copy with its first chunks)
    if ehvi is not None:
        best, idx = ehvi.sweep(k=1)
        return best, idx + int(index_offset), (Xs[idx] if return_points else None)
    if con is not None:
        best, idx = (a[:, 0] for a in _constrained_topk(criteria, 1))
        return best, idx + int(index_offset), (Xs[idx] if return_points else None)
    acq = [(c.acq_id, c.acq_par()) for c in criteria]
    best, idx = eng.sweep(acq, c0.effective_plugin(), c0.minimize)
    if getattr(eng, "comm_world", 0):  # the library's own exchange: device records, ONE ncclAllGather, no host bounce
        return eng.exchange_argmax(len(acq), int(index_offset), return_points)
    gidx = idx + int(index_offset)
    xbest = Xs[idx] if return_points else None
    return distributed.exchange_argmax(best, gidx, xbest, group=group)


def sweep_generated(criteria: Sequence, bounds, M: int, seed: int, rank: int = 0, world: int = 1, group=None,
                    method: str = "uniform", lift: Optional[Lift] = None):
    """`sweep_argmax` over M candidates in `bounds` (a list of (lo, hi) pairs, a `Box`, or the reference's `RealSpace` -- scales
    and precisions of its variables are honoured on the device) that never touch the host: rank r draws rows
    [r M / R, (r+1) M / R) of the design on its GPU, sweeps them, and the ranks exchange their winners (value, global
    row, point).  `method` names the design like `RealSpace._sample` does (search_space.py:742-754): "uniform" (Philox
    stream `seed`), "LHS" (an M-point Latin hypercube of stream `seed`; "LHS-maximin": pyDOE's criterion, one rank only),
    "sobol" (points 1..M of the unscrambled
    sequence; `seed` unused).  The union of the shards is the same M-point set for every world size.  `lift`: as in
    `sweep_argmax` (`bounds` is then the box of the reduced space; one rank only)."""
    c0 = criteria[0]
    model = c0.model
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    a, b_ = shard_bounds(int(M), rank, world)
    eng = model.engine
    if lift is not None:
        if world > 1:
            raise NotImplementedError("a lifted sweep (PCA-BO) runs on one rank (no multi-rank exchange of penalised winners)")
        _generate(eng, bounds, int(M), seed, 0, method, int(M))
        best, idx = _lifted_topk(criteria, eng, lift, 1, group)
        return best[:, 0], idx[:, 0], eng.read_candidates(idx[:, 0])
    ehvi = _ehvi_of(criteria, eng, group)
    con = _constrained_of(criteria, eng, group)
    _generate(eng, bounds, b_ - a, seed, a, method, int(M))
    if ehvi is not None:
        best, idx = ehvi.sweep(k=1)
        return best, idx + a, eng.read_candidates(idx)
    if con is not None:
        best, idx = (v[:, 0] for v in _constrained_topk(criteria, 1))
        return best, idx + a, eng.read_candidates(idx)
    best, idx = eng.sweep([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize)
    if getattr(eng, "comm_world", 0):
        return eng.exchange_argmax(len(criteria), a, True)
    return distributed.exchange_argmax(best, idx + a, eng.read_candidates(idx), group=group)


def _topk_points(idx, rows, n_rows):
    """(q, k, d) points of the (q, k) local indices `idx` through `rows(flat indices) -> (n, d)`; NaN where idx < 0."""
    flat = np.clip(idx, 0, n_rows - 1).ravel()
    pts = np.asarray(rows(flat), dtype=float)
    return np.where((idx >= 0)[..., None], pts.reshape(idx.shape + (pts.shape[-1],)), np.nan)


def sweep_topk(criteria: Sequence, Xs: np.ndarray, k: int, index_offset: int = 0, group=None, lift: Optional[Lift] = None):
    """As `sweep_argmax`, returning the k best candidates per criterion:
    (values (q, k), global indices (q, k), points (q, k, d)), identical on every rank.  `lift`: as in `sweep_argmax`."""
    c0 = criteria[0]
    model = c0.model
    if lift is not None:
        if _forest.is_forest_model(model):
            raise NotImplementedError("a lifted sweep (PCA-BO) serves a Gaussian process model, not a forest")
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        Xs = model._check_X(Xs)
        model.engine.upload_candidates(Xs, lazy=True)
        best, idx = _lifted_topk(criteria, model.engine, lift, int(k), group)
        return best, np.where(idx >= 0, idx + int(index_offset), -1), _topk_points(idx, lambda f: Xs[f], len(Xs))
    if _forest.is_forest_model(model):  # rows in the reference's format; points come back as q lists of k rows
        _forest._one_rank(group)
        return _forest.sweep_topk_host(criteria, Xs, k)
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    Xs = model._check_X(Xs)
    eng = model.engine
    ehvi = _ehvi_of(criteria, eng, group)
    con = _constrained_of(criteria, eng, group)
    eng.upload_candidates(Xs, lazy=True)  # (the sweep right below overlaps the copy with its first chunks)
    if ehvi is not None:
        best, idx = (a[None, :] for a in ehvi.sweep(k=int(k)))
    elif con is not None:
        best, idx = _constrained_topk(criteria, k)
    else:
        best, idx = eng.sweep_topk([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize, k)
    if getattr(eng, "comm_world", 0):
        return eng.exchange_topk(len(criteria), k, int(index_offset), True)
    xb = np.where((idx >= 0)[..., None], Xs[np.clip(idx, 0, len(Xs) - 1)], np.nan)
    gidx = np.where(idx >= 0, idx + int(index_offset), -1)
    return distributed.exchange_topk(best, gidx, xb, k, group=group)


def sweep_topk_generated(criteria: Sequence, bounds, M: int, k: int, seed: int, rank: int = 0, world: int = 1, group=None,
                         method: str = "uniform", lift: Optional[Lift] = None):
    """`sweep_topk` over M candidates generated on the device (`method` as in `sweep_generated`): rank r draws and sweeps
    its block of the design; (values (q, k), global rows (q, k), points (q, k, d)) are identical on every rank.  `lift`: as in
    `sweep_generated`."""
    c0 = criteria[0]
    model = c0.model
    if lift is not None:
        if _forest.is_forest_model(model):
            raise NotImplementedError("a lifted sweep (PCA-BO) serves a Gaussian process model, not a forest")
        if world > 1:
            raise NotImplementedError("a lifted sweep (PCA-BO) runs on one rank (no multi-rank exchange of penalised winners)")
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        eng = model.engine
        _generate(eng, bounds, int(M), seed, 0, method, int(M))
        best, idx = _lifted_topk(criteria, eng, lift, int(k), group)
        return best, idx, _topk_points(idx, eng.read_candidates, int(M))
    if _forest.is_forest_model(model):  # `bounds` is the mixed search space; points come back as q lists of k rows in its format
        _forest._one_rank(group, rank, world)
        if method != "uniform":
            raise NotImplementedError("method=%r: a forest model on a mixed space takes the uniform design only" % method)
        return _forest.sweep_topk_device(criteria, bounds, int(M), int(k), seed)
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    a, b_ = shard_bounds(int(M), rank, world)
    eng = model.engine
    ehvi = _ehvi_of(criteria, eng, group)
    con = _constrained_of(criteria, eng, group)
    _generate(eng, bounds, b_ - a, seed, a, method, int(M))
    if ehvi is not None:
        best, idx = (v[None, :] for v in ehvi.sweep(k=int(k)))
    elif con is not None:
        best, idx = _constrained_topk(criteria, k)
    else:
        best, idx = eng.sweep_topk([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize, k)
    if getattr(eng, "comm_world", 0):
        return eng.exchange_topk(len(criteria), k, a, True)
    flat = np.clip(idx, 0, b_ - a - 1).ravel()
    xb = np.where((idx >= 0)[..., None], eng.read_candidates(flat).reshape(idx.shape + (eng.d,)), np.nan)
    gidx = np.where(idx >= 0, idx + a, -1)
    return distributed.exchange_topk(best, gidx, xb, k, group=group)


def batch_argmax(criteria: Sequence, search_space, eval_budget: int, history: Optional[np.ndarray] = None, k: int = 8,
                 index_offset: Optional[int] = None, group=None, Xs: Optional[np.ndarray] = None, design: Optional[str] = None,
                 seed: Optional[int] = None, rank: Optional[int] = None, world: Optional[int] = None, masks=None, values=None,
                 h: Optional[Callable] = None, g: Optional[Callable] = None, strategy: str = "topk"):
    """The q-point proposal of `ParallelBO._batch_arg_max_acquisition` (bayes_opt.py:100-115) in ONE posterior pass:
    q criteria (same model; they differ only in t / alpha) share (mu, MSE); each takes its best candidate that is
    neither already taken by an earlier criterion nor `np.isclose` to an evaluated point in `history`
    (BO.pre_eval_check, bayes_opt.py:27-55) -- falling back through its top-k instead of the reference's random
    padding (base.py:282-289).  Returns (xopt: tuple of q lists, fopt: tuple of q floats) like the reference.
    `design` = "uniform" | "LHS" | "sobol" draws the `eval_budget` candidates on the device (rank r of `world` its block
    of ONE design); otherwise every rank sweeps its own host sample (`search_space.sample`, or `Xs`) and the union of the
    world x eval_budget points competes.  `masks` / `values` (ask(fixed=...), utils.py:184-213): `search_space` spans the
    free variables only, the fixed columns are filled in for the model, `history` holds full points, and the returned
    points hold the free variables (the caller's `fillin_fixed_value` completes them, base.py:476).  `h` / `g` (constraints
    over the free variables, one point as a list): only host-sampled candidates the reference would accept as a restart's
    outcome (`feasible_rows`) enter the sweep; with none, `((), ())` -- the reference's "no feasible restart" answer.
    `strategy`: "topk" (the above) or "believer" -- `believer_batch`: criterion j is maximised on the variance conditioned on
    the winners before it, and a row that is a winner does not compete again: the q points differ by construction.  `history`
    and `k` are not used then: a winner `np.isclose` to an evaluated point is left to the caller's padding, as the last
    fall-back above is.  "thompson" -- `thompson_batch`: one posterior sample path per criterion, each minimised (maximised) over
    the candidates as the criteria's `minimize` says; the criteria supply model and direction, their kind is not used, and
    `history` and `k` keep their meaning above."""
    if strategy == "thompson":
        criteria = list(criteria)
        return thompson_batch(criteria[0].model, search_space, eval_budget, len(criteria), Xs=Xs, design=design, seed=seed, history=history,
                              k=k, minimize=criteria[0].minimize, masks=masks, values=values, h=h, g=g, group=group, rank=rank, world=world,
                              criteria=criteria)  # fmt: skip
    if strategy == "believer":
        xs, fs = believer_batch(list(criteria), search_space, eval_budget, Xs=Xs, design=design, seed=seed, masks=masks, values=values,
                                h=h, g=g, group=group, rank=rank, world=world)
        return xs, fs
    if strategy != "topk":
        raise ValueError("strategy must be 'topk', 'believer' or 'thompson', not %r" % (strategy,))
    if _forest.is_forest_model(criteria[0].model):
        _forest.check_optimizer("sweep", h, g, masks)
        _forest._one_rank(group, rank, world)
        return _forest.batch_argmax(criteria, search_space, eval_budget, history=history, k=k, design=design, seed=seed, Xs=Xs)
    if rank is None or world is None:
        rank, world = engine_rank_world(criteria[0].model.engine, group)
    if design is not None:  # "uniform" | "LHS" | "sobol": the candidates are drawn on the GPU(s) and never touch the host
        if int(eval_budget) < world:  # (only ONE design is sharded; on the host-sampled path every rank draws its own eval_budget rows)
            raise ValueError("%d candidates cannot be sharded over %d ranks (every rank must own at least one)" % (eval_budget, world))
        if masks is not None or h is not None or g is not None:
            raise NotImplementedError("device-generated designs take neither fixed variables nor constraints")
        seed = int(np.random.randint(0, 2**62)) if seed is None else int(seed)
        vals, gidx, pts = sweep_topk_generated(criteria, search_space, int(eval_budget), k, seed, rank, world, group, design)
    else:
        if Xs is None:
            Xs = np.asarray(search_space.sample(int(eval_budget), method="uniform"), dtype=float)
        if h is not None or g is not None:
            if world > 1:
                raise NotImplementedError("a constrained sweep runs on one rank (a shard without feasible rows cannot join the exchange)")
            Xs = np.asarray(Xs, dtype=float)[feasible_rows(np.asarray(Xs, dtype=float), h, g)]
            if len(Xs) == 0:
                return (), ()
        full = np.asarray(Xs, dtype=float)
        if masks is not None:
            full = np.empty((len(Xs), len(masks)))
            full[:, ~masks] = Xs
            full[:, masks] = np.asarray(values, dtype=float)
        off = rank * len(full) if index_offset is None else int(index_offset)
        vals, gidx, pts = sweep_topk(criteria, full, k, index_offset=off, group=group)
    chosen_x, chosen_f, taken = [], [], set()
    hist = None if history is None or len(history) == 0 else np.asarray(history, dtype=float)
    for c in range(len(criteria)):
        pick = None
        for r in range(k):
            gi = int(gidx[c, r])
            if gi < 0 or gi in taken:
                continue
            if hist is not None and np.any(np.all(np.isclose(hist, pts[c, r]), axis=1)):
                continue
            pick = r
            break
        if pick is None:  # every fall-back exhausted: keep the argmax (the caller's duplicate check will pad)
            pick = 0
        taken.add(int(gidx[c, pick]))
        x = np.asarray(pts[c, pick], dtype=float)
        chosen_x.append((x[~masks] if masks is not None else x).tolist())
        chosen_f.append(float(vals[c, pick]))
    return tuple(chosen_x), tuple(chosen_f)


def _stage_candidates(model, search_space, eval_budget, Xs, design, seed):
    """The candidates of a believer or Thompson batch onto the model's engine: `design` drawn on the device (a missing seed from
    NumPy's global stream, drawn here and only then), else the rows `Xs` or `eval_budget` rows of `search_space.sample`."""
    eng = model.engine
    if design is not None:
        seed = int(np.random.randint(0, 2**62)) if seed is None else int(seed)
        _generate(eng, search_space, int(eval_budget), seed, 0, design, int(eval_budget))
    else:
        if Xs is None:
            Xs = np.asarray(search_space.sample(int(eval_budget), method="uniform"), dtype=float)
        eng.upload_candidates(model._check_X(Xs), lazy=True)


def _believer_preamble(model, lift, masks, h, g, group, rank, world, under="", no_front=None):
    """What every believer batch refuses alike, in the order all four keep: a forest, a lift, fixed variables, constraints h / g,
    a criterion without a front (`no_front`: that ValueError's message, None where the criterion has one), a model that is not
    fitted, several ranks.
    `under`: the family's wording behind "have no believer batches".  Returns the model's engine."""
    if _forest.is_forest_model(model):
        raise NotImplementedError("the Kriging believer conditions a Gaussian process: a forest model has no believer batches")
    if lift is not None:
        raise NotImplementedError("a lift (PCA-BO) has no believer batches" + under)
    if masks is not None and np.any(masks):
        raise NotImplementedError("fixed variables have no believer batches" + under)
    if h is not None or g is not None:
        if under:
            raise NotImplementedError("cheap constraints h / g have no believer batches%s: model them as columns of y" % under)
        raise NotImplementedError("constraints have no believer batches")
    if no_front is not None:
        raise ValueError(no_front)
    if getattr(model, "_committed_par", None) is None:
        raise Exception("The model is not fitted yet!")
    eng = model.engine
    if rank is None or world is None:
        rank, world = engine_rank_world(eng, group)
    if world > 1:
        raise NotImplementedError("the Kriging believer runs on one rank (every step depends on the winner before it)")
    return eng


def _believed_cap(q, pending):  # (behind each family's own checks of its criteria and of q, so not part of the preamble)
    if q + (0 if pending is None else len(pending)) > _lib.MAX_BELIEVED:
        raise ValueError("at most %d points are believed in one call (q + pending)" % _lib.MAX_BELIEVED)


def _believer_result(out):
    """(xopt: tuple of q lists, fopt: tuple of q floats) of an engine's believer dict, in `batch_argmax`'s format."""
    return tuple(np.asarray(x, dtype=float).tolist() for x in out["best_x"]), tuple(float(v) for v in out["best_val"])


def believer_batch(criteria, search_space, eval_budget: int, q: Optional[int] = None, Xs: Optional[np.ndarray] = None,
                   design: Optional[str] = None, seed: Optional[int] = None, pending=None, believe_plugin: bool = True, lift=None,
                   masks=None, values=None, h: Optional[Callable] = None, g: Optional[Callable] = None, group=None, rank=None, world=None):
    """A q-point proposal by the Kriging believer (Ginsbourger et al. 2010; `bogp_sweep_believer`): ONE posterior pass, then one
    streaming pass over the candidates per proposed point.  Step j maximises criterion j on the posterior mean and on the
    variance conditioned on `pending` (rows submitted but not yet evaluated, (n, d)) and on the winners of the steps before it
    -- believed at their predicted mean, which leaves the mean as it is.  `criteria`: one criterion (replicated `q` times; EI
    and EpsilonPI serve as well as MGFI and UCB) or a sequence used in order (same model, minimize and plugin).  With
    `believe_plugin` the plugin of a step is the best of the criterion's own and the believed means.  The candidates are
    `eval_budget` rows of `search_space.sample`, the rows `Xs`, or -- `design` = "uniform" | "LHS" | "sobol" -- drawn on the
    device, as in `batch_argmax`.  Returns (xopt: tuple of q lists, fopt: tuple of q floats) in `batch_argmax`'s format.
    Refused (NotImplementedError): a forest model, EHVI, a lift, fixed variables, constraints, more than one rank."""
    if hasattr(criteria, "acq_id") or is_ehvi(criteria) or not isinstance(criteria, (list, tuple)):
        criteria = [criteria] * int(1 if q is None else q)
    else:
        criteria = list(criteria)
        if q is not None and int(q) != len(criteria):
            raise ValueError("q = %d but %d criteria were given" % (q, len(criteria)))
    if len(criteria) == 0:
        raise ValueError("the believer needs at least one criterion")
    c0 = criteria[0]
    model = c0.model
    if _forest.is_forest_model(model):  # (here too: in front of the refusals of the criteria's kinds, which the preamble follows)
        raise NotImplementedError("the Kriging believer conditions a Gaussian process: a forest model has no believer batches")
    if any(is_constrained_ehvi(c) for c in criteria):
        raise NotImplementedError("%s has no believer batches" % _CEHVI)
    if any(is_ehvi(c) for c in criteria):
        raise NotImplementedError("EHVI has no believer batches: the front and its cells change with each believed point "
                                  "(`ehvi_believer_batch` rebuilds them between the steps)")
    if any(is_constrained(c) for c in criteria):
        raise NotImplementedError("modelled constraints (bogp.Constrained) have no believer batches: strategy='topk' serves them")
    eng = _believer_preamble(model, lift, masks, h, g, group, rank, world)
    plugins = {c.effective_plugin() for c in criteria if c.acq_id != _lib.ACQ_UCB}  # (UCB reads no plugin: it may join any batch)
    if any(c.model is not model or c.minimize != c0.minimize for c in criteria[1:]) or len(plugins) > 1:
        raise ValueError("criteria sharing one sweep must share model, minimize and plugin")
    plugin = plugins.pop() if plugins else 0.0
    _believed_cap(len(criteria), pending)
    _stage_candidates(model, search_space, eval_budget, Xs, design, seed)
    pend = None if pending is None or len(pending) == 0 else model._check_X(pending)
    out = eng.sweep_believer([(c.acq_id, c.acq_par()) for c in criteria], plugin, c0.minimize, pending=pend,
                             believe_plugin=believe_plugin)
    return _believer_result(out)


def _thompson_preamble(model, lift, masks, h, g, state_of, q, k, under=""):
    """What both Thompson batches refuse alike behind their refusals of the criterion's kind, in the order both keep: a lift, fixed
    variables, constraints h / g, what `state_of` refuses of the model, q < 1.  `under`: the family's wording behind "have no
    Thompson batches".  Returns (the model's state, q, k)."""
    if lift is not None:
        raise NotImplementedError("a lift (PCA-BO) has no Thompson batches" + under)
    if masks is not None and np.any(masks):
        raise NotImplementedError("fixed variables have no Thompson batches" + under)
    if h is not None or g is not None:
        if under:
            raise NotImplementedError("cheap constraints h / g have no Thompson batches%s: model them as columns of y" % under)
        raise NotImplementedError("constraints have no Thompson batches")
    st = state_of(model)
    q, k = int(q), int(k)
    if q < 1:
        raise ValueError("q = %d: Thompson sampling proposes at least one point" % q)
    return st, q, k


def _thompson_stage(model, search_space, eval_budget, Xs, design, seed, history, group, rank, world):
    """Behind every check of the arguments: one rank only, the candidates onto the engine.  Returns (engine, history rows or None)."""
    eng = model.engine
    if rank is None or world is None:
        rank, world = engine_rank_world(eng, group)
    if world > 1:
        raise NotImplementedError("Thompson batches run on one rank (the paths of a call share one candidate set)")
    _stage_candidates(model, search_space, eval_budget, Xs, design, seed)
    return eng, None if history is None or len(history) == 0 else np.asarray(history, dtype=float)


def _thompson_picks(sizes, seed, k, hist, call):
    """The calls of a Thompson batch (`sizes` members each, seeds derived from `seed`) and every member's pick: its first candidate
    that no earlier member took and that is not `np.isclose` to a row of `hist`.  `call(qb, sd, kk)` runs one call and returns (what
    is yielded back, per member ([(row, x, tag)] in order, the candidate kept with an empty list)).  Yields (that, member, candidate)."""
    from . import thompson as _th

    taken = set()
    for qb, sd in zip(sizes, _th.batch_seeds(seed, len(sizes))):
        kk = int(max(1, min(_lib.MAX_TOPK, k + len(taken))))  # a later call also steps over the rows the earlier ones took
        back, members = call(qb, sd, kk)
        for c, (cands, kept) in enumerate(members):
            free = (e for e in cands if e[0] not in taken and not (hist is not None and np.any(np.all(np.isclose(hist, e[1]), axis=1))))
            pick = next(free, cands[0] if cands else kept)  # every fall-back exhausted: the first listed row (the caller's check will pad)
            taken.add(pick[0])
            yield back, c, pick


def thompson_batch(model, search_space, eval_budget: int, q: int, n_features: int = 1024, seed: Optional[int] = None,
                   Xs: Optional[np.ndarray] = None, design: Optional[str] = None, history: Optional[np.ndarray] = None, k: int = 8,
                   minimize: bool = True, lift=None, masks=None, values=None, h: Optional[Callable] = None, g: Optional[Callable] = None,
                   group=None, rank=None, world=None, criteria=None):
    """A q-point proposal by Thompson sampling (`bogp_sweep_thompson`): q posterior sample paths of `model` (`bogp.thompson`:
    pathwise conditioning on `n_features` random Fourier features), each minimised -- maximised with `minimize=False` -- over the
    candidates.  ONE producer pass and one streaming pass serve 16 paths; the variance contraction never runs.  The candidates
    are set as in `believer_batch` (`eval_budget` rows of `search_space.sample`, the rows `Xs`, or a `design` drawn on the
    device).  Every path returns its `k` best rows and takes the first one that no earlier path took and that is not `np.isclose`
    to a row of `history` (`batch_argmax`'s rule), so the q proposals are q distinct rows.  More than 16 paths run in calls of 16
    with seeds derived from `seed` (`thompson.batch_seeds`).  Returns (xopt: tuple of q lists, fopt: tuple of q floats) in
    `batch_argmax`'s format; fopt is the path's value at its proposal.
    Refused (NotImplementedError): a forest model, EHVI / several targets, a lift, fixed variables, constraints, polynomial
    trends, more than one rank, the cubic and generalized-exponential kernels, the noisy and noise-estimating modes."""
    from . import thompson as _th

    if _forest.is_forest_model(model):
        raise NotImplementedError("Thompson sampling draws paths of a Gaussian process: a forest model has no Thompson batches")
    if criteria is not None and any(is_constrained_ehvi(c) for c in criteria):
        raise NotImplementedError("%s has no Thompson batches" % _CEHVI)
    if criteria is not None and any(is_ehvi(c) for c in criteria):
        raise NotImplementedError("EHVI / several targets have no Thompson batches")
    if criteria is not None and any(is_constrained(c) for c in criteria):
        raise NotImplementedError("modelled constraints (bogp.Constrained) have no Thompson batches: strategy='topk' serves them")
    _, q, k = _thompson_preamble(model, lift, masks, h, g, _th.state_of, q, k)  # (state_of: not fitted, mode, trend, targets, kernel)
    eng, hist = _thompson_stage(model, search_space, eval_budget, Xs, design, seed, history, group, rank, world)

    def call(qb, sd, kk):  # a path lists its ranks in order; every fall-back exhausted, it keeps the argmax
        out = eng.sweep_thompson(_th.draw(model, qb, n_features, sd), minimize=minimize, k=kk)
        idx, bx = out["best_idx"], out["best_x"]
        return out, [([(int(idx[c, r]), bx[c, r], r) for r in range(kk) if idx[c, r] >= 0], (int(idx[c, 0]), bx[c, 0], 0)) for c in range(qb)]

    chosen_x, chosen_f = [], []
    sizes = [min(_th.MAX_PATHS, q - a) for a in range(0, q, _th.MAX_PATHS)]
    for out, c, (_, x, r) in _thompson_picks(sizes, seed, k, hist, call):
        chosen_x.append(np.asarray(x, dtype=float).tolist())
        v = float(out["best_val"][c, r])
        chosen_f.append(-v if minimize else v)
    return tuple(chosen_x), tuple(chosen_f)


def constrained_thompson_batch(criterion, search_space, eval_budget: int, q: int, n_features: int = 1024, seed: Optional[int] = None,
                               Xs: Optional[np.ndarray] = None, design: Optional[str] = None, history: Optional[np.ndarray] = None,
                               k: int = 8, lift=None, masks=None, values=None, h: Optional[Callable] = None,
                               g: Optional[Callable] = None, group=None, rank=None, world=None):
    """A q-point proposal under modelled constraints by Thompson sampling (`bogp_sweep_thompson_constrained`; Eriksson & Poloczek
    2021): per proposed point ONE joint draw of the objective and the constraints of `criterion.model` (`bogp.thompson`:
    `draw_multi`, independent weights over shared random Fourier features), and among the candidates the best objective value where
    the DRAWN constraints hold -- the least violating row (largest excess over a bound in units of that constraint's prior standard
    deviation) where they hold nowhere, so a run without a feasible observation needs no other criterion.  `criterion`: one
    `bogp.Constrained`; it supplies model, `lo`, `hi` and `minimize` -- its `fun` is not used, and a feasibility-only criterion is
    served as any other.  ONE producer pass and one streaming pass serve `16 // m` members (m targets); more run in further calls
    with seeds derived from `seed` (`thompson.batch_seeds`).  Candidates as in `believer_batch`.  Every member lists its `k` best
    rows (`thompson.merge_ranks`: feasible rows first) and takes the first that no earlier member took and that is not `np.isclose`
    to a row of `history` (`thompson_batch`'s rule), so the q proposals are q distinct rows.  Returns (xopt: tuple of q lists, fopt:
    tuple of q floats) in `batch_argmax`'s format; fopt is the objective path's value at the proposal (for a least violating row:
    that row of the dense restatement, `thompson.objective_path_at`).
    TypeError: a criterion that is not `bogp.Constrained`.  Refused (NotImplementedError): `ConstrainedEHVI`, a forest model, a
    lift, fixed variables, cheap constraints h / g, more than one rank, and what `thompson.state_of_multi` refuses of the model."""
    from . import thompson as _th

    if is_constrained_ehvi(criterion):
        raise NotImplementedError("%s has no Thompson batches: constrained_thompson_batch takes one objective" % _CEHVI)
    if not is_constrained(criterion):
        raise TypeError("constrained_thompson_batch takes one bogp.Constrained criterion (a model alone goes to thompson_batch)")
    model = criterion.model
    if _forest.is_forest_model(model):
        raise NotImplementedError("Thompson sampling draws paths of a Gaussian process: a forest model has no Thompson batches")
    st, q, k = _thompson_preamble(model, lift, masks, h, g, _th.state_of_multi, q, k, " under modelled constraints")  # (the model's among them)
    if k < 1:
        raise ValueError("k = %d: every member lists at least one row" % k)
    eng, hist = _thompson_stage(model, search_space, eval_budget, Xs, design, seed, history, group, rank, world)
    minimize = bool(criterion.minimize)

    def call(qb, sd, kk):  # a member lists `merge_ranks`; with an empty list it keeps the first B rank
        dr = _th.draw_multi(model, qb, n_features, sd)
        out = eng.sweep_thompson_constrained(dr, qb, criterion.lo, criterion.hi, minimize=minimize, k=kk)
        idx, bx = out["best_idx"], out["best_x"]
        return (out, dr), [([(gi, bx[c, which, r], (which, r)) for gi, which, r in _th.merge_ranks(out["best_val"][c], idx[c], kk)],
                            (int(idx[c, 1, 0]), bx[c, 1, 0], (1, 0))) for c in range(qb)]  # fmt: skip

    chosen_x, chosen_f = [], []
    per_call = _th.MAX_PATHS // st.y.shape[1]
    sizes = [min(per_call, q - a) for a in range(0, q, per_call)]
    for (out, dr), c, (_, x, (which, r)) in _thompson_picks(sizes, seed, k, hist, call):
        chosen_x.append(np.asarray(x, dtype=float).tolist())
        if which == 0:  # an A rank is the objective path's value in the criterion's sign
            v = float(out["best_val"][c, 0, r])
            chosen_f.append(-v if minimize else v)
        else:  # a least violating row: its objective value is in no ranking -- one row of the restatement on the device's g
            chosen_f.append(_th.objective_path_at(st, dr, out["coef"], c, x))
    return tuple(chosen_x), tuple(chosen_f)


def ehvi_believer_batch(criterion, search_space, eval_budget: int, q: int, Xs: Optional[np.ndarray] = None, design: Optional[str] = None,
                        seed: Optional[int] = None, pending=None, believe_front: bool = True, lift=None, masks=None, values=None,
                        h: Optional[Callable] = None, g: Optional[Callable] = None, group=None, rank=None, world=None):
    """A q-point proposal for a multi-objective run by the Kriging believer under EHVI (`bogp_sweep_believer_ehvi`): what the
    reference's `MOBO` names and leaves open (mobo.py:168-178).  ONE posterior pass, then one streaming pass over the
    candidates per proposed point: step j maximises EHVI on the m posterior means and on the variances conditioned on `pending`
    (rows submitted but not yet evaluated, (n, d)) and on the winners of the steps before it, over the cells of the front --
    which, with `believe_front`, every believed mean joins before the next step (without it only the variance is conditioned).
    `criterion`: a `bogp.EHVI` built with `Y=` or `partitioning=`, so that it carries its front (`pareto_Y`); one built from
    `cells=` has no front to extend and is refused (ValueError).  Candidates as in `believer_batch`.  Returns (xopt: tuple of q
    lists, fopt: tuple of q floats) in `believer_batch`'s format.
    Refused (NotImplementedError): a forest model, a lift, fixed variables, constraints, more than one rank."""
    if is_constrained_ehvi(criterion):
        raise NotImplementedError("%s has no believer batches: ehvi_believer_batch conditions the objectives only and would drop "
                                  "the constraints" % _CEHVI)  # fmt: skip
    if not is_ehvi(criterion):
        raise TypeError("ehvi_believer_batch takes a bogp.EHVI criterion (the single-objective criteria go to believer_batch)")
    model = criterion.model
    no_front = None
    if getattr(criterion, "pareto_Y", None) is None:
        no_front = "an EHVI built from cells= has no front to extend with the believed means: build it with Y= or partitioning="
    eng = _believer_preamble(model, lift, masks, h, g, group, rank, world, no_front=no_front)
    q = int(q)
    if q < 1:
        raise ValueError("q = %d: the believer proposes at least one point" % q)
    _believed_cap(q, pending)
    _stage_candidates(model, search_space, eval_budget, Xs, design, seed)
    pend = None if pending is None or len(pending) == 0 else model._check_X(pending)
    out = eng.sweep_believer_ehvi(np.asarray(criterion.pareto_Y, dtype=float).reshape(-1, criterion.n_obj), criterion.ref_point, q,
                                  pending=pend, believe_front=believe_front)
    return _believer_result(out)


def constrained_believer_batch(criteria, search_space, eval_budget: int, q: Optional[int] = None, Xs: Optional[np.ndarray] = None,
                               design: Optional[str] = None, seed: Optional[int] = None, pending=None, believe_plugin: bool = True,
                               lift=None, masks=None, values=None, h: Optional[Callable] = None, g: Optional[Callable] = None, group=None,
                               rank=None, world=None):
    """A q-point proposal under modelled constraints by the Kriging believer (`bogp_sweep_believer_constrained`): ONE posterior
    pass over the m targets, then one streaming pass over the candidates per proposed point.  Step j maximises criterion j -- its
    criterion on the objective times the constraints' probabilities of feasibility -- on the m posterior means and on the variances
    conditioned on `pending` (rows submitted but not yet evaluated, (n, d)) and on the winners of the steps before it.  `criteria`:
    one `bogp.Constrained` (replicated `q` times) or a sequence used in order, sharing model, bounds, minimize and plugin; a
    feasibility-only step stays feasibility-only.  With `believe_plugin` a believed point whose believed constraint values all
    lie inside their bounds lowers the plugin of the later steps; an infeasible one leaves it.  Candidates as in `believer_batch`.
    Returns (xopt: tuple of q lists, fopt: tuple of q floats) in `believer_batch`'s format.
    TypeError: a criterion that is not `bogp.Constrained`.  Refused (NotImplementedError): a forest model, a lift, fixed
    variables, cheap constraints h / g, more than one rank."""
    if is_constrained(criteria) or not isinstance(criteria, (list, tuple)):
        criteria = [criteria] * int(1 if q is None else q)
    else:
        criteria = list(criteria)
        if q is not None and int(q) != len(criteria):
            raise ValueError("q = %d but %d criteria were given" % (q, len(criteria)))
    if len(criteria) == 0:
        raise ValueError("the believer needs at least one criterion")
    if any(is_constrained_ehvi(c) for c in criteria):
        raise NotImplementedError("%s has no believer batches: constrained_believer_batch takes one objective" % _CEHVI)
    if not all(is_constrained(c) for c in criteria):
        raise TypeError("constrained_believer_batch takes bogp.Constrained criteria (the single-objective criteria go to believer_batch, "
                        "EHVI to ehvi_believer_batch)")  # fmt: skip
    c0 = criteria[0]
    model = c0.model
    eng = _believer_preamble(model, lift, masks, h, g, group, rank, world, under=" under modelled constraints")
    for c in criteria[1:]:
        if (c.model is not model or c.minimize != c0.minimize or c.effective_plugin() != c0.effective_plugin()
                or not np.array_equal(c.lo, c0.lo) or not np.array_equal(c.hi, c0.hi)):  # fmt: skip
            raise ValueError("Constrained criteria sharing one sweep must share model, bounds, plugin and minimize")
    _believed_cap(len(criteria), pending)
    _stage_candidates(model, search_space, eval_budget, Xs, design, seed)
    pend = None if pending is None or len(pending) == 0 else model._check_X(pending)
    out = eng.sweep_believer_constrained([(c.acq_id, c.acq_par()) for c in criteria], c0.effective_plugin(), c0.minimize, c0.lo, c0.hi,
                                         pending=pend, believe_plugin=believe_plugin)
    return _believer_result(out)


def constrained_ehvi_believer_batch(criterion, search_space, eval_budget: int, q: int, Xs: Optional[np.ndarray] = None,
                                    design: Optional[str] = None, seed: Optional[int] = None, pending=None, believe_front: bool = True,
                                    lift=None, masks=None, values=None, h: Optional[Callable] = None, g: Optional[Callable] = None,
                                    group=None, rank=None, world=None):
    """A q-point proposal for a multi-objective run under modelled constraints by the Kriging believer
    (`bogp_sweep_believer_ehvi_constrained`): ONE posterior pass over the m + c targets, then one streaming pass over the candidates
    per proposed point.  Step j maximises EHVI of the objectives times the constraints' probabilities of feasibility on the
    posterior means and on the variances conditioned on `pending` (rows submitted but not yet evaluated, (n, d)) and on the
    winners of the steps before it, over the cells of the FEASIBLE front -- which, with `believe_front`, the objective part of a
    believed mean joins before the next step if and only if every believed constraint value lies inside its closed interval (a
    point infeasible by belief conditions the variances only).  A criterion without a feasible row (`feasibility_only`) stays the
    probability of feasibility alone for all q steps.
    `criterion`: a `bogp.ConstrainedEHVI` built with `Y=` or from the model's own rows; one built from `cells=` has no front to
    extend and is refused (ValueError).  Candidates as in `believer_batch`.  Returns (xopt: tuple of q lists, fopt: tuple of q
    floats) in `believer_batch`'s format.
    TypeError: a criterion that is not `bogp.ConstrainedEHVI`.  Refused (NotImplementedError): a forest model, a lift, fixed
    variables, cheap constraints h / g, more than one rank."""
    if not is_constrained_ehvi(criterion):
        raise TypeError("constrained_ehvi_believer_batch takes a %s criterion (EHVI goes to ehvi_believer_batch, bogp.Constrained to "
                        "constrained_believer_batch, the single-objective criteria to believer_batch)" % _CEHVI)  # fmt: skip
    model = criterion.model
    no_front = None
    if getattr(criterion, "from_cells", False):
        no_front = "a ConstrainedEHVI built from cells= has no front to extend with the believed means: build it with Y= or from the model's rows"
    eng = _believer_preamble(model, lift, masks, h, g, group, rank, world, under=" under constrained EHVI", no_front=no_front)
    q = int(q)
    if q < 1:
        raise ValueError("q = %d: the believer proposes at least one point" % q)
    _believed_cap(q, pending)
    _stage_candidates(model, search_space, eval_budget, Xs, design, seed)
    pend = None if pending is None or len(pending) == 0 else model._check_X(pending)
    m = criterion.n_obj
    feasibility_only = criterion.n_feasible == 0  # (no feasible observation; a feasible set below ref_point has the one cell)
    front = np.zeros((0, m)) if criterion.pareto_Y is None else np.asarray(criterion.pareto_Y, dtype=float).reshape(-1, m)
    out = eng.sweep_believer_ehvi_constrained(front, criterion.ref_point, q, criterion.lo, criterion.hi, pending=pend,
                                              believe_front=believe_front, feasibility_only=feasibility_only)
    return _believer_result(out)


def unwrap_criterion(obj):
    """Find the acquisition object behind what `BaseBO._create_acquisition` hands to `argmax_restart`
    (base.py:482-494): `partial_argument(functools.partial(criterion, return_dx=...), var_name, fixed)` -- a
    `functools.wraps` wrapper (utils.py:184-213).  Returns (criterion, masks, values): `masks` marks the variables
    the wrapper fills in with the fixed `values` (None when nothing is fixed or `obj` is the criterion itself)."""
    masks = values = None
    for _ in range(8):
        if (hasattr(obj, "acq_id") and hasattr(obj, "acq_par")) or is_ehvi(obj):
            return obj, masks, values
        if isinstance(obj, functools.partial):
            obj = obj.func
        elif hasattr(obj, "__wrapped__"):
            try:
                nl = inspect.getclosurevars(obj).nonlocals
                if "masks" in nl and np.any(nl["masks"]):
                    masks, values = np.asarray(nl["masks"], dtype=bool), list(nl["values"])
            except TypeError:
                pass
            obj = obj.__wrapped__
        else:
            break
    return None, None, None


def _lift_wrapper_parts(obj):
    """(inner acquisition callable, pca, bounds) of PCA-BO's wrapper (`PCABO._create_acquisition`, extension.py:121-133: a
    `functools.partial` of `penalized_acquisition` whose keywords hold `acquisition_func`, `bounds` and `pca`), else None."""
    kw = getattr(obj, "keywords", None) if isinstance(obj, functools.partial) else None
    if not kw or not all(k in kw for k in ("acquisition_func", "bounds", "pca")):
        return None
    return kw["acquisition_func"], kw["pca"], kw["bounds"]


def unwrap_lift(obj):
    """(criterion, lift) behind PCA-BO's penalising wrapper: this package's criterion the wrapper maximises (None when it
    wraps something else) and the `Lift` of its fitted PCA and original box.  (None, None) when `obj` is not that wrapper."""
    parts = _lift_wrapper_parts(obj)
    if parts is None:
        return None, None
    inner, pca, bounds = parts
    return unwrap_criterion(inner)[0], Lift.from_pca(pca, bounds)


def _lifted_argmax_restart(obj_func, search_space, h, g, eval_budget, optimizer):
    """`argmax_restart` for PCA-BO's wrapper under the sweep family: the candidates are rows of the reduced box
    `search_space`, swept under the wrapper's lift; the returned point is a reduced-space row (`PCABO.ask` maps it back
    itself, extension.py:151-152)."""
    inner = _lift_wrapper_parts(obj_func)[0]
    crit, masks, _ = unwrap_criterion(inner)
    if crit is None:
        raise TypeError("optimizer=%r needs one of this package's criteria behind PCA-BO's wrapper (a bogp.GaussianProcess as the "
                        "surrogate: construct the PCABO after bogp.install())" % optimizer)  # fmt: skip
    if optimizer in ("sweep-BFGS", "sweep-device-BFGS"):
        raise NotImplementedError("optimizer=%r under a lift (PCA-BO): the box penalty has no device polish; use 'sweep', "
                                  "'sweep-device[-lhs|-sobol]' or the reference's 'BFGS'" % optimizer)  # fmt: skip
    if masks is not None:
        raise NotImplementedError("a lifted sweep (PCA-BO) takes no fixed variables")
    if h is not None or g is not None:
        raise NotImplementedError("a lifted sweep (PCA-BO) takes no constraints h / g")
    if is_constrained_ehvi(crit):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not %s" % _CEHVI)
    if is_ehvi(crit):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not EHVI")
    if is_constrained(crit):
        raise NotImplementedError("a lifted sweep (PCA-BO) serves the single-objective criteria, not modelled constraints (bogp.Constrained)")
    if engine_rank_world(crit.model.engine)[1] > 1:
        raise NotImplementedError("a lifted sweep (PCA-BO) runs on one rank (no multi-rank exchange of penalised winners)")
    lift = unwrap_lift(obj_func)[1]
    if optimizer in DEVICE_DESIGNS:
        best, _, xb = sweep_generated([crit], search_space, int(eval_budget), int(np.random.randint(0, 2**62)),
                                      method=DEVICE_DESIGNS[optimizer], lift=lift)  # fmt: skip
    else:
        Xs = np.asarray(search_space.sample(int(eval_budget), method="uniform"), dtype=float)
        best, _, xb = sweep_argmax([crit], Xs, return_points=True, lift=lift)
    return np.asarray(xb[0], dtype=float).tolist(), float(best[0])


# optimizer name -> sampling method of RealSpace._sample (search_space.py:742-754) realised on the device
DEVICE_DESIGNS = {"sweep-device": "uniform", "sweep-device-lhs": "LHS", "sweep-device-sobol": "sobol"}


def _reference_argmax_restart():
    """The reference's own `argmax_restart` when `bayes_optim` is importable in this process (it is whenever a reference
    driver is the caller), read from its DEFINING module -- which no integration route re-points -- else None."""
    try:
        import importlib

        return importlib.import_module("bayes_optim.acquisition.optim").argmax_restart
    except Exception:
        return None


def argmax_restart(
    obj_func: Callable,
    search_space,
    h: Callable = None,
    g: Callable = None,
    eval_budget: int = 100,
    n_restart: int = 10,
    wait_iter: int = 3,
    optimizer: str = "BFGS",
    logger=None,
):
    """Same signature and return convention as the reference's `argmax_restart` (optim/__init__.py:55-153).

    optimizer="sweep": `obj_func` must be one of this package's acquisition objects; `eval_budget` candidates are
    drawn with `search_space.sample(N, "uniform")` and swept on the GPU.  With constraints `h` / `g`, only the sampled
    candidates the reference would accept as a restart's outcome (`feasible_rows`) are swept; `([], [])` when there is none.
    optimizer="sweep-device" / "sweep-device-lhs" / "sweep-device-sobol": the candidates (uniform / Latin hypercube /
    Sobol') are generated on the GPU and never touch the host.
    optimizer="sweep-BFGS" / "sweep-device-BFGS": the sweep's best `n_restart` candidates (host-sampled / drawn on the GPU)
    are polished together on the device (`polish_topk`: lock-step projected L-BFGS, one batched value + gradient call
    per iteration).
    optimizer="BFGS": the reference's multi-restart L-BFGS-B loop on `obj_func(x) -> (value, dx)` (host; every
    evaluation is one device call through the acquisition object).
    PCA-BO's wrapper (`unwrap_lift`) under "sweep" / "sweep-device[-lhs|-sobol]": the candidates are rows of the reduced box and
    are swept under the wrapper's lift (`sweep_argmax(..., lift=)`); the polish hybrids, fixed variables, constraints and
    several ranks are refused by name.
    A `bogp.Constrained` criterion (modelled constraints) is served under "sweep" and "sweep-device[-lhs|-sobol]" through
    `bogp_sweep_constrained`; "BFGS" and the "-BFGS" hybrids are refused by name (it has no input gradient) unless it was built with
    `input_gradient=True`: then "BFGS" is the loop on `bogp_point_eval_constrained` and the hybrids polish the sweep's best rows with
    `bogp_polish_constrained`; fixed variables, cheap callables h / g, a lift and several ranks are refused by name.
    A `bogp.ConstrainedEHVI` criterion is served under "sweep" and "sweep-device[-lhs|-sobol]" through `bogp_sweep_ehvi_constrained`;
    built with `input_gradient=True` also under "BFGS" (the loop on `bogp_point_eval_ehvi_constrained`) and the hybrids (the sweep's
    best rows polished with `bogp_polish_ehvi_constrained`); every other optimiser, fixed variables, cheap callables h / g, a lift and
    several ranks are refused by name.
    Anything else ("MIES", "OnePlusOne_Cholesky_CMA", constraints under "BFGS", a non-continuous space) is the
    reference's own business: the call is handed to its `argmax_restart` when `bayes_optim` is importable, for which a
    bogp criterion is an ordinary callable; without the reference, NotImplementedError.
    """
    ours = optimizer in DEVICE_DESIGNS or optimizer in ("sweep", "sweep-BFGS", "sweep-device-BFGS")
    if ours and _lift_wrapper_parts(obj_func) is not None:  # PCA-BO's penalising wrapper: the lifted sweep
        return _lifted_argmax_restart(obj_func, search_space, h, g, eval_budget, optimizer)
    fcrit, fmasks, _ = unwrap_criterion(obj_func)
    if fcrit is not None and _forest.is_forest_model(getattr(fcrit, "model", None)) and (ours or optimizer == "BFGS"):
        # a forest model (any space of Real / Integer / Ordinal / Discrete / Subset / Bool variables): "sweep" and "sweep-device"
        # are served, everything else this package knows is refused with the limitation named
        return _forest.argmax_restart(fcrit, search_space, eval_budget, optimizer, h=h, g=g, masks=fmasks)
    if is_constrained_ehvi(fcrit):  # served under "sweep" and "sweep-device[-lhs|-sobol]"; nothing else may drop its constraints
        # ConstrainedEHVI(input_gradient=True): "BFGS" is the loop below on the one-point call (bogp_point_eval_ehvi_constrained), the
        # hybrids are crit.sweep(k) + polish_topk (bogp_polish_ehvi_constrained)
        polishes = getattr(fcrit, "input_gradient", False) and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS")
        if optimizer not in DEVICE_DESIGNS and optimizer != "sweep" and not polishes:
            raise NotImplementedError("optimizer=%r for %s: it has no input gradient and no polish; use 'sweep' or "
                                      "'sweep-device[-lhs|-sobol]'" % (optimizer, _CEHVI))  # fmt: skip
        if not is_continuous(search_space):
            raise NotImplementedError("optimizer=%r for %s takes a continuous space" % (optimizer, _CEHVI))
        if fmasks is not None:
            raise NotImplementedError("optimizer=%r for %s takes no fixed variables" % (optimizer, _CEHVI))
        if h is not None or g is not None:
            raise NotImplementedError("optimizer=%r for %s takes no cheap constraints h / g: model them as columns instead" % (optimizer, _CEHVI))
        if engine_rank_world(fcrit.model.engine)[1] > 1:
            raise NotImplementedError("optimizer=%r for %s runs on one rank" % (optimizer, _CEHVI))
    if is_ehvi(fcrit) and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS") and is_continuous(search_space):
        if not getattr(fcrit, "input_gradient", False):
            raise NotImplementedError("optimizer=%r needs an input gradient, which EHVI does not have: use 'sweep' or "
                                      "'sweep-device[-lhs|-sobol]' (or build the criterion with input_gradient=True)" % optimizer)  # fmt: skip
        # EHVI(input_gradient=True): "BFGS" is the loop below on the one-point call (bogp_point_eval_ehvi), the hybrids are
        # ehvi.sweep(k) + polish_topk (bogp_polish_ehvi); fixed variables, constraints, a lift and several ranks are refused
        # by name where the single-objective polish hybrids refuse them
    if is_constrained(fcrit) and optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        if not getattr(fcrit, "input_gradient", False):
            raise NotImplementedError("optimizer=%r needs an input gradient, which the feasibility-weighted criterion (bogp.Constrained) "
                                      "does not have: use 'sweep' or 'sweep-device[-lhs|-sobol]'" % optimizer)  # fmt: skip
        # Constrained(input_gradient=True): "BFGS" is the loop below on the one-point call (bogp_point_eval_constrained), the hybrids are
        # crit.sweep(k) + polish_topk (bogp_polish_constrained); what the single-objective polish hybrids refuse is refused by name
        if not is_continuous(search_space):
            raise NotImplementedError("optimizer=%r for modelled constraints (bogp.Constrained) takes a continuous space" % optimizer)
        if fmasks is not None:
            raise NotImplementedError("optimizer=%r for modelled constraints (bogp.Constrained) takes no fixed variables" % optimizer)
        if h is not None or g is not None:
            raise NotImplementedError("optimizer=%r for modelled constraints (bogp.Constrained) takes no cheap constraints h / g: they "
                                      "would be dropped or filtered outside the polish; model them as columns instead" % optimizer)  # fmt: skip
        if engine_rank_world(fcrit.model.engine)[1] > 1:
            raise NotImplementedError("optimizer=%r for modelled constraints (bogp.Constrained) runs on one rank" % optimizer)
    if not ours and (optimizer != "BFGS" or h is not None or g is not None or not is_continuous(search_space)):
        ref = _reference_argmax_restart()
        if ref is None:
            raise NotImplementedError(
                "optimizer %r / constraints / non-continuous spaces are served by the reference's own argmax_restart "
                "(bayes_optim is not importable here); this package serves 'BFGS', 'sweep', 'sweep-device[-lhs|-sobol]' "
                "and 'sweep-BFGS' on continuous spaces" % optimizer)  # fmt: skip
        return ref(obj_func, search_space, h=h, g=g, eval_budget=eval_budget, n_restart=n_restart, wait_iter=wait_iter,
                   optimizer=optimizer, logger=logger)  # fmt: skip
    if optimizer == "sweep-device-BFGS":  # as "sweep-BFGS" with the candidates drawn on the GPU: nothing of size M on the host
        crit, masks, _ = unwrap_criterion(obj_func)
        if crit is None or masks is not None or h is not None or g is not None:
            raise NotImplementedError("optimizer=%r takes an unconstrained bogp criterion without fixed variables" % optimizer)
        rank, world = engine_rank_world(crit.model.engine)
        if int(eval_budget) < world:
            raise ValueError("%d candidates cannot be sharded over %d ranks" % (eval_budget, world))
        k = int(max(1, min(n_restart, 32, int(eval_budget))))
        tv, _, tx = sweep_topk_generated([crit], search_space, int(eval_budget), k, int(np.random.randint(0, 2**62)), rank, world)
        ok = np.isfinite(tv[0])
        if not ok.any():
            return [], []
        xp, fp = polish_topk(crit, tx[0][ok], np.array(search_space.bounds, dtype=float))
        j = int(np.argmax(fp))
        return xp[j].tolist(), float(fp[j])
    if optimizer in DEVICE_DESIGNS:  # candidates drawn on the GPU; the stream is seeded from the global np.random
        crit, masks, _ = unwrap_criterion(obj_func)
        if crit is None or masks is not None or h is not None or g is not None:
            raise NotImplementedError("optimizer=%r takes an unconstrained bogp criterion without fixed variables" % optimizer)
        rank, world = engine_rank_world(crit.model.engine)
        if int(eval_budget) < world:
            raise ValueError("%d candidates cannot be sharded over %d ranks" % (eval_budget, world))
        best, _, xb = sweep_generated([crit], search_space, int(eval_budget), int(np.random.randint(0, 2**62)), rank, world,
                                      method=DEVICE_DESIGNS[optimizer])  # fmt: skip
        return xb[0].tolist(), float(best[0])
    if ours:  # "sweep" | "sweep-BFGS": host-sampled candidates
        crit, masks, values = unwrap_criterion(obj_func)
        if crit is None:
            raise TypeError("optimizer=%r needs a bogp acquisition object (or the reference's wrapper around one)" % optimizer)
        Xs = np.asarray(search_space.sample(int(eval_budget), method="uniform"), dtype=float)
        # Under a communicator / process group every rank sweeps ITS OWN draw of `eval_budget` candidates (the union is
        # world x eval_budget points; global row = rank x eval_budget + local row) and the winner's POINT comes out of the
        # exchange, so that every rank returns the same (xopt, fopt) whatever its local sample was.
        rank, world = engine_rank_world(crit.model.engine)
        if h is not None or g is not None:
            if world > 1:
                raise NotImplementedError("a constrained sweep runs on one rank (a shard without feasible rows cannot join the exchange)")
            Xs = Xs[feasible_rows(Xs, h, g)]
            if len(Xs) == 0:
                return [], []  # what the reference returns when no restart ends feasible (optim/__init__.py:148-149)
        full = Xs
        if masks is not None:  # ask(fixed=...): the free columns are swept, the fixed ones are filled in
            full = np.empty((len(Xs), len(masks)))
            full[:, ~masks] = Xs
            full[:, masks] = np.asarray(values, dtype=float)
        if optimizer == "sweep":
            best, _, xb = sweep_argmax([crit], full, index_offset=rank * int(eval_budget), return_points=True)
            x = np.asarray(xb[0], dtype=float)
            return (x[~masks] if masks is not None else x).tolist(), float(best[0])
        # hybrid: the sweep picks the n_restart most promising candidates, which are then polished
        if masks is not None or h is not None or g is not None:
            raise NotImplementedError("optimizer='sweep-BFGS' takes an unconstrained bogp criterion without fixed variables")
        k = int(max(1, min(n_restart, 32, len(Xs))))
        tv, _, tx = sweep_topk([crit], Xs, k, index_offset=rank * int(eval_budget))
        ok = np.isfinite(tv[0])
        if not ok.any():
            return [], []
        xp, fp = polish_topk(crit, tx[0][ok], np.array(search_space.bounds, dtype=float))
        j = int(np.argmax(fp))
        return xp[j].tolist(), float(fp[j])

    xopt, fopt = [], []
    best = -np.inf
    wait_count = 0
    bounds = np.array(search_space.bounds)

    direct = hasattr(obj_func, "acq_id") or is_ehvi(obj_func)  # our criterion object itself; otherwise the reference's one-point wrapper

    def neg(x):  # Penalized without constraints (optim/__init__.py:45-52)
        x = np.asarray(x, dtype=float)
        f, fg = obj_func(x.reshape(1, -1), return_dx=True) if direct else obj_func(x)
        return -1.0 * float(np.asarray(f, float).ravel()[0]), -1.0 * np.asarray(fg, float).ravel()

    for iteration in range(n_restart):
        x0 = np.asarray(search_space.sample(N=1, method="uniform")[0], dtype=float)
        xopt_, fopt_, stop_dict = fmin_l_bfgs_b(neg, x0, pgtol=1e-8, factr=1e6, bounds=bounds, maxfun=eval_budget)
        xopt_ = xopt_.flatten().tolist()
        fopt_ = -float(fopt_)
        if fopt_ > best:
            best = fopt_
            wait_count = 0
        else:
            wait_count += 1
        eval_budget -= stop_dict["funcalls"]
        xopt.append(xopt_)
        fopt.append(fopt_)
        if eval_budget <= 0 or wait_count >= wait_iter:
            break
    if len(xopt) == 0:
        return [], []
    idx = np.argsort(fopt)[::-1]
    return xopt[idx[0]], fopt[idx[0]]


def polish_topk(crit, starts: np.ndarray, bounds: np.ndarray, max_iter: int = 50):
    """Local refinement of `starts` (k, d) inside the box `bounds` (d, 2); returns (points (k, d), values (k,)) with
    values[i] >= the criterion at starts[i].  On the device engine all k starts advance in lock step (`bogp_polish`:
    one batched value + gradient evaluation per iteration, the optimiser state never leaves the GPU; an EHVI criterion built
    with `input_gradient=True` goes to `bogp_polish_ehvi`, a Constrained one to `bogp_polish_constrained`, a ConstrainedEHVI one to
    `bogp_polish_ehvi_constrained`) -- the reference
    runs its restarts one after the other, one point per call (optim/__init__.py:74-153).  An engine without `polish`
    (the test stand-ins) or a model the fused call does not serve (polynomial trend basis) gets the reference-style
    sequential L-BFGS-B through the one-point call."""
    starts = np.atleast_2d(np.asarray(starts, dtype=float))
    bounds = np.asarray(bounds, dtype=float)
    model = crit.model
    eng = getattr(model, "engine", None)
    fused = getattr(model, "_fused_point_ok", None)
    if is_constrained_ehvi(crit) and not getattr(crit, "input_gradient", False):
        raise NotImplementedError("%s has no polish: bogp_polish_ehvi knows the objectives only and would drop the constraints" % _CEHVI)
    if is_constrained_ehvi(crit) and eng is not None and hasattr(eng, "polish_ehvi_constrained"):  # ConstrainedEHVI(input_gradient=True)
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        xs, fs, _ = eng.polish_ehvi_constrained(model._check_X(starts), bounds[:, 0], bounds[:, 1], crit.cell_lower_bounds,
                                                crit.cell_upper_bounds, crit.lo, crit.hi, max_evals=int(max_iter))  # fmt: skip
        return xs, fs
    if is_ehvi(crit) and not is_constrained_ehvi(crit) and eng is not None and hasattr(eng, "polish_ehvi"):  # EHVI(input_gradient=True): bogp_polish_ehvi
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        xs, fs, _ = eng.polish_ehvi(model._check_X(starts), bounds[:, 0], bounds[:, 1], crit.cell_lower_bounds, crit.cell_upper_bounds,
                                    max_evals=int(max_iter))  # fmt: skip
        return xs, fs
    if is_constrained(crit) and eng is not None and hasattr(eng, "polish_constrained"):  # Constrained(input_gradient=True)
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        xs, fs, _ = eng.polish_constrained(model._check_X(starts), bounds[:, 0], bounds[:, 1], (crit.acq_id, crit.acq_par()),
                                           crit.effective_plugin(), crit.minimize, crit.lo, crit.hi, max_evals=int(max_iter))  # fmt: skip
        return xs, fs
    if not is_ehvi(crit) and not is_constrained(crit) and eng is not None and hasattr(eng, "polish") and fused is not None and fused():  # (r05: any d up to BOGP_MAX_DIM; r03-r04 stopped at 64)
        if getattr(model, "_committed_par", None) is None:
            raise Exception("The model is not fitted yet!")
        xs, fs, _ = eng.polish(model._check_X(starts), bounds[:, 0], bounds[:, 1], (crit.acq_id, crit.acq_par()), crit.effective_plugin(),
                               crit.minimize, max_evals=int(max_iter))  # fmt: skip
        return xs, fs
    xs, fs = [], []
    for x0 in starts:
        def neg(x):
            f, fg = crit(np.asarray(x, dtype=float).reshape(1, -1), return_dx=True)
            return -1.0 * float(np.asarray(f, float).ravel()[0]), -1.0 * np.asarray(fg, float).ravel()

        f0 = -neg(x0)[0]
        x1, f1, _ = fmin_l_bfgs_b(neg, x0, pgtol=1e-8, factr=1e6, bounds=bounds, maxfun=max_iter)
        if -float(f1) >= f0:
            xs.append(np.asarray(x1, dtype=float).ravel()), fs.append(-float(f1))
        else:
            xs.append(x0), fs.append(f0)
    return np.array(xs), np.array(fs)
