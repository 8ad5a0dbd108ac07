"""Random-forest surrogate on the device: packing of a fitted forest, `bogp.RandomForest`, and the sweep over mixed spaces.

The reference's surrogate for every search space that is not a `RealSpace` is `RandomForest`
(`bayes_optim/surrogate/random_forest.py:63-155`): scikit-learn's regressor with the categorical columns one-hot encoded,
mu = mean over the trees, MSE = `std(ddof=1) ** 2` over the trees.  The trees are still fitted by scikit-learn on the host (the
caller's side, like scipy's L-BFGS-B in the default `tell`); everything after the fit runs in libbogp (`bogp_forest_*`,
csrc/kernels_forest.hip).  There is no CPU fallback for prediction.

  pack(model)            flat node arrays of anything shaped like a fitted RandomForestRegressor, plus the raw <-> encoded column map
                         of the reference's `_check_X` (:105-110); `multi_output=True` admits a forest fitted on y (N, m): one tree
                         structure, m values a leaf (what MOBO fits, mobo.py:155-160), served by `bogp_forest_*_multi` and, for
                         `bogp.EHVI`, `bogp_forest_sweep_ehvi` (csrc/kernels_forest_ehvi.hip)
  PackedForest.raw()     the same forest rewritten onto the RAW columns: a split of a one-hot column becomes `x[v] != level -> left`
                         on the column that holds the level index, so a mixed candidate stays d wide instead of d_enc wide
  RandomForest           scikit-learn's regressor with the reference's defaults; `predict(X, eval_MSE)` on the device
  device_of(model)       the engine holding a model's packed forest (re-packed after every fit)
  sweep_topk_host / sweep_topk_device / argmax_restart / batch_argmax: what `optim` routes a forest model to

scikit-learn is imported lazily (`RandomForest` is built on first access): the package imports without it.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import _lib

_SUPPORTED = "Real, Integer, Ordinal, Discrete, Subset or Bool"


class PackedForest:
    """Flat arrays of T trees in the forest's own (encoded) feature space, and the column map.

    tree_offset (T + 1), feature / left / right (int32), threshold / value (float64): scikit-learn's `tree_` arrays, concatenated;
    child indices are relative to their tree, a leaf has left == right == -1.  `value` is (nodes,) for one output (m = 1) and
    (nodes, m) for a forest with several outputs.
    d_raw, d_enc; noncat: raw indices of the non-categorical columns in order (encoded columns 0 .. len(noncat) - 1); cat_idx: raw
    indices of the categorical columns, sorted; categories[j]: the level labels of cat_idx[j], one encoded column each, block after
    block behind the non-categorical ones -- as `_check_X` builds them."""

    def __init__(self, tree_offset, feature, threshold, left, right, value, d_raw, noncat, cat_idx, categories):
        self.tree_offset, self.feature, self.threshold = tree_offset, feature, threshold
        self.left, self.right, self.value = left, right, value
        self.d_raw, self.noncat, self.cat_idx, self.categories = int(d_raw), list(noncat), list(cat_idx), [list(c) for c in categories]
        self.T = len(tree_offset) - 1
        self.m = int(value.shape[1]) if np.ndim(value) == 2 else 1
        # encoded column -> (raw column, level index or -1)
        self.enc_cols = [(v, -1) for v in self.noncat]
        for v, cats in zip(self.cat_idx, self.categories):
            self.enc_cols += [(v, l) for l in range(len(cats))]
        self.d_enc = len(self.enc_cols)
        self._lookup = [_label_lookup(c) for c in self.categories]

    @property
    def n_nodes(self) -> int:
        return int(self.tree_offset[-1])

    def raw(self):
        """(feature, threshold, test) on the raw columns: test 0 keeps `x <= threshold -> left`, test 1 is `x != threshold -> left`
        with threshold the level index (a one-hot column takes the values 0 and 1 only, so a split at 0 <= t < 1 sends the rows of
        every OTHER level left)."""
        inner = self.left >= 0
        f = np.where(inner, self.feature, 0)
        v = np.array([c[0] for c in self.enc_cols], dtype=np.int32)[f]
        lvl = np.array([c[1] for c in self.enc_cols], dtype=np.int64)[f]
        onehot = inner & (lvl >= 0)
        if np.any(onehot & ~((self.threshold >= 0) & (self.threshold < 1))):
            raise ValueError("a split of a one-hot column lies outside [0, 1): not a forest fitted on 0 / 1 columns")
        feature = np.where(inner, v, self.feature).astype(np.int32)
        threshold = np.where(onehot, lvl.astype(float), self.threshold)
        return feature, threshold, onehot.astype(np.int32)

    # -- rows ---------------------------------------------------------------------------------------------------------------------
    def _object_rows(self, X):
        X_ = np.array(X, dtype=object)
        if X_.ndim == 1:
            X_ = X_.reshape(1, -1)
        if X_.ndim != 2 or X_.shape[1] != self.d_raw:
            raise ValueError("rows must have %d columns" % self.d_raw)
        return X_

    def to_index(self, X) -> np.ndarray:
        """Rows in the reference's format (labels in the categorical columns) -> float (M, d_raw) with level INDICES there."""
        X_ = self._object_rows(X)
        out = np.empty(X_.shape, dtype=float)
        for v in self.noncat:
            out[:, v] = X_[:, v].astype(float)
        for j, v in enumerate(self.cat_idx):
            out[:, v] = [self._lookup[j](x) for x in X_[:, v]]
        return out

    def encode(self, X) -> np.ndarray:
        """What `_check_X` returns (random_forest.py:105-110): the non-categorical columns as floats, then one 0 / 1 column per level."""
        idx = self.to_index(X)
        out = np.zeros((len(idx), self.d_enc))
        for c, (v, l) in enumerate(self.enc_cols):
            out[:, c] = idx[:, v] if l < 0 else (idx[:, v] == l)
        return out

    def encode_index(self, Xi) -> np.ndarray:
        """Index rows (as `to_index` gives them, or as the device generates them) -> encoded rows."""
        Xi = np.asarray(Xi, dtype=float)
        out = np.zeros((len(Xi), self.d_enc))
        for c, (v, l) in enumerate(self.enc_cols):
            out[:, c] = Xi[:, v] if l < 0 else (Xi[:, v] == l)
        return out


def _label_lookup(cats):
    try:
        table = {c: i for i, c in enumerate(cats)}
    except TypeError:  # unhashable labels
        table = None

    def find(x):
        try:
            return table[x] if table is not None else list(cats).index(x)
        except (KeyError, ValueError, TypeError):
            for i, c in enumerate(cats):  # numpy scalars, tuples read back as arrays
                if np.array_equal(np.asarray(c, dtype=object), np.asarray(x, dtype=object)):
                    return i
            raise ValueError("unknown level %r (levels: %r)" % (x, list(cats))) from None

    return find


def n_outputs(model) -> int:
    """Outputs of a fitted forest (1 before the fit)."""
    return int(getattr(model, "n_outputs_", 1) or 1)


def pack(model, multi_output: bool = False) -> PackedForest:
    """Flat arrays of a fitted forest: anything with `estimators_[t].tree_` (`children_left`, `children_right`, `feature`,
    `threshold`, `value`) and, if present, the reference's `_cat_idx` / `_categories`.  A forest with several outputs is packed
    only on request (`multi_output=True`: `value` becomes (nodes, m) = `tree_.value[:, :, 0]`); the one-output entry points do not
    serve it."""
    est = getattr(model, "estimators_", None)
    if not est:
        raise ValueError("the forest is not fitted (no estimators_)")
    m = n_outputs(model)
    if m > 1 and not multi_output:
        raise NotImplementedError("forests with several outputs (n_outputs_ = %d) are not served by the one-output calls: "
                                  "pack(model, multi_output=True)" % m)
    if m > _lib.MAX_TARGETS:
        raise NotImplementedError("forests with several outputs: n_outputs_ = %d, at most %d are served" % (m, _lib.MAX_TARGETS))
    off, feat, thr, left, right, val = [0], [], [], [], [], []
    for e in est:
        t = e.tree_
        v = np.asarray(t.value, dtype=float)
        n = len(t.children_left)
        if m > 1:
            if v.shape != (n, m, 1):
                raise ValueError("tree_.value has shape %s, expected (%d, %d, 1)" % (v.shape, n, m))
        elif v.ndim > 1 and int(np.prod(v.shape[1:])) != 1:
            raise NotImplementedError("forests with several outputs are not served")
        off.append(off[-1] + n)
        feat.append(np.asarray(t.feature, dtype=np.int32))
        thr.append(np.asarray(t.threshold, dtype=float))
        left.append(np.asarray(t.children_left, dtype=np.int32))
        right.append(np.asarray(t.children_right, dtype=np.int32))
        val.append(v.reshape(n, m) if m > 1 else v.reshape(n))
    d_enc = int(getattr(model, "n_features_in_", 0) or (max(int(f.max()) for f in feat) + 1))
    cat_idx = list(getattr(model, "_cat_idx", []) or [])
    categories = list(getattr(model, "_categories", []) or []) if cat_idx else []
    d_raw = d_enc - sum(len(c) for c in categories) + len(cat_idx)
    noncat = [v for v in range(d_raw) if v not in set(cat_idx)]
    cat = np.concatenate
    return PackedForest(np.asarray(off, dtype=np.int64), cat(feat), cat(thr), cat(left), cat(right), cat(val), d_raw, noncat, cat_idx, categories)


def is_forest_model(model) -> bool:
    """True for a fitted-or-not forest surrogate: this package's `RandomForest`, the reference's, or scikit-learn's regressor."""
    return any(c.__name__ in ("RandomForest", "RandomForestRegressor") for c in type(model).__mro__)


class _Device:
    """The engine of one forest model, and the packed forest it currently holds."""

    def __init__(self, device=0):
        self.engine = _lib.Engine(device)
        self.packed: Optional[PackedForest] = None
        self.fitted_on = None

    def sync(self, model) -> "_Device":
        est = getattr(model, "estimators_", None)
        if not est:
            raise Exception("The model is not fitted yet!")
        if self.fitted_on is not est:  # a fit builds a new list
            p = pack(model, multi_output=True)
            f, t, test = p.raw()
            if p.m > 1:
                self.engine.forest_set_multi(p.d_raw, p.m, p.tree_offset, f, t, p.left, p.right, p.value, test)
            else:
                self.engine.forest_set(p.d_raw, p.tree_offset, f, t, p.left, p.right, p.value, test)
            self.engine.set_candidate_transform()
            self.packed, self.fitted_on = p, est
        return self


def device_of(model) -> _Device:
    dev = model.__dict__.get("_bogp_forest")
    if dev is None:
        dev = _Device(int(getattr(model, "device", 0) or 0))
        model.__dict__["_bogp_forest"] = dev
    return dev.sync(model)


def predict(model, X, eval_MSE=False):
    """`RandomForest.predict(X, eval_MSE)` (random_forest.py:124-155) of a fitted forest on the device: (M,) moments for one
    output, (M, m) for a forest fitted on y (N, m), as the reference returns them."""
    dev = device_of(model)
    dev.engine.upload_candidates(dev.packed.to_index(X))
    if dev.packed.m > 1:
        mu, mse = dev.engine.forest_predict_multi(eval_MSE=bool(eval_MSE))
    else:
        mu, mse = dev.engine.forest_predict(eval_MSE=bool(eval_MSE))
    return (mu, mse) if eval_MSE else mu


# ---------------------------------------------------------------------------------------------------------------------------------
# the surrogate class (built on first access: scikit-learn is imported lazily)
# ---------------------------------------------------------------------------------------------------------------------------------
_CLASS = None


def _build_class():
    from collections import OrderedDict

    from sklearn.ensemble import RandomForestRegressor

    class RandomForest(RandomForestRegressor):
        """`bayes_optim.surrogate.RandomForest` (random_forest.py:63-155) with prediction on the device: scikit-learn's regressor
        with the reference's defaults, categorical columns (`levels`: {column: labels}) one-hot encoded by comparison with the
        labels, mu / MSE over the trees from libbogp."""

        def __init__(self, n_estimators: int = 100, max_features: float = 5 / 6, min_samples_leaf: int = 2, levels: dict = None,
                     device: int = 0, **kwargs):
            super().__init__(n_estimators=n_estimators, max_features=max_features, min_samples_leaf=min_samples_leaf, **kwargs)
            levels = {} if levels is None else levels
            assert isinstance(levels, dict)
            self.levels = levels
            self.device = device
            self.is_fitted = False
            if self.levels:
                self._levels = OrderedDict(sorted(levels.items()))
                self._cat_idx = list(self._levels.keys())
                self._categories = [list(v) for v in self._levels.values()]

        def _column_map(self, d_raw) -> PackedForest:
            cat_idx = list(getattr(self, "_cat_idx", []))
            cats = list(getattr(self, "_categories", []))
            z = np.zeros(0, dtype=np.int32)
            return PackedForest(np.zeros(1, dtype=np.int64), z, np.zeros(0), z, z, np.zeros(0), d_raw,
                                [v for v in range(d_raw) if v not in set(cat_idx)], cat_idx, cats)

        def _check_X(self, X) -> np.ndarray:
            X_ = np.array(X, dtype=object)
            if X_.ndim == 1:
                X_ = X_.reshape(1, -1)
            return self._column_map(X_.shape[1]).encode(X_)

        def fit(self, X, y):
            y = np.asarray(y, dtype=float)
            if y.ndim == 2 and y.shape[1] == 1:
                y = y.ravel()
            self.X = self._check_X(X)
            self.y = y
            self.is_fitted = True
            return super().fit(self.X, self.y)

        def predict(self, X, eval_MSE=False):
            from sklearn.utils.validation import check_is_fitted

            check_is_fitted(self)
            return predict(self, X, eval_MSE)

        def __getstate__(self):
            state = dict(super().__getstate__())
            state.pop("_bogp_forest", None)  # the engine is a device handle
            return state

    return RandomForest


def __getattr__(name):
    global _CLASS
    if name == "RandomForest":
        if _CLASS is None:
            _CLASS = _build_class()
        return _CLASS
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


# ---------------------------------------------------------------------------------------------------------------------------------
# mixed search spaces
# ---------------------------------------------------------------------------------------------------------------------------------
class _Column:
    def __init__(self, kind, lo, hi, levels=0, scale="linear", precision=None, decode=float):
        self.kind, self.lo, self.hi, self.levels, self.scale, self.precision, self.decode = kind, lo, hi, levels, scale, precision, decode


def _var_kind(var) -> str:
    names = [c.__name__ for c in type(var).__mro__]
    for k in ("Real", "Integer", "Bool", "Subset", "Ordinal", "Discrete"):
        if k in names:
            return k
    return names[0]


def space_columns(space, packed: PackedForest):
    """One `_Column` per variable of a mixed search space: how the device draws it and how a drawn value becomes the reference's
    entry.  Real: uniform on the transformed scale (variable.py:240-257).  Integer: lo + index * step.  A column the model encodes
    one-hot: the level index, decoded to the MODEL's label of that index.  Any other Ordinal / Discrete / Bool column is a number to
    the model, so its labels must be equally spaced."""
    data = getattr(space, "data", None)
    if data is None:
        raise NotImplementedError("a forest sweep needs a search space with variables (%s)" % _SUPPORTED)
    if len(data) != packed.d_raw:
        raise ValueError("the search space has %d variables, the forest %d columns" % (len(data), packed.d_raw))
    from .optim import _TRANS

    cols = []
    for v, var in enumerate(data):
        kind = _var_kind(var)
        if kind == "Real":
            sc = getattr(var, "scale", "linear") or "linear"
            lo, hi = float(var.bounds[0]), float(var.bounds[1])
            c = _Column(_lib.COLUMN_REAL, lo, hi, 0, sc, getattr(var, "precision", None), float)
            c.lo_t, c.hi_t = float(_TRANS[sc][0](np.float64(lo))), float(_TRANS[sc][0](np.float64(hi)))
            cols.append(c)
            continue
        if kind not in ("Integer", "Bool", "Subset", "Ordinal", "Discrete"):
            raise NotImplementedError("variable %r is a %s: a forest sweep serves %s variables" % (getattr(var, "name", v), kind, _SUPPORTED))
        if v in packed.cat_idx:
            cats = packed.categories[packed.cat_idx.index(v)]
            labels = list(var.bounds)
            if len(labels) != len(cats) or any(_safe_index(cats, b) < 0 for b in labels):
                raise ValueError("the levels of variable %r differ from the model's levels of column %d" % (getattr(var, "name", v), v))
            cols.append(_Column(_lib.COLUMN_DISCRETE, 0.0, float(len(cats) - 1), len(cats), decode=lambda i, cats=cats: cats[int(round(i))]))
            continue
        if kind == "Integer":
            step = getattr(var, "step", 1) or 1
            L = int(var._size) if hasattr(var, "_size") else int(np.floor((var.bounds[1] - var.bounds[0]) / step) + 1)
            lo = var.bounds[0]
            integral = all(float(z).is_integer() for z in (lo, step))
            dec = (lambda x: int(round(x))) if integral else float
            cols.append(_Column(_lib.COLUMN_DISCRETE, float(lo), float(lo + (L - 1) * step), L, decode=dec))
            continue
        labels = list(var.bounds)  # an Ordinal / Discrete / Bool column the model reads as a number
        try:
            num = np.array([float(b) for b in labels])
        except (TypeError, ValueError):
            raise NotImplementedError("variable %r has non-numeric levels that the model does not one-hot encode (pass them in "
                                      "`levels=`)" % getattr(var, "name", v)) from None
        L = len(num)
        if L > 2 and not np.allclose(np.diff(num), (num[-1] - num[0]) / (L - 1), rtol=0, atol=0):
            raise NotImplementedError("variable %r: numeric levels that are not equally spaced are drawn on the device only when the "
                                      "model one-hot encodes them (pass them in `levels=`)" % getattr(var, "name", v))
        step = (num[-1] - num[0]) / (L - 1) if L > 1 else 0.0
        dec = (lambda x, labels=labels, lo=num[0], step=step: labels[int(round((x - lo) / step)) if step else 0])
        cols.append(_Column(_lib.COLUMN_DISCRETE, float(num[0]), float(num[-1]), L, decode=dec))
    return cols


def _safe_index(cats, x) -> int:
    try:
        return _label_lookup(cats)(x)
    except ValueError:
        return -1


def generate(dev: _Device, cols: Sequence[_Column], M: int, seed: int, first_row: int = 0):
    """Draw M rows of the mixed space on the device (bogp_candidates_generate_mixed + the Real variables' transform)."""
    real = [c.kind == _lib.COLUMN_REAL for c in cols]
    plain = all(c.scale == "linear" and c.precision is None for c in cols)
    eng = dev.engine
    if plain:
        eng.set_candidate_transform()
    else:
        eng.set_candidate_transform([c.scale for c in cols], [c.precision for c in cols], [c.lo for c in cols], [c.hi for c in cols])
    lo = [c.lo_t if r else c.lo for c, r in zip(cols, real)]
    hi = [c.hi_t if r else c.hi for c, r in zip(cols, real)]
    eng.generate_candidates_mixed([c.kind for c in cols], lo, hi, [c.levels for c in cols], int(M), int(seed), int(first_row))


def decode_rows(cols: Sequence[_Column], Xi: np.ndarray) -> list:
    """Device rows (reals, integers, level indices) -> rows in the reference's format (labels)."""
    return [[c.decode(x) for c, x in zip(cols, row)] for row in np.atleast_2d(Xi)]


# ---------------------------------------------------------------------------------------------------------------------------------
# sweeps
# ---------------------------------------------------------------------------------------------------------------------------------
def _is_ehvi(c) -> bool:
    return bool(getattr(c, "is_ehvi", False))


def _shared(criteria):
    """(first criterion, its model's device, [(acq_id, par)] -- None for an EHVI, which sweeps alone on a forest with n_obj outputs)."""
    c0 = criteria[0]
    ehvi = any(_is_ehvi(c) for c in criteria)
    m = n_outputs(c0.model)
    fitted = bool(getattr(c0.model, "estimators_", None))  # (an unfitted model is device_of's to refuse)
    if ehvi:
        if len(criteria) != 1:
            raise ValueError("an EHVI criterion sweeps alone: it cannot share a sweep with other criteria")
        if fitted and (m < 2 or c0.n_obj != m):
            raise NotImplementedError("EHVI over %d objectives on a forest with %d output%s: EHVI takes a forest fitted on y (N, n_obj), "
                                      "2 <= n_obj <= %d" % (c0.n_obj, m, "" if m == 1 else "s", _lib.MAX_TARGETS))
    elif m > 1:
        raise NotImplementedError("%s on a forest with %d outputs: the single-target criteria (EI, PI, EpsilonPI, UCB, MGFI) take a "
                                  "forest with one output; a forest with several takes EHVI" % (type(c0).__name__, m))
    for c in criteria[1:]:
        if c.model is not c0.model or c.minimize != c0.minimize or c.effective_plugin() != c0.effective_plugin():
            raise ValueError("criteria sharing one sweep must share model, minimize and plugin")
    dev = device_of(c0.model)
    if getattr(dev.engine, "comm_world", 0) > 1:
        raise NotImplementedError("a forest sweep runs on one rank (no multi-rank exchange of its winners)")
    return c0, dev, (None if ehvi else [(c.acq_id, c.acq_par()) for c in criteria])


def _sweep(c0, dev, acq, k: int, return_values: bool = False):
    """The sweep over the engine's current candidates: (values (q, k), indices (q, k)[, criterion values (q, M)])."""
    if acq is None:  # EHVI on the moments of a forest with several outputs (bogp_forest_sweep_ehvi)
        out = dev.engine.forest_sweep_ehvi(c0.cell_lower_bounds, c0.cell_upper_bounds, k=int(k), return_values=return_values)
        return tuple(np.asarray(a)[None, :] for a in out)
    return dev.engine.forest_sweep_topk(acq, c0.effective_plugin(), c0.minimize, int(k), return_values=return_values)


def ehvi_sweep(criterion, k: int = 1, return_values: bool = False):
    """`EHVI.sweep` on a forest model, over the engine's current candidates: (best (k,), idx (k,)[, values (M,)])."""
    c0, dev, acq = _shared([criterion])
    return tuple(a[0] for a in _sweep(c0, dev, acq, k, return_values))


def _one_rank(group=None, rank=None, world=None):
    from . import distributed

    if (world or 1) > 1 or distributed.rank_world(group)[1] > 1:
        raise NotImplementedError("a forest sweep runs on one rank (no multi-rank exchange of its winners)")


def criterion_values(criterion, X) -> np.ndarray:
    """The criterion at every row of X (rows in the reference's format): one device pass."""
    c0, dev, acq = _shared([criterion])
    dev.engine.upload_candidates(dev.packed.to_index(X))
    return _sweep(c0, dev, acq, 1, return_values=True)[2][0]


def sweep_topk_host(criteria, X, k: int = 1):
    """q criteria over host rows X (the reference's format): (values (q, k), indices (q, k), rows: q lists of k rows)."""
    c0, dev, acq = _shared(criteria)
    X_ = dev.packed._object_rows(X)
    dev.engine.upload_candidates(dev.packed.to_index(X_))
    vals, idx = _sweep(c0, dev, acq, k)
    rows = [[X_[i].tolist() if i >= 0 else None for i in r] for r in idx]
    return vals, idx, rows


def sweep_topk_device(criteria, space, M: int, k: int = 1, seed: int = 0):
    """q criteria over M rows of `space` drawn on the device: (values (q, k), rows (q, k), points: q lists of k rows in the
    reference's format)."""
    c0, dev, acq = _shared(criteria)
    cols = space_columns(space, dev.packed)
    generate(dev, cols, int(M), int(seed))
    vals, idx = _sweep(c0, dev, acq, k)
    ok = idx >= 0
    Xi = dev.engine.read_candidates(np.clip(idx, 0, int(M) - 1).ravel())
    dec = decode_rows(cols, Xi)
    rows = [[dec[r * idx.shape[1] + j] if ok[r, j] else None for j in range(idx.shape[1])] for r in range(idx.shape[0])]
    return vals, idx, rows


_HOST, _DEVICE = "sweep", "sweep-device"


def check_optimizer(optimizer: str, h=None, g=None, masks=None):
    if optimizer not in (_HOST, _DEVICE):
        what = {"sweep-device-lhs": "Latin hypercube designs", "sweep-device-sobol": "Sobol' designs"}.get(optimizer)
        if what is not None:
            raise NotImplementedError("optimizer=%r: %s are defined on real boxes; a forest model on a mixed space takes 'sweep' or "
                                      "'sweep-device'" % (optimizer, what))
        if optimizer in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
            raise NotImplementedError("optimizer=%r needs an input gradient, which a forest does not have: use 'sweep' or "
                                      "'sweep-device'" % optimizer)
        raise NotImplementedError("optimizer=%r does not serve a forest model: use 'sweep' or 'sweep-device'" % optimizer)
    if h is not None or g is not None:
        raise NotImplementedError("a forest sweep takes no constraints (h / g)")
    if masks is not None:
        raise NotImplementedError("a forest sweep takes no fixed variables")


def argmax_restart(criterion, search_space, eval_budget: int, optimizer: str, h=None, g=None, masks=None):
    """`optim.argmax_restart` for a criterion on a forest model: (xopt: list in the reference's row format, fopt: float)."""
    check_optimizer(optimizer, h, g, masks)
    _one_rank()
    if optimizer == _HOST:
        vals, _, rows = sweep_topk_host([criterion], search_space.sample(int(eval_budget), method="uniform"), 1)
    else:
        vals, _, rows = sweep_topk_device([criterion], search_space, int(eval_budget), 1, int(np.random.randint(0, 2**62)))
    return rows[0][0], float(vals[0, 0])


def batch_argmax(criteria, search_space, eval_budget: int, history=None, k: int = 8, design: Optional[str] = None,
                 seed: Optional[int] = None, Xs=None):
    """`optim.batch_argmax` for q criteria on one forest model: every criterion takes its best candidate that is neither taken by an
    earlier criterion nor an evaluated row of `history` (rows compared entry by entry), falling back through its top-k."""
    if design not in (None, "uniform"):
        raise NotImplementedError("design=%r: a forest model on a mixed space takes the uniform design only" % design)
    if design is None:
        X = search_space.sample(int(eval_budget), method="uniform") if Xs is None else Xs
        vals, idx, rows = sweep_topk_host(criteria, X, int(k))
    else:
        seed = int(np.random.randint(0, 2**62)) if seed is None else int(seed)
        vals, idx, rows = sweep_topk_device(criteria, search_space, int(eval_budget), int(k), seed)
    seen = [list(r) for r in (history if history is not None else [])]
    xs, fs, taken = [], [], set()
    for c in range(len(criteria)):
        pick = 0
        for r in range(idx.shape[1]):
            gi = int(idx[c, r])
            if gi < 0 or gi in taken or any(_same_row(rows[c][r], s) for s in seen):
                continue
            pick = r
            break
        taken.add(int(idx[c, pick]))
        xs.append(rows[c][pick])
        fs.append(float(vals[c, pick]))
    return tuple(xs), tuple(fs)


def _same_row(a, b) -> bool:
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        try:
            if not np.isclose(float(x), float(y)):
                return False
        except (TypeError, ValueError):
            if x != y:
                return False
    return True
