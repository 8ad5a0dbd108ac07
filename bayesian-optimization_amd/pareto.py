"""Pareto fronts and the cell decomposition behind `acquisition.EHVI` (maximised objectives, numpy only).

The region of objective space above a reference point r that a finite front P does NOT dominate is cut into axis-aligned
cells (l_c, u_c).  The decomposition here is the plain grid one: along each of the first m - 1 axes the cut points are
r_k and the distinct front coordinates above it, the last axis is left open.  Inside one grid column every front point
either covers the column's whole extent in all of the first m - 1 axes or none of it, so the dominated part of the
column is exactly {y_m <= L}, L = the largest last coordinate of the covering points (r_m when none covers): the column
contributes the cell [column] x [L, +inf).  That gives (P + 1)^(m - 1) cells at most -- fine for the fronts a BO run
builds (m = 2: P + 1 cells; m = 3, P = 32: 1 089).  EHVI does not depend on which partition is used.
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from ._lib import MAX_EHVI_CELLS


def is_non_dominated(Y) -> np.ndarray:
    """Boolean mask of the rows of Y (n x m, maximised) that no other row dominates (>= in every objective, > in one).
    Of several identical non-dominated rows only the first is kept."""
    Y = np.atleast_2d(np.asarray(Y, dtype=float))
    n = len(Y)
    keep = np.ones(n, dtype=bool)
    for i in range(n):
        ge = np.all(Y >= Y[i], axis=1)
        gt = np.any(Y > Y[i], axis=1)
        if np.any(ge & gt):
            keep[i] = False
            continue
        same = np.all(Y[:i] == Y[i], axis=1) & keep[:i]
        if np.any(same):
            keep[i] = False
    return keep


def pareto_front(Y, ref_point) -> np.ndarray:
    """The non-dominated rows of Y that lie strictly above `ref_point` in every objective (the only ones that dominate
    any volume above it)."""
    Y = np.atleast_2d(np.asarray(Y, dtype=float))
    r = np.asarray(ref_point, dtype=float).ravel()
    if Y.shape[1] != len(r):
        raise ValueError("Y has %d objectives, ref_point %d" % (Y.shape[1], len(r)))
    P = Y[is_non_dominated(Y)]
    return P[np.all(P > r, axis=1)]


def _grid_parts(Y, ref_point):
    """What `hypercell_bounds` and `hypercell_grid` share: (edges, idx, last, r_last) -- per axis k < m - 1 its cut points
    r_k, the distinct front coordinates and +inf; the C x (m - 1) interval indices of the columns, row-major with axis 0
    slowest; the lower bound of each column on the last axis; the reference point's last coordinate.  Raises ValueError past
    `MAX_EHVI_CELLS` columns."""
    r = np.asarray(ref_point, dtype=float).ravel()
    m = len(r)
    if m < 2:
        raise ValueError("hypercell_bounds needs at least two objectives")
    P = pareto_front(Y, r)
    edges = [np.r_[r[k], np.unique(P[:, k]), np.inf] for k in range(m - 1)]  # P > r: every front coordinate lies above r_k
    n_cells = math.prod(len(e) - 1 for e in edges)  # (Python integers: no wrap-around before the limit check)
    if n_cells > MAX_EHVI_CELLS:
        raise ValueError("a front of %d points in %d objectives gives %d cells (more than %d): pass the cells explicitly "
                         "(EHVI(cells=(lower, upper)) or a partitioning object with fewer cells)" % (len(P), m, n_cells, MAX_EHVI_CELLS))
    idx = np.array(list(itertools.product(*[range(len(e) - 1) for e in edges])), dtype=np.int64).reshape(n_cells, m - 1)
    if len(P):
        hi = np.stack([edges[k][idx[:, k] + 1] for k in range(m - 1)], axis=1)
        cover = np.all(P[None, :, : m - 1] >= hi[:, None, :], axis=2)  # n_cells x P
        last = np.max(np.where(cover, P[None, :, m - 1], r[m - 1]), axis=1)
    else:
        last = np.full(n_cells, r[m - 1])
    return edges, idx, last, r[m - 1]


def _expand(edges, idx, last):
    """(lower, upper) of the columns `idx` of the grid `edges` with the last-axis lower bounds `last`."""
    m1 = len(edges)
    lo = np.stack([edges[k][idx[:, k]] for k in range(m1)], axis=1)
    hi = np.stack([edges[k][idx[:, k] + 1] for k in range(m1)], axis=1)
    return np.column_stack([lo, last]), np.column_stack([hi, np.full(len(idx), np.inf)])


def hypercell_bounds(Y, ref_point):
    """(lower, upper), each C x m: cells that together cover exactly the region above `ref_point` that the front of Y
    does not dominate (upper bounds may be +inf).  Raises ValueError past `MAX_EHVI_CELLS` cells."""
    edges, idx, last, _ = _grid_parts(Y, ref_point)
    return _expand(edges, idx, last)


class HypercellGrid:
    """The cells of `hypercell_bounds`, not expanded: `edges[k]` (n_k + 1 cut points of axis k < m - 1, the last +inf), the
    columns row-major over the axes' intervals with axis 0 slowest, `last_val` (V,) the distinct lower bounds on the last
    axis in ascending order, `last_idx` (C,) int32 the entry of `last_val` of each column."""

    def __init__(self, edges, last_val, last_idx):
        self.edges = [np.asarray(e, dtype=float) for e in edges]
        self.last_val = np.asarray(last_val, dtype=float)
        self.last_idx = np.asarray(last_idx, dtype=np.int32)

    @property
    def n_cells(self):
        return [len(e) - 1 for e in self.edges]


def hypercell_grid(Y, ref_point) -> HypercellGrid:
    """The decomposition of `hypercell_bounds(Y, ref_point)` as a grid (`expand_grid` gives those cells back, bit for bit):
    what `Engine.sweep_ehvi_grid` evaluates per axis and not per cell.  Raises ValueError as `hypercell_bounds` does."""
    edges, _, last, _ = _grid_parts(Y, ref_point)
    last_val, last_idx = np.unique(last, return_inverse=True)
    return HypercellGrid(edges, last_val, last_idx.reshape(-1))


def expand_grid(grid):
    """(lower, upper), each C x m, of the cells of a `HypercellGrid`."""
    n = grid.n_cells
    idx = np.array(list(itertools.product(*[range(k) for k in n])), dtype=np.int64).reshape(math.prod(n), len(n))
    return _expand(grid.edges, idx, grid.last_val[grid.last_idx])


def ehvi_grid_numpy(mu, mse, grid) -> np.ndarray:
    """EHVI of M rows of moments (M x m each) over the cells of `grid` by the factored sum of `bogp_sweep_ehvi_grid`, dense
    float64: per axis t_k[i] = sd_k (G(a_i) - G(a_{i+1})), G = 0 at +inf, t_last[v] = sd G((last_val[v] - mu) / sd), and the
    sum over the columns of their products (G(z) = phi(z) - z Phi(-z), sd = sqrt(max(mse, 1e-9)))."""
    from scipy.special import ndtr

    mu, mse = np.atleast_2d(np.asarray(mu, dtype=float)), np.atleast_2d(np.asarray(mse, dtype=float))
    sd = np.sqrt(np.maximum(mse, 1e-9))

    def G(z):
        return np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) - z * ndtr(-z)

    n = grid.n_cells
    prod = np.ones((len(mu), 1))
    for k, e in enumerate(grid.edges):  # the product over the axes as an outer product: M x (n_0 .. n_k), flattened row-major
        g = np.concatenate([G((e[None, :-1] - mu[:, k : k + 1]) / sd[:, k : k + 1]), np.zeros((len(mu), 1))], axis=1)
        t = sd[:, k : k + 1] * (g[:, :-1] - g[:, 1:])
        prod = (prod[:, :, None] * t[:, None, :]).reshape(len(mu), -1)
    t_last = sd[:, -1:] * G((grid.last_val[None, :] - mu[:, -1:]) / sd[:, -1:])
    assert prod.shape[1] == math.prod(n) == len(grid.last_idx)
    return np.sum(prod * t_last[:, grid.last_idx], axis=1)
