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


def hypercell_bounds(Y, ref_point):
    """(lower, upper), each C x m: cells that together cover exactly the region above `ref_point` that the front of Y
    does not dominate (upper bounds may be +inf).  Raises ValueError past `MAX_EHVI_CELLS` cells."""
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
    lo = np.stack([edges[k][idx[:, k]] for k in range(m - 1)], axis=1)
    hi = np.stack([edges[k][idx[:, k] + 1] for k in range(m - 1)], axis=1)
    if len(P):
        cover = np.all(P[None, :, : m - 1] >= hi[:, None, :], axis=2)  # n_cells x P
        last = np.max(np.where(cover, P[None, :, m - 1], r[m - 1]), axis=1)
    else:
        last = np.full(n_cells, r[m - 1])
    lower = np.column_stack([lo, last])
    upper = np.column_stack([hi, np.full(n_cells, np.inf)])
    return lower, upper
