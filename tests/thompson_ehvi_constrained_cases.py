"""The cases of Thompson batches for constrained multi-objective runs, shared by tests/test_gpu_thompson_ehvi_constrained.py and
tests/test_thompson_ehvi_constrained_host.py (which asserts, on the restatement alone, what each case is built for).  Problems, states
and allowances are tests/thompson_constrained_cases.py's, the named fronts tests/thompson_ehvi_cases.py's.  No test lives here."""
from types import SimpleNamespace

import numpy as np

import thompson_constrained_cases as TC
import thompson_ehvi_cases as EC
from bogp import _lib, pareto, thompson

MS, DS, NS, LS, CS = [1, 15, 16, 17, 63, 64, 65, 1000], [1, 4, 5, 20, 33], [5, 64, 67], [16, 48], [1, 2, 33, 128]
# (m_obj, n_con, q): 80 pairs a wave and up to 320 a workgroup; 16 live lanes; exactly 64 / 256; one partial round; the widest m_obj, n_con
MNQ = [(2, 1, 5), (2, 1, 1), (2, 2, 4), (3, 1, 4), (2, 3, 3), (4, 4, 2), (7, 1, 2), (2, 6, 1)]
KERNELS = EC.KERNELS
# 16 shapes: every value of every parameter, in changing company; M = 65 and M = 1 leave a last block of one row
SHAPES = [(MS[i % 8], DS[(i + i // 8) % 5], NS[(i + i // 3) % 3], LS[(i // 2) % 2], CS[(i + i // 4) % 4]) + MNQ[(i + i // 8) % 8] + (KERNELS[i % 3],)
          for i in range(16)]  # fmt: skip

# The selection cases (M = 1000, L = 48): name -> (m_obj, n_con, q, N, d, kernel, cells, feasible share of the (row, member) pairs by
# construction, seed of the draw).  cells: a count C (`cells_of`) or one of EC's named fronts ("far": no row improves; "empty": one cell).
CASES = {
    "none": (2, 1, 5, 67, 4, _lib.KERNEL_MATERN52, 33, 0.0, 1),   # no list: every A and B is -inf, V decides
    "tenth": (2, 1, 5, 67, 4, _lib.KERNEL_SE, 33, 0.1, 2),
    "half": (3, 1, 4, 64, 5, _lib.KERNEL_MATERN52, "stairs", 0.5, 3),
    "half-wide": (4, 4, 2, 67, 4, _lib.KERNEL_SE, 2, 0.5, 4),
    "all": (2, 1, 5, 67, 4, _lib.KERNEL_MATERN52, 33, 1.0, 5),    # infinite bounds: F = 320 > 256
    "far": (2, 2, 4, 67, 4, _lib.KERNEL_MATERN52, "far", 0.5, 6),  # feasible rows, none improving: B decides
    "empty": (2, 1, 5, 5, 1, _lib.KERNEL_SE, "empty", 0.5, 7),
}
BAND = {0.0: (0.0, 0.0), 0.1: (0.03, 0.25), 0.5: (0.3, 0.7), 1.0: (1.0, 1.0)}  # where the realised share must lie
CASE_M, CASE_L = 1000, 48


def cells_of(C, Y, level=0.3):
    """(lower, upper), C x m_obj each: the C cells of a front of C - 1 points on an arc in the first two objectives (C = 1: no point)
    above the reference point at the `level` quantile of Y's columns; every further objective has [ref_k, +inf) in every cell."""
    m = Y.shape[1]
    ref, top = np.quantile(Y, level, axis=0), Y.max(axis=0)
    a = np.linspace(0.05, 0.95, C - 1) * np.pi / 2
    P = ref[:2] + 0.6 * (top[:2] - ref[:2]) * np.column_stack([np.cos(a), np.sin(a)])
    l2, u2 = pareto.hypercell_bounds(P, ref[:2]) if C > 1 else (ref[None, :2].copy(), np.full((1, 2), np.inf))
    assert len(l2) == C
    return (np.ascontiguousarray(np.hstack([l2, np.tile(ref[2:], (C, 1))])), np.ascontiguousarray(np.hstack([u2, np.full((C, m - 2), np.inf)])))


def bounds_for_share(paths, m_obj, share):
    """(lo, hi) at which about `share` of the (row, member) pairs of `paths` (q, m, M) are feasible: hi_i the share^(1 / n_con) quantile
    of constraint i's path values (the constraints are drawn independently), lo = -inf; share 0: lo = hi = 50; share 1: infinite."""
    n_con = paths.shape[1] - m_obj
    if share == 0.0:
        return np.full(n_con, 50.0), np.full(n_con, 50.0)
    if share == 1.0:
        return np.full(n_con, -np.inf), np.full(n_con, np.inf)
    return np.full(n_con, -np.inf), np.array([np.quantile(paths[:, m_obj + i], share ** (1.0 / n_con)) for i in range(n_con)])


def case(name, sigma2=None):
    m_obj, n_con, q, N, d, kernel, front, share, seed = CASES[name]
    X, Y, theta, Xs = TC.problem(CASE_M, d, N, kernel, m_obj + n_con)
    lower, upper = cells_of(front, Y[:, :m_obj]) if isinstance(front, int) else EC.cells(front, Y[:, :m_obj], 0.0 if front == "empty" else 0.3)
    st = TC.state(X, Y, theta, kernel, sigma2)
    return SimpleNamespace(X=X, Y=Y, theta=theta, Xs=Xs, kernel=kernel, lower=lower, upper=upper, q=q, m_obj=m_obj, n_con=n_con, st=st,
                           front=front, share=share, dr=thompson.draw_multi(st, q, CASE_L, seed=seed))  # fmt: skip
