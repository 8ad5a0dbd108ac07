"""The cases the CPU twin (tests/test_constrained_ehvi_grad_host.py) and the device tests (tests/test_gpu_constrained_ehvi_grad.py) of
`bogp_point_eval_ehvi_constrained` share: plain data and generators, no test.  The CPU twin asserts on the restatement alone that in
every configuration at least half of the rows are alive (every MSE_k > 0, P > 0, value > 0, a non-zero finite gradient), that P is not
one constant, that no row sits at the small-variance guard, and that the list holds a configuration without cells and one with more
than 10 000, so that a device test cannot hide a failure behind an ill-posed case.  A configuration that fails one of these conditions
gets another seed, never another threshold.

27 configurations: N in {37, 100, 157} (below a row block, not a multiple of 64, just past the one-launch fit) x d in {2, 12, 23} (12
columns in one pass, 22 in one pass, two passes) x 3, with (m, c) dealt over nine pairs and the four kernels, noisy and noiseless models
and B in {1, 33} in rotation.  Every configuration has 33 rows; one with B = 1 sends them through the one-point call one by one."""
import itertools

import numpy as np

from bogp import _lib, pareto

INF = float("inf")
BOX = (-2.0, 2.0)
KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP]
PAIRS = [(2, 1), (2, 2), (3, 1), (3, 2), (2, 6), (7, 1), (4, 1), (5, 3), (6, 2)]  # (objectives, constraints)
ROWS = 33


def bounds(Y, m, first=0):
    """The four kinds in rotation over the constraint columns: (-inf, median], [q25, q75], [q50, +inf), [-0.6 std, 0.6 std]."""
    lo, hi = [], []
    for j in range(Y.shape[1] - m):
        col = Y[:, m + j]
        kind = (first + j) % 4
        if kind == 0:
            lo.append(-INF), hi.append(float(np.median(col)))
        elif kind == 1:
            lo.append(float(np.quantile(col, 0.25))), hi.append(float(np.quantile(col, 0.75)))
        elif kind == 2:
            lo.append(float(np.median(col))), hi.append(INF)
        else:
            tol = 0.6 * float(col.std())
            lo.append(-tol), hi.append(tol)
    return np.array(lo), np.array(hi)


def cells(Y, m, lo, hi):
    """(ref_point, lower, upper, feasible rows): the cells of the front of the first 8 feasible training rows (4 for m >= 5: (4 + 1)^(m - 1)
    cells at most) above ref = min - 0.1 |min| of the objective columns; no feasible row: no cells."""
    ref = Y[:, :m].min(0) - 0.1 * np.abs(Y[:, :m].min(0))
    feasible = np.all((Y[:, m:] >= lo) & (Y[:, m:] <= hi), axis=1)
    take = np.flatnonzero(feasible)[: 8 if m < 5 else 4]
    if len(take) == 0:
        return ref, np.zeros((0, m)), np.zeros((0, m)), 0
    lower, upper = pareto.hypercell_bounds(Y[take, :m], ref)
    return ref, np.ascontiguousarray(lower), np.ascontiguousarray(upper), int(feasible.sum())


def problem(kernel, noisy, N, d, m, c, first=0, seed=0, theta=None):
    """(par, mode, X, Y, lo, hi): tests/test_gpu_constrained_grad.py::_problem's recipe and hyper-parameters for m + c targets."""
    rng = np.random.default_rng(seed)
    mt = m + c
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, mt))) * (1.0 + np.arange(mt)) + 0.3 * rng.normal(size=(N, mt))
    if noisy:
        par, mode = np.r_[np.full(d, theta or (10.0 if d == 2 else 0.6 / d)), 0.9], _lib.MODE_NOISE_ESTIM
    else:  # (short length scales keep the noiseless R well conditioned)
        par, mode = np.full(d, theta or 200.0 / d), _lib.MODE_NOISELESS
    lo, hi = bounds(Y, m, first)
    return par, mode, X, Y, lo, hi


def rows_of(rng, X, n=ROWS):
    """n rows: uniform draws and, last, one next to a training point."""
    rows = rng.uniform(*BOX, size=(n, X.shape[1]))
    rows[-1] = X[1] + 1e-3
    return rows


class Config:
    def __init__(self, i, N, d, m, c, kernel, noisy, first, B, seed):
        self.i, self.N, self.d, self.m, self.c, self.kernel, self.noisy, self.first, self.B, self.seed = i, N, d, m, c, kernel, noisy, first, B, seed
        self.id = "k%d-%s-N%d-d%d-m%d-c%d-b%d-B%d" % (kernel, "noisy" if noisy else "exact", N, d, m, c, first, B)

    def build(self):
        """dict: par, mode, X, Y, lo, hi (constraints), ref, lower, upper (cells), n_feasible, rows (33, d)"""
        par, mode, X, Y, lo, hi = problem(self.kernel, self.noisy, self.N, self.d, self.m, self.c, self.first, self.seed)
        ref, lower, upper, n_feasible = cells(Y, self.m, lo, hi)
        return dict(par=par, mode=mode, X=X, Y=Y, lo=lo, hi=hi, ref=ref, lower=lower, upper=upper, n_feasible=n_feasible,
                    rows=rows_of(np.random.default_rng(1), X))  # fmt: skip


def configs():
    out = []
    for i, (N, d, r) in enumerate(itertools.product((37, 100, 157), (2, 12, 23), range(3))):
        m, c = PAIRS[(i + 4 * (i // 9)) % 9]
        out.append(Config(i, N, d, m, c, KERNELS[(i + i // 4) % 4], i % 3 != 2, i % 4, (1, 33)[(i + i // 3) % 2], seed=N + d + m + c + SEED_SHIFT.get(i, 0)))
    return out


SEED_SHIFT = {}  # configuration index -> added to its seed where the first draw missed a condition of the CPU twin
CONFIGS = configs()
IDS = [c.id for c in CONFIGS]
