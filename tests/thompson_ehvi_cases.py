"""The cases of Thompson batches for multi-objective runs, shared by tests/test_gpu_thompson_ehvi.py and tests/test_thompson_ehvi_host.py
(which asserts, on the restatement alone, what each case is chosen for).  Problems, states and allowances are
tests/thompson_constrained_cases.py's.  Fronts by name: "empty" (C = 1), "one" (one point: 2^(m-1) cells), "arc" (m = 2, 32 points:
C = 33), "stairs" (m = 3, 10 points: C = 121), "far" (one point at 50: no row improves); cells from `pareto.hypercell_bounds`."""
from types import SimpleNamespace

import numpy as np

import thompson_constrained_cases as TC
from bogp import _lib, pareto, thompson

MS, DS, NS, LS = [1, 15, 16, 17, 63, 64, 65, 1000], [1, 4, 5, 20, 33], [5, 64, 67], [16, 48]
MQ = [(2, 8), (2, 1), (3, 5), (5, 3), (8, 2), (8, 1)]  # two pairs a lane; 16 live lanes; a partial second round; 48, 32 and 16 lanes
FRONTS = {2: ["arc", "one", "empty"], 3: ["stairs", "one"], 5: ["one", "empty"], 8: ["one", "empty"]}
KERNELS = [_lib.KERNEL_MATERN52, _lib.KERNEL_SE, _lib.KERNEL_MATERN12]
# 16 shapes: every value of every parameter, in changing company; M = 65 and M = 1 leave a last block of one row
SHAPES = [(MS[i % 8], DS[(i + i // 8) % 5], NS[(i + i // 3) % 3], LS[(i // 2) % 2]) + MQ[(i + i // 6) % 6] + (KERNELS[i % 3],) for i in range(16)]

# The selection cases (M = 1000, L = 48): name -> (m, q, N, d, kernel, front, quantile of each training column at which the reference
# point stands, seed of the draw), chosen so that the share of improving (row, member) pairs is what the host twin asserts.
CASES = {
    "m2-mixed": (2, 8, 67, 4, _lib.KERNEL_MATERN52, "arc", 0.3, 1),
    "m2-single": (2, 1, 67, 4, _lib.KERNEL_SE, "one", 0.3, 2),
    "m3-mixed": (3, 5, 64, 5, _lib.KERNEL_MATERN52, "stairs", 0.3, 3),
    "m5-mixed": (5, 3, 67, 4, _lib.KERNEL_SE, "one", 0.3, 4),
    "m8-mixed": (8, 2, 64, 4, _lib.KERNEL_MATERN12, "one", 0.2, 5),
    "m3-none": (3, 5, 67, 4, _lib.KERNEL_MATERN52, "far", 0.3, 6),
    "m2-empty": (2, 8, 5, 1, _lib.KERNEL_SE, "empty", 0.0, 7),
}
CASE_M, CASE_L = 1000, 48


def cells(front, Y, level):
    """(lower, upper), C x m each, of the named front over a reference point at the `level` quantile of Y's columns (level 0: 1.0 below)."""
    m = Y.shape[1]
    ref = np.quantile(Y, level, axis=0) - (1.0 if level == 0 else 0.0)
    top = Y.max(axis=0)
    if front == "empty":
        P = np.empty((0, m))
    elif front == "far":
        P = np.full((1, m), 50.0)
    elif front == "one":
        P = (ref + 0.5 * (top - ref))[None, :]
    elif front == "arc":
        a = np.linspace(0.05, 0.95, 32) * np.pi / 2
        P = ref + 0.6 * (top - ref) * np.column_stack([np.cos(a), np.sin(a)])
    else:  # "stairs"
        s = np.linspace(0.1, 0.8, 10)
        P = ref + (top - ref) * np.column_stack([s, s[::-1], 0.3 + 0.4 * np.abs(s - 0.45)])
    return pareto.hypercell_bounds(P, ref) if len(P) else (ref[None, :].copy(), np.full((1, m), np.inf))


def case(name, sigma2=None):
    m, q, N, d, kernel, front, level, seed = CASES[name]
    X, Y, theta, Xs = TC.problem(CASE_M, d, N, kernel, m)
    lower, upper = cells(front, Y, level)
    st = TC.state(X, Y, theta, kernel, sigma2)
    return SimpleNamespace(X=X, Y=Y, theta=theta, Xs=Xs, kernel=kernel, lower=lower, upper=upper, q=q, m=m, st=st, front=front,
                           dr=thompson.draw_multi(st, q, CASE_L, seed=seed))  # fmt: skip
