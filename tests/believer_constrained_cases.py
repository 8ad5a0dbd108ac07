"""The cases the CPU twin (tests/test_believer_constrained_host.py) and the device tests (tests/test_gpu_believer_constrained.py) of
`bogp_sweep_believer_constrained` share: plain data and generators, no test.  The CPU twin asserts on the restatement alone that every
case is free of ties, of rows at EI's variance guard and of believed means at a bound, so that a device test cannot hide a failure
behind an ill-posed case.  A case that fails one of these conditions gets another seed or other bounds, never another threshold."""
import numpy as np

from bogp import _lib

INF = float("inf")
D, M, Q = 3, 1500, 4
ACQ_MIXED = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_EPSILON_PI, 0.0), (_lib.ACQ_MGFI, 2.0), (_lib.ACQ_EI, 0.0)]  # EI, PI, MGFI (t = 2), EI
ACQ_FEASIBILITY = [(_lib.ACQ_NONE, 0.0)] * 4


def problem(N, m, kernel, noisy, seed=0, rows=M):
    """tests/test_gpu_believer_ehvi.py::problem's recipe: (X, Y, commit arguments, candidates, two pending rows off the candidates).
    N = 70 pads to 96 rows, N = 530 is chunked under BOGP_CHUNK_MB=1; distinct per-target scales, short length scales."""
    rng = np.random.default_rng(1000 * seed + 10 * N + m)
    X = rng.uniform(-2, 2, size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    theta = np.array([1.0, 0.8, 1.3]) * (4.0 if N < 100 else 8.0)
    if noisy:
        args = (kernel, _lib.MODE_NOISE_ESTIM, np.r_[theta, 0.9], 0.0, False, 0.1)
    else:
        args = (kernel, _lib.MODE_NOISELESS, theta, 0.0, False, 0.1)
    Xs = rng.uniform(-2.2, 2.2, size=(M, D))[:rows]
    pend = rng.uniform(-2, 2, size=(2, D))
    return X, Y, args, Xs, pend


def quantile_bounds(Y):
    """tests/test_gpu_constrained.py::_bounds: intervals cycling through (-inf, q50], [q25, q75], [q50, +inf) of the training columns"""
    lo, hi = [], []
    for k in range(1, Y.shape[1]):
        q25, q50, q75 = np.quantile(Y[:, k], [0.25, 0.5, 0.75])
        a, b = ((-INF, q50), (q25, q75), (q50, INF))[(k - 1) % 3]
        lo.append(a), hi.append(b)
    return np.array(lo), np.array(hi)


def narrow_bounds(Y):
    """[q40, q60] on every constraint: the probability of feasibility reaches 1.0 on no row, so a feasibility-only step has no ties"""
    q = np.quantile(Y[:, 1:], [0.4, 0.6], axis=0)
    return q[0].copy(), q[1].copy()


def plugin_of(Y, lo, hi, minimize):
    """the best feasible training value in the criterion's sign (the best value of all rows where no row is feasible)"""
    ok = np.all((Y[:, 1:] >= lo) & (Y[:, 1:] <= hi), axis=1)
    y0 = Y[ok, 0] if ok.any() else Y[:, 0]
    return float(y0.min() if minimize else -y0.max())


class Case:
    def __init__(self, N, m, kernel, noisy, n_pend, minimize, acq, bounds, rows=M, seed=0):
        self.N, self.m, self.kernel, self.noisy, self.n_pend, self.minimize = N, m, kernel, noisy, n_pend, minimize
        self.acq, self.bounds, self.rows, self.seed = acq, bounds, rows, seed
        self.id = "N%d-m%d-%s-%s-p%d-%s-%s" % (N, m, "m52" if kernel == _lib.KERNEL_MATERN52 else "se", "noisy" if noisy else "noiseless", n_pend,
                                                "min" if minimize else "max", "pof" if acq is ACQ_FEASIBILITY else "mixed")  # fmt: skip

    def build(self):
        """(X, Y, commit arguments, candidates, pending rows, lo, hi, plugin)"""
        X, Y, args, Xs, pend = problem(self.N, self.m, self.kernel, self.noisy, self.seed, self.rows)
        lo, hi = self.bounds(Y)
        return X, Y, args, Xs, pend[: self.n_pend], lo, hi, plugin_of(Y, lo, hi, self.minimize)


MODELS = [(_lib.KERNEL_MATERN52, False), (_lib.KERNEL_SE, True)]  # Matern-5/2 noiseless, SE noise-estimating
CASES = [Case(N, m, k, noisy, n_pend, minimize, ACQ_MIXED, quantile_bounds)
         for N in (70, 530) for m in (2, 3) for k, noisy in MODELS for n_pend in (0, 2) for minimize in (True, False)]  # fmt: skip
CASES.append(Case(70, 8, _lib.KERNEL_MATERN52, False, 2, True, ACQ_MIXED, quantile_bounds, rows=599))
# feasibility only, four steps: the cases of the narrow bounds that are free of ties
CASES += [Case(70, m, k, noisy, n_pend, True, ACQ_FEASIBILITY, narrow_bounds) for m in (2, 3) for k, noisy in MODELS for n_pend in (0, 2)]
CASES += [Case(530, 3, _lib.KERNEL_MATERN52, False, n_pend, True, ACQ_FEASIBILITY, narrow_bounds) for n_pend in (0, 2)]
IDS = [c.id for c in CASES]
