"""The cases the CPU twin (tests/test_believer_constrained_ehvi_host.py) and the device tests
(tests/test_gpu_believer_constrained_ehvi.py) of `bogp_sweep_believer_ehvi_constrained` share: plain data and generators, no test.  The
recipe is tests/believer_constrained_cases.py's (distinct per-target scales, short length scales, a noiseless Matern-5/2 model and a
noise-estimating SE model); targets 0 .. m_obj - 1 are the objectives, maximised as given, the others constraints.  The CPU twin
asserts on the restatement alone that every case is free of ties, of rows at the variance guard, of believed constraint means at a
bound and of believed objective means at a coordinate that decides dominance, so that a device test cannot hide a failure behind an
ill-posed case.  A case that fails one of these conditions gets another seed or other bounds, never another threshold."""
import numpy as np

from bogp import _lib
from believer_constrained_cases import D, M, MODELS, narrow_bounds, problem, quantile_bounds  # noqa: F401

Q = 4


def constraint_bounds(Y, m_obj, bounds=quantile_bounds):
    """`bounds` of tests/believer_constrained_cases.py on the constraint columns m_obj .. of Y (they skip the first column they are given)"""
    return bounds(Y[:, m_obj - 1 :])


def feasible_rows(Y, m_obj, lo, hi):
    return np.all((Y[:, m_obj:] >= lo) & (Y[:, m_obj:] <= hi), axis=1)


def low_ref(Y, m_obj):
    """below every training row: the feasible front has several points"""
    return Y[:, :m_obj].min(axis=0) - 0.1


def high_ref(Y, m_obj, ok):
    """above every feasible training row: the one cell [ref, +inf)"""
    return Y[ok, :m_obj].max(axis=0) + 0.25


class Case:
    def __init__(self, N, m_obj, c, kernel, noisy, n_pend, bounds=quantile_bounds, rows=M, seed=0, feasibility_only=False, one_cell=False, front_rows=None, believe_front=True):
        self.N, self.m_obj, self.c, self.kernel, self.noisy, self.n_pend = N, m_obj, c, kernel, noisy, n_pend
        self.bounds, self.rows, self.seed, self.feasibility_only, self.one_cell = bounds, rows, seed, feasibility_only, one_cell
        self.front_rows = front_rows  # the first feasible rows only (seven objectives: the grid has (front + 1)^6 cells)
        self.believe_front = believe_front
        self.m = m_obj + c
        self.id = "N%d-o%d-c%d-%s-%s-p%d-%s" % (N, m_obj, c, "m52" if kernel == _lib.KERNEL_MATERN52 else "se", "noisy" if noisy else "noiseless",
                                                  n_pend, "pof" if feasibility_only else "onecell" if one_cell else "cells")  # fmt: skip

    def build(self):
        """(X, Y, commit arguments, candidates, pending rows, lo, hi, ref_point, front): `front` the objective rows of the feasible
        training rows (empty for a feasibility-only case: the criterion is the caller's)"""
        X, Y, args, Xs, pend = problem(self.N, self.m, self.kernel, self.noisy, self.seed, self.rows)
        lo, hi = constraint_bounds(Y, self.m_obj, self.bounds)
        ok = feasible_rows(Y, self.m_obj, lo, hi)
        ref = high_ref(Y, self.m_obj, ok) if self.one_cell else low_ref(Y, self.m_obj)
        front = np.zeros((0, self.m_obj)) if self.feasibility_only else Y[ok, : self.m_obj][: self.front_rows].copy()
        return X, Y, args, Xs, pend[: self.n_pend], lo, hi, ref, front


SHAPES = [(2, 1), (2, 2), (3, 1)]
CASES = [Case(N, mo, c, k, noisy, n_pend) for mo, c in SHAPES for N in (70, 530) for k, noisy in MODELS for n_pend in (0, 2)]
# MT = 8 at both ends of the objective count, on 599 rows
CASES.append(Case(70, 2, 6, _lib.KERNEL_MATERN52, False, 2, rows=599))
# (seven objectives: one front point gives 2^6 cells; a front that grew by three believed means would give 5^6, so this front stays)
CASES.append(Case(70, 7, 1, _lib.KERNEL_MATERN52, False, 0, rows=599, front_rows=1, believe_front=False))
# feasibility only under the narrow bounds [q40, q60], four steps
# (seed 0 of the SE model with one constraint has two rows at P == 1.0, a tie: seed 1)
CASES += [Case(70, mo, c, k, noisy, n_pend, bounds=narrow_bounds, feasibility_only=True, seed=1 if (c == 1 and noisy) else 0)
          for mo, c in ((2, 1), (2, 2)) for k, noisy in MODELS for n_pend in (0, 2)]  # fmt: skip
CASES += [Case(530, 3, 1, _lib.KERNEL_MATERN52, False, n_pend, bounds=narrow_bounds, feasibility_only=True) for n_pend in (0, 2)]
# every feasible row below the reference point: one cell
CASES.append(Case(70, 2, 1, _lib.KERNEL_MATERN52, False, 2, one_cell=True))
IDS = [c.id for c in CASES]
