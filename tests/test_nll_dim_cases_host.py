"""CPU companion of tests/test_gpu_nll_dims.py: the conditions under which that test's per-component gradient bound cannot let a
wrong, swapped or dropped component through, checked in the oracle alone for every case of tests/nll_dim_cases.py -- none is
skipped or filtered; one that misses a condition is replaced in nll_dim_cases.py (RESEEDED).  With go the oracle's gradient and
b = TOL_G + 200 eps cond(R) the device test's bound relative to max|go|:
  * b <= 3e-7, the cap up to which the cases were chosen;
  * min_k |go_k| >= 100 b max|go|: a component that is dropped (left at zero, or at another tile's value) is 100 bounds off;
  * any two components differ by >= 10 b max|go|: two swapped components are 10 bounds off.
The conditions are asserted at the bound in use and at the cap itself, so they hold for whatever TOL_G a later measurement sets.
And which path bogp_nll_path chooses on both sides of every (N, d) at which k_nll_small's LDS test or its 64-dimension cap gives
way, the expected side derived from that test's formula as restated in nll_dim_cases.one_launch_fits (no device needed).
"""
import os
import re

import numpy as np
import pytest

import nll_dim_cases as DC
from bogp import _lib
from oracle import gp_oracle as O

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bogp.h")


@pytest.mark.parametrize("case", DC.GRADIENT_CASES, ids=DC.case_id)
def test_no_gradient_component_vanishes_or_coincides_with_another(case):
    llf, go, cond = DC.oracle(case)
    assert np.isfinite(llf) and llf <= 0.0  # (the reference rejects the parameters otherwise, gpr.py:981-982)
    assert np.all(np.isfinite(go)) and len(go) == len(DC.parameters(case)[0])
    assert DC.TOL_G <= DC.grad_rel_bound(case) <= DC.TOL_G_CAP
    top = np.max(np.abs(go))
    gaps = np.diff(np.sort(go))
    for b in (DC.grad_rel_bound(case), DC.TOL_G_CAP):
        assert np.min(np.abs(go)) >= 100 * b * top, (np.min(np.abs(go)) / top, b)
        assert len(go) == 1 or np.min(gaps) >= 10 * b * top, (np.min(gaps) / top, b)


@pytest.mark.parametrize("case", DC.VALUE_ONLY_CASES, ids=DC.case_id)
def test_value_only_cases_have_a_finite_likelihood(case):
    llf, go, cond = DC.oracle(case)
    assert go is None and np.isfinite(llf) and llf <= 0.0
    assert 8 * DC.EPS * cond <= 1e-10  # the llf bound stays at its floor: 1e-10 relative


def test_case_list_covers_every_dimension_block_and_path():
    """Every row count with every dimension edge and gradient kernel on the default path; at N = 200 every mode, trend flavour and
    theta layout on every edge, and all five kernels among them; the three tile sides of k_grad_contract; no duplicates."""
    cs = DC.DEFAULT_CASES
    plain = {(c.N, c.d, c.kernel) for c in cs if c.mode == O.MODE_NOISY and c.est and not c.iso}
    assert plain >= {(N, d, k) for N in DC.ROWS for d in DC.D_EDGES for k in DC.GRAD_KERNELS}
    assert plain >= {(N, d, k) for N, d in DC.LDS_EDGES for k in DC.GRAD_KERNELS}
    assert plain >= {(DC.N_TILE64, d, O.KERNEL_MATERN52) for d in DC.D_TILE64}
    at200 = {(c.d, c.mode, c.est, c.iso) for c in cs if c.N == 200}
    assert at200 == {(d, m, e, i) for d in DC.D_EDGES for m in DC.MODES for e in (True, False) for i in (True, False)}
    assert {c.kernel for c in cs if c.N == 200 and c.mode != O.MODE_NOISY} == set(DC.GRAD_KERNELS)
    assert max(c.N for c in DC.ALL_CASES) == DC.N_TILE64
    assert {1 if N <= 256 else 2 if N <= 1024 else 4 for N in DC.ROWS + (DC.N_TILE64,)} == {1, 2, 4}  # points a thread and tile side / 16
    assert {c.N for c in DC.GENERAL_CASES} == {200, DC.N_TILE64} and len(DC.GENERAL_CASES) >= 5 * len(DC.D_EDGES) + 2
    assert [len(b) for b in DC.BATCH_CASES] == [DC.BATCH_P] * len(DC.BATCH_SHAPES)
    assert [(b[0].N, b[0].d) for b in DC.BATCH_CASES] == list(DC.BATCH_SHAPES)
    for b in DC.BATCH_CASES:  # five DIFFERENT vectors
        pars = np.array([DC.parameters(c)[0] for c in b])
        assert all(np.all(pars[i] != pars[j]) for i in range(len(b)) for j in range(i))
    assert len(set(DC.ALL_CASES)) == len(DC.ALL_CASES) and len({DC.case_id(c) for c in DC.ALL_CASES}) == len(DC.ALL_CASES)
    assert all(c.seed == 0 or c.seed % 1000000 == 1000 * c.N + c.d for c in DC.ALL_CASES)
    for N, d in {(c.N, c.d) for c in DC.ALL_CASES}:  # no two dimensions share a length scale
        theta = DC.problem(N, d)[2]
        assert len(np.unique(theta)) == d


LDS_PAIRS = [(156, 21, 22), (144, 35, 36), (128, 57, 58), (100, 64, 65), (1, 64, 65)]


def test_one_launch_limit_moves_with_the_dimension_as_its_lds_formula_says():
    """bogp_nll_path at the four pairs where X at pitch d | 1 + the block image + 36 KB of static LDS cross 160 KB (or d crosses the
    64 theta of the kernel's arguments), and at (N, 64) | (N, 65) for N = 1 and 100: one launch on the near side; on the far side
    the elimination where ld >= 192 (N = 144, 156), the general path where ld = 128 (N = 100, 128) or 64 (N = 1)."""
    consts = dict(re.findall(r"#define\s+(BOGP_[A-Z_0-9]+)\s+\(?(-?\d+)\)?", open(HEADER).read()))
    general, one, elim = (int(consts["BOGP_NLL_PATH_" + k]) for k in ("GENERAL", "ONE_LAUNCH", "ELIM"))
    assert (general, one, elim) == (DC.PATH_GENERAL, DC.PATH_ONE_LAUNCH, DC.PATH_ELIM)
    assert DC.LDS_EDGES == tuple((N, d) for N, near, far in LDS_PAIRS[:4] for d in (near, far))
    p = _lib.load().bogp_nll_path
    for N, near, far in LDS_PAIRS:
        assert DC.one_launch_fits(N, near) and not DC.one_launch_fits(N, far), (N, near, far)
        assert p(N, near, 0, 1) == DC.expected_path(N, near) == one, (N, near)
        want = elim if N in (144, 156) else general
        assert p(N, far, 0, 1) == DC.expected_path(N, far) == want, (N, far)
    for N, near, far in LDS_PAIRS[:3]:  # the pitch is d | 1: the limit can only move where d goes from odd to even
        assert near % 2 == 1 and far == near + 1
    assert DC.one_launch_fits(156, 1) and not DC.one_launch_fits(157, 1)
    # and every (N, d) the device test runs takes the path this module expects
    for N, d in sorted({(c.N, c.d) for c in DC.ALL_CASES}):
        assert p(N, d, 0, 1) == DC.expected_path(N, d), (N, d)
    assert {DC.expected_path(c.N, c.d) for c in DC.DEFAULT_CASES} == {general, one, elim}
