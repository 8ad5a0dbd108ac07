"""The likelihood and its gradient where the input dimension crosses the blocks the kernels walk it in -- 16 staged dimensions (KC)
in k_grad_contract, k_build_R and k_resid_gamma (csrc/kernels_pairs.hip), the pitch d | 1, the 64-dimension cap and the moving
LDS limit of k_nll_small (csrc/kernels_nllsmall.hip) -- against the CPU oracle (oracle/gp_oracle.py), for the cases of
tests/nll_dim_cases.py: d in {15, 16, 17, 31, 32, 33, 48, 63, 64, 65} at N = 100 (one launch; general path at d = 65), 200
(elimination, 16 x 16 gradient tiles), 300 (32 x 32) and 1025 (64 x 64), both sides of the four (N, d) at which the one-launch
limit gives way, every gradient kernel, mode, trend flavour and theta layout; the general path forced; batches on the NS_BPAR and
up8(d + 1) layouts at their widest; the restricted likelihood; the value-only families; a column permutation; k_min_pdist2.

Tolerances.  Log-likelihood: test_gpu_nll_fused.check's rule, 1e-10 + 8 eps cond(R) relative.  Gradient: PER COMPONENT,
|g_k - go_k| <= (TOL_G + 200 eps cond(R)) max|go| -- not a norm over the vector: tests/test_nll_dim_cases_host.py asserts that no
component of go is within 100 bounds of zero and no two are within 10 bounds of each other, so a wrong, swapped or dropped
component cannot pass.  Measured on an MI355X over the 483 gradient comparisons of this module (every path, batch slot and the
restricted likelihood; profiles/nll_dims_parity.txt): the worst |g_k - go_k| / max|go| is 6.41e-15 (N = 1025, d = 33, Matern 5/2,
component 7 of 34, cond(R) = 153; the next ones 3.98e-15 and 3.71e-15 at N = 300), the worst likelihood error 1.7e-15 relative
(cubic, cond(R) = 1.3e3).  TOL_G = 7e-14 (nll_dim_cases.py) is ten times the worst gradient error, rounded up; with 200 eps cond(R)
beside it the bound is 1.2e-13 ... 1.5e-11 over the cases, far below the cap of 3e-7 that the host test asserts for every case.
With neighbouring components swapped past the first 16-dimension block of k_grad_contract, and k_nll_small's last dimension
clamped one short, exactly the cases that run those lines with an ARD theta failed (265 of 475), the others passed.
Needs a real MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import nll_dim_cases as DC  # noqa: E402
from bogp import _lib  # noqa: E402
from oracle import philox as P  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def general_path(fn):
    os.environ["BOGP_NLL_FUSED"] = "0"
    try:
        return fn()
    finally:
        del os.environ["BOGP_NLL_FUSED"]


def args_of(c):
    par, nv = DC.parameters(c)
    return (c.kernel, c.mode, par, nv, c.est, DC.beta_of(c))


def hold_to_the_oracle(c, llf, g, what=""):
    """Value at the llf rule, every gradient component at one absolute bound; the figures are printed before they are asserted."""
    lo, go, cond = DC.oracle(c)
    err_l = abs(llf - lo) / max(1.0, abs(lo))
    line = "nll-dims %s%s cond %.3g llf_err %.3g" % (DC.case_id(c), what, cond, err_l)
    if go is not None:
        err_g = np.abs(g - go) / np.max(np.abs(go))
        line += " grad_err %.3g at k = %d of %d, bound %.3g" % (err_g.max(), int(err_g.argmax()), len(go), DC.grad_rel_bound(c))
    print(line)
    assert abs(llf - lo) <= DC.llf_bound(c)
    if go is not None:
        assert g.shape == go.shape
        bad = np.flatnonzero(~(np.abs(g - go) <= DC.grad_bound(c)))
        assert bad.size == 0, "components %s: %s against %s" % (bad, g[bad], go[bad])


def load(eng, c):
    X, y, _ = DC.problem(c.N, c.d, c.seed)
    eng.set_train(X, y)


@pytest.mark.parametrize("case", DC.DEFAULT_CASES, ids=DC.case_id)
def test_value_and_gradient_against_the_oracle(eng, case):
    assert _lib.load().bogp_nll_path(case.N, case.d, 0, 1) == DC.expected_path(case.N, case.d)
    load(eng, case)
    llf, g = eng.nll(*args_of(case), eval_grad=True)
    hold_to_the_oracle(case, llf, g)
    assert eng.nll(*args_of(case)) == pytest.approx(llf, rel=1e-13)  # value-only evaluation: the same number


@pytest.mark.parametrize("case", DC.GENERAL_CASES, ids=DC.case_id)
def test_general_path_against_the_oracle(eng, case):
    """BOGP_NLL_FUSED=0: k_build_R + the Cholesky chain + k_grad_contract at sizes the library itself gives to the elimination."""
    load(eng, case)
    llf, g = general_path(lambda: eng.nll(*args_of(case), eval_grad=True))
    hold_to_the_oracle(case, llf, g, " (general)")
    assert general_path(lambda: eng.nll(*args_of(case))) == pytest.approx(llf, rel=1e-13)


@pytest.mark.parametrize("slots", DC.BATCH_CASES, ids=lambda b: "N%d-d%d" % (b[0].N, b[0].d))
def test_batch_slots_are_the_sequential_bits_and_the_oracles_numbers(eng, slots):
    """Five different parameter vectors in one round trip: slot s is bit-identical to the s-th sequential call (bogp_nll_batch's
    contract) with 64 theta in a slot of NS_BPAR doubles (100, 64), on the per-slot general path (100, 65) and on the elimination's
    up8(d + 1) layout -- and every slot is the oracle's value and gradient."""
    c0 = slots[0]
    load(eng, c0)
    pars = np.array([DC.parameters(c)[0] for c in slots])
    nv = DC.parameters(c0)[1]
    seq = [eng.nll(*args_of(c), eval_grad=True) for c in slots]
    l, g, info = eng.nll_batch(c0.kernel, c0.mode, pars, nv, c0.est, DC.beta_of(c0), eval_grad=True)
    assert np.all(info == _lib.OK)
    np.testing.assert_array_equal(l, [s[0] for s in seq])
    np.testing.assert_array_equal(g, [s[1] for s in seq])
    for s, c in enumerate(slots):
        hold_to_the_oracle(c, l[s], g[s])
    l0, g0, info0 = eng.nll_batch(c0.kernel, c0.mode, pars, nv, c0.est, DC.beta_of(c0), eval_grad=False)
    assert g0 is None and np.all(info0 == _lib.OK)
    np.testing.assert_array_equal(l0, [eng.nll(*args_of(c)) for c in slots])


@pytest.mark.parametrize("case", DC.REML_CASES, ids=DC.case_id)
def test_restricted_likelihood_against_the_oracle(eng, case):
    """gpr.py:813-918 with an estimated constant trend: k_grad_contract with the (L^-T Q)(L^-T Q)^T term (qv) past the first block."""
    load(eng, case)
    llf, g = eng.nll_restricted(*args_of(case), eval_grad=True)
    hold_to_the_oracle(case, llf, g)
    assert eng.nll_restricted(*args_of(case)) == pytest.approx(llf, rel=1e-13)


@pytest.mark.parametrize("case", DC.VALUE_ONLY_CASES, ids=DC.case_id)
def test_value_only_families_against_the_oracle(eng, case):
    """cubic and generalized_exponential have no theta-derivative: k_build_R's own dist_fold over three blocks of dimensions."""
    load(eng, case)
    hold_to_the_oracle(case, eng.nll(*args_of(case)), None)
    if DC.expected_path(case.N, case.d) != DC.PATH_GENERAL:
        hold_to_the_oracle(case, general_path(lambda: eng.nll(*args_of(case))), None, " (general)")


@pytest.mark.parametrize("case", DC.PERMUTED_CASES, ids=DC.case_id)
def test_reversed_columns_give_the_reversed_gradient(eng, case):
    """X and theta with their columns reversed: the same model, so the same value and the gradient's theta entries in reverse order --
    the kc + kk indexing of the gradient pinned without the oracle.  (Dimension k then sits in another block and at another place
    of it: 33 -> blocks of 16 | 16 | 1, so old block 0 is spread over new blocks 1 and 2.)"""
    load(eng, case)
    llf, g = eng.nll(*args_of(case), eval_grad=True)
    X, y, _ = DC.problem(case.N, case.d, case.seed)
    par, nv = DC.parameters(case)
    eng.set_train(X[:, ::-1], y)
    llf_r, g_r = eng.nll(case.kernel, case.mode, np.r_[par[:-1][::-1], par[-1]], nv, case.est, DC.beta_of(case), eval_grad=True)
    err = np.abs(np.r_[g_r[:-1][::-1], g_r[-1]] - g) / np.max(np.abs(g))
    print("nll-dims %s (reversed) llf_err %.3g grad_err %.3g" % (DC.case_id(case), abs(llf_r - llf) / max(1.0, abs(llf)), err.max()))
    assert abs(llf_r - llf) <= DC.llf_bound(case)
    assert np.all(err <= 2 * DC.grad_rel_bound(case))
    assert not np.all(np.abs(g_r[:-1] - g[:-1]) / np.max(np.abs(g)) <= 2 * DC.grad_rel_bound(case))  # (the reversal is no identity)


@pytest.mark.parametrize("M,d", DC.PDIST_SHAPES)
def test_min_pairwise_distance_past_the_first_block_of_dimensions(eng, M, d):
    """k_min_pdist2 stages the coordinates as k_build_R does; its sum is sequential and uncontracted, so the result is exact."""
    rng = np.random.default_rng(100 * d + M)
    eng.set_train(rng.uniform(-3, 3, size=(8, d)), rng.standard_normal((8, 1)))  # (the handle takes its dimension from the training set)
    Xs = rng.uniform(-3, 3, size=(M, d))
    eng.upload_candidates(Xs)
    assert eng.min_pairwise_distance() == P.min_pdist(Xs)
    Xs[M - 1, : d - 1] = Xs[0, : d - 1]  # the closest pair now differs in the LAST dimension only: dropping it would give 0
    Xs[M - 1, d - 1] = Xs[0, d - 1] + 1e-3
    eng.upload_candidates(Xs)
    assert eng.min_pairwise_distance() == P.min_pdist(Xs) > 0.0
