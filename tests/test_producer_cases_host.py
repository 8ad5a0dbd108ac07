"""CPU companion of tests/test_gpu_producer_a.py: the preconditions under which that test's unconditional assertions are licensed,
checked in the oracle for every case of tests/producer_cases.py (and for the cubic rows that module adds to
test_fused_small_sweep_equals_the_chunked_schedule_and_the_oracle).  No case is skipped: one that misses a condition is replaced
in producer_cases.py.
  * the likelihood is finite (the reference rejects the parameters otherwise, gpr.py:981-982);
  * cond of the factorised matrix <= 1e9, the cap of test_randomised_configurations_match_the_oracle: beyond it the oracle's own
    rounding reaches the 1e-6 tolerances;
  * winner and runner-up of every criterion are >= 1e-4 apart, relative: two orders above the 1e-6 tolerance on the values, so a
    correct device cannot pick another row;
  * rows whose MSE is rounding noise (<= 1e-9 sigma2: MGFI is not compared there) are at most the 200 on / near rows, <= 12 %.
"""
import numpy as np
import pytest

import producer_cases as PC
from oracle import gp_oracle as O

COND_CAP = 1e9
MIN_GAP = 1e-4
MAX_NOISE_SHARE = 0.12


@pytest.mark.parametrize("case", PC.CASES + [c for pair in PC.IDENTITIES for c in pair], ids=PC.case_id)
def test_case_is_feasible_and_has_clear_winners(case):
    o = PC.oracle(case)  # raises LinAlgError where the likelihood is -inf
    assert np.isfinite(o["llf"]) and o["llf"] <= 0.0
    assert o["sigma2"] == PC.SIGMA2_PAR
    cond = PC.correlation_cond(o["st"])
    assert cond <= COND_CAP, cond
    assert np.all(np.isfinite(o["mu"])) and np.all(np.isfinite(o["mse"])) and np.all(np.isfinite(o["vals"]))
    assert np.all(o["gaps"] >= MIN_GAP), o["gaps"]
    noise = o["mse"][: PC.M_STACK] <= 1e-9 * o["sigma2"]
    assert noise.mean() <= MAX_NOISE_SHARE
    assert not np.any(noise[PC.N_ON + PC.N_NEAR :])  # only rows on or beside a training point
    # the small batches (constant trend only) have their own winners: rows ON training points, where only UCB is compared, and box rows
    if PC.trend_size(case) == 1:
        assert noise[: PC.SMALL_M].all() and not noise[PC.SMALL_BOX].any()
        assert PC.relative_gaps(o["vals"][2:, : PC.SMALL_M])[0] >= MIN_GAP and PC.ACQ[2][0] == O.ACQ_UCB
        sub = PC.relative_gaps(o["vals"][:, PC.SMALL_BOX])
        assert np.all(sub >= MIN_GAP), sub


def test_far_block_reaches_the_prior_where_the_support_ends():
    """The +-60 block does what it is there for: for cubic at least one row has every training point outside the support (r = 0
    exactly: mu = beta, MSE = (1 + u^2) sigma2 >= sigma2), and the exponential kernels underflow to r = 0.0 on some row."""
    for c in PC.CASES:
        if c.kernel != O.KERNEL_CUBIC or c.trend != O.TREND_CONSTANT:
            continue
        b, o = PC.build(c), PC.oracle(c)
        outside = np.all(np.max(np.abs(b["Xall"][PC.M_STACK :, None, :] - b["X"][None, :, :]), axis=2) * c.theta >= 1.0, axis=1)
        assert outside.any(), PC.case_id(c)
        assert np.all(o["mse"][PC.M_STACK :][outside] >= o["sigma2"])
        assert np.all(o["mu"][PC.M_STACK :][outside] == o["st"].beta[0, 0])


def test_case_list_covers_the_boundaries():
    ps = {PC.trend_size(c) for c in PC.FAMILY2}
    assert {16, 17, 32, 33} <= ps and any(1 < p <= 15 for p in ps)
    assert all(PC.trend_size(c) == 1 for c in PC.FAMILY1)
    assert {c.kernel for c in PC.FAMILY1} == {O.KERNEL_ABSEXP, O.KERNEL_CUBIC, O.KERNEL_GENEXP, O.KERNEL_MATERN_NU}
    assert {c.kernel for c in PC.FAMILY2} >= {O.KERNEL_ABSEXP, O.KERNEL_CUBIC, O.KERNEL_GENEXP, O.KERNEL_MATERN_NU}  # PV > 0 with them too
    for k in (O.KERNEL_CUBIC, O.KERNEL_MATERN_NU):  # the low-dimension rows stand in for d = 1
        assert min(c.d for c in PC.FAMILY1 if c.kernel == k) == 2
    assert {c.d for c in PC.FAMILY1 if c.kernel in (O.KERNEL_ABSEXP, O.KERNEL_GENEXP)} >= {1, 7, 20, 50}
    assert all(c.N > 512 for c in PC.CASES)  # the chunked schedule for absolute_exponential and cubic as well
    assert {PC.slices(c.N) for c in PC.CASES} >= {3, 4}
    assert all(PC.chunks_1mib(c) >= 8 for c in PC.CASES) and PC.M_STACK % 64 != 0
    # the chunk count at 1 MiB tells the trend-rows path from the fused one (what the device test reads from last_timing)
    assert all(PC.chunks_1mib(c, trend_rows=True) != PC.chunks_1mib(c, trend_rows=False) for c in PC.FAMILY2)
    assert len(set(PC.CASES)) == len(PC.CASES) and len({PC.case_id(c) for c in PC.CASES}) == len(PC.CASES)


def test_identity_pairs_agree_exactly_in_the_oracle():
    for a, b in PC.IDENTITIES:
        oa, ob = PC.oracle(a), PC.oracle(b)
        assert np.array_equal(PC.build(a)["X"], PC.build(b)["X"]) and np.array_equal(PC.build(a)["Xall"], PC.build(b)["Xall"])
        assert oa["llf"] == ob["llf"]
        np.testing.assert_array_equal(oa["mu"], ob["mu"])
        np.testing.assert_array_equal(oa["mse"], ob["mse"])
        np.testing.assert_array_equal(oa["idx"], ob["idx"])


@pytest.mark.parametrize("N,d", PC.DRIVER_CUBIC)
def test_cubic_rows_of_the_fused_small_sweep_test(N, d):
    """The two cubic rows of tests/test_gpu_driver.py, on that test's own data and candidates: one on the four-wave schedule of
    k_sweep_small, one on the eight-wave one; the same conditions, for its four criteria at each of its candidate counts (that test
    lets the argmax go only when the oracle's winner is the row ON a training point)."""
    assert PC.padded_rows(PC.DRIVER_CUBIC[0][0]) <= 256 and PC.DRIVER_CUBIC[0][1] <= 32 and 256 < PC.DRIVER_CUBIC[1][0] <= 512
    rng, X, y, par, nv = PC.driver_model(N, d, O.MODE_NOISY)
    st = O.make_state(par, X, y, O.KERNEL_CUBIC, O.MODE_NOISY, nv, estimate_trend=True, beta=0.0)
    assert np.isfinite(st.llf) and st.llf <= 0.0
    assert PC.correlation_cond(st) <= COND_CAP
    for M in PC.DRIVER_MS:
        Xs = PC.driver_candidates(rng, X, M)
        mu, mse = O.predict_chunked(st, Xs, 512)
        vals = PC.criteria(st, mu[:, 0], mse[:, 0], float(y.min()), PC.DRIVER_ACQ)
        assert np.all(np.isfinite(vals))
        gaps = PC.relative_gaps(vals)
        assert np.all(gaps >= MIN_GAP), (M, gaps)
        assert np.mean(mse[:, 0] <= 1e-9 * float(st.sigma2[0])) <= MAX_NOISE_SHARE
