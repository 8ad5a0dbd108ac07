"""The pruned sweep's two rules on the host (no GPU): acq_upper_bound (csrc/bogp_device.h, through bogp_acq_upper_bound)
dominates the oracle's criterion for every standard deviation in [0, sd_ub], and the prune test (bogp_prune_below) only fires
for a bound strictly below a finite, normal threshold.  Also: the oracle's count of what the bound lets through on the
inputs of tests/test_gpu_prune.py, so that its peaked cases cannot pass vacuously."""
import numpy as np
import pytest

import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI


def _bound(a_id, par, y_hat, sd_ub, plugin, s2):
    return float(_lib.load().bogp_acq_upper_bound(int(a_id), float(par), float(y_hat), float(sd_ub), float(plugin), float(s2)))


def _below(bound, thr):
    return bool(_lib.load().bogp_prune_below(float(bound), float(thr)))


@pytest.mark.parametrize("a_id,pars", [(EI, (0.0,)), (PI, (0.0, 0.05, 0.5, 1.5)), (UCB, (0.5, 50.0, -0.5, -3.0)), (MGFI, (0.5, 2.0, 10.0, 30.0))])
def test_bound_dominates_the_criterion_on_the_whole_range(a_id, pars):
    """Random (y_hat, plugin, sigma2) on both sides of plugin - y_hat and in the tail z in [-37, -20] (PC.domination_cases, shared with
    the device's run of the same property in tests/test_gpu_criteria.py), every parameter, sd on a grid over [0, sd_ub]: the oracle's
    value never exceeds the bound by more than the prune margin -- i.e. the prune test, given that value as the threshold, would
    not prune the row itself -- and a NaN value only occurs where the bound is +inf or NaN."""
    assert pars == PC.DOMINATION_PARS[a_id]
    worst = 0.0
    for s2, plugin, y_hat, sd_ub in PC.domination_cases(a_id):
        sd = PC.sd_grid(sd_ub, s2)
        for par in pars:
            b = _bound(a_id, par, y_hat, sd_ub, plugin, s2)
            with np.errstate(all="ignore"):
                v = O.acquisition(a_id, par, np.full(len(sd), y_hat), sd * sd, plugin, s2, True)
            if np.any(np.isnan(v)):
                assert np.isnan(b) or b == np.inf, (a_id, par, y_hat, plugin, sd_ub)
                continue
            if np.isnan(b) or b == np.inf:
                continue  # never pruned
            slack = v - (b + PC.prune_margin(b, v))
            worst = max(worst, float(slack.max()))
            assert np.all(slack <= 0), (a_id, par, y_hat, plugin, s2, sd_ub, float(sd[int(np.argmax(slack))]), b, float(v.max()))
            assert not any(_below(b, float(x)) for x in v)
    assert worst <= 0.0


def test_bound_rules_for_nan_and_infinity():
    s2, nan, inf = 0.5, float("nan"), float("inf")
    # EpsilonPI: num > 0 -> 1; num == 0 -> +inf (the value is NaN at sd = 0, and a NaN wins the argmax); num < 0 -> ndtr(num / sd_ub)
    assert _bound(PI, 0.0, 1.0, 0.3, 2.0, s2) == 1.0
    assert _bound(PI, 0.0, 2.0, 0.3, 2.0, s2) == inf
    assert np.isnan(O.acquisition(PI, 0.0, np.array([2.0]), np.array([0.0]), 2.0, s2, True)[0])
    assert 0.0 < _bound(PI, 0.0, 2.5, 0.3, 2.0, s2) < 0.05
    assert _bound(PI, 0.0, 2.5, 0.0, 2.0, s2) == 0.0
    # UCB: par >= 0 -> y_hat + par sd_ub, par < 0 -> y_hat (sd = 0 is the best case)
    assert _bound(UCB, 2.0, 1.0, 0.25, 0.0, s2) == 1.5 and _bound(UCB, -2.0, 1.0, 0.25, 0.0, s2) == 1.0
    # MGFI: t < 0 -> +inf; an overflowing bound -> +inf, although the criterion itself returns 0 there and is large just below
    assert _bound(MGFI, -1.0, 0.0, 0.3, 0.0, s2) == inf
    assert _bound(MGFI, 22.0, -40.0, 3.0, 0.0, s2) == inf and _bound(MGFI, 22.0, 5.0, 30.0, 0.0, s2) == inf
    assert _bound(MGFI, 2.0, 1.0, 1e-9, 0.0, s2) == 0.0  # y_hat >= plugin and the whole range inside the guard
    # a NaN in y_hat or sd_ub: NaN or +inf, and the prune test never fires on either
    for a_id, par in ((EI, 0.0), (PI, 0.05), (UCB, 0.5), (UCB, -0.5), (MGFI, 2.0)):
        for y_hat, sd_ub in ((nan, 0.3), (1.0, nan), (nan, nan)):
            b = _bound(a_id, par, y_hat, sd_ub, 0.0, s2)
            if a_id == UCB and par < 0 and not np.isnan(y_hat):
                assert b == y_hat  # sd_ub does not enter; mu and sd share their NaNs on the device (both come from the row's r)
                continue
            assert np.isnan(b) or b == inf, (a_id, par, y_hat, sd_ub, b)
            assert not _below(b, 1.0) and not _below(b, inf)


def test_prune_test_margin_and_thresholds():
    inf, nan = float("inf"), float("nan")
    assert _below(1.0, 2.0) and _below(-5.0, -3.0) and _below(0.0, 1e-290)
    assert not _below(2.0, 2.0) and not _below(2.0 * (1 - 1e-12), 2.0)  # within the margin: a tie stays a tie for the index rule
    assert _below(2.0 * (1 - 1e-8), 2.0)
    assert not _below(0.0, 0.0) and not _below(0.0, 5e-324) and not _below(0.0, 1e-310) and not _below(0.0, 1e-300)  # zero / subnormal thresholds
    assert not _below(-inf, inf) and not _below(0.0, nan) and not _below(0.0, -inf) and not _below(nan, 1.0) and not _below(inf, 1.0)
    assert not _below(-inf, 0.0)  # (the margin of an infinite bound is infinite: -inf + inf is a NaN, and the row is simply kept)


@pytest.fixture(scope="module")
def peaked():
    X, y, par, st = PC.model(False)
    return st, PC.candidates(), float(y.min())


@pytest.mark.parametrize("acq", [[(EI, 0.0)], [(MGFI, 2.0)], [(MGFI, 2.0), (EI, 0.0)]])
@pytest.mark.parametrize("where", [1500, 2990])
def test_oracle_count_of_survivors_on_the_peaked_inputs(peaked, acq, where):
    """What tests/test_gpu_prune.py relies on: with the winner in a middle chunk or in the last one, the rows whose bound reaches
    the threshold the 192-row pilot sets are fewer than a quarter of all rows (and no row's exact value exceeds its bound)."""
    st, Xs, pl = peaked
    Xw = PC.place_winner(st, Xs, acq, pl, where)
    assert PC.surviving_fraction(st, Xw, acq, pl) < 0.25
    mu, mse, sd_ub = PC.oracle_rows(st, Xw)
    for a_id, a_par in acq:
        v = O.acquisition(a_id, a_par, mu, mse, pl, float(st.sigma2[0]), True)
        b = PC.upper_bounds(a_id, a_par, mu, sd_ub, pl, float(st.sigma2[0]))
        assert np.all(v <= b + PC.prune_margin(b, v))


def test_flat_landscape_prunes_nothing_in_the_oracle(peaked):
    st, Xs, pl = peaked
    assert PC.surviving_fraction(st, Xs, [(UCB, 50.0)], pl) == (len(Xs) - PC.CHUNK_ROWS) / len(Xs)
