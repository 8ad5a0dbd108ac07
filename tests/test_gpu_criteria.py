"""The scalar criterion functions of csrc/bogp_device.h ON THE DEVICE, at arguments the test chooses (ledger T20): ndtr, norm_pdf,
ehvi_G, acq_value (EI, EpsilonPI, UCB, MGFI), feasibility, acq_upper_bound, acq_upper_bound_interval and prune_below through
`bogp_selftest_criteria`, whose kernel calls the functions themselves.

a. accuracy: every criterion against the committed truth table tests/golden/G46_criteria_truth.npz (mpmath at the double inputs,
   oracle/make_criteria_table.py) within F x its allowance, F = 4 x the reference's own worst ratio (tests/criteria_cases.py), and
   never further from the reference's value than the reference is from the truth, + F allowances;
b. the guards, switch points and non-finite inputs, compared with == / isnan;
c. the two domination properties of the pruned sweep (tests/test_prune_bounds_host.py, tests/test_bound32_host.py: the same rows)
   with every value computed on the device, and the device's bounds against the host's within 2 F allowances;
d. the instrument measures what the sweeps run: ACQ_VALUE / FEASIBILITY at the moments a path reports return the bytes that path stored;
e. the entry point's error returns."""
import ctypes as C

import numpy as np
import pytest

import bound32_cases as BC
import criteria_cases as CC
import prune_cases as PC
from conftest import load_golden
from bogp import _lib

pytestmark = pytest.mark.gpu

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
NAME = {EI: "EI", PI: "PI", UCB: "UCB", MGFI: "MGFI"}
INF, NAN = float("inf"), float("nan")
ACQ4 = [(EI, 0.0), (PI, 0.05), (UCB, 0.5), (MGFI, 2.0)]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _value(eng, a_id, par, y_hat, sd, plugin, s2):
    return eng.selftest_criteria(_lib.CRITERIA_ACQ_VALUE, a_id, par, y_hat, sd, plugin, s2)


def _bound(eng, a_id, par, y_hat, sd_ub, plugin, s2):
    return eng.selftest_criteria(_lib.CRITERIA_ACQ_UPPER_BOUND, a_id, par, y_hat, sd_ub, plugin, s2)


def _interval(eng, a_id, par, y32, e, sd_ub, plugin, s2):
    return eng.selftest_criteria(_lib.CRITERIA_ACQ_UPPER_BOUND_INTERVAL, a_id, par, y32, e, sd_ub, plugin, s2)


def _below(eng, bound, thr):
    return eng.selftest_criteria(_lib.CRITERIA_PRUNE_BELOW, bound, thr)


# ----------------------------------------------------------------------------------------------------------------------
# a. accuracy against the truth table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.NAMES)
def test_device_value_against_the_truth_table(eng, name):
    """Measured on an MI355X (worst |device - exact| / allowance; F): see README, ledger row T20."""
    g = load_golden("G46_criteria_truth")
    c = CC.draw(name)
    assert CC.checksum(c) == float(g[name + "_checksum"])
    true, rlo = g[name + "_true"], g[name + "_rlo"]
    allow = CC.allowance(name, c, true)
    sel, cols = CC.device_columns(name, c)
    dev = eng.selftest_criteria(getattr(_lib, sel), *cols)
    ref = CC.reference(name, c)
    r_dev, cmp = CC.ratios(dev, true, rlo, allow)
    r_ref, _ = CC.ratios(ref, true, rlo, allow)
    w = int(np.argmax(r_dev))
    print("T20 %-12s device: worst |value - exact| / allowance = %.4g (z = %.6g), median %.3g; reference %.4g; F = %d; %d of %d rows compared"
          % (name, r_dev.max(), c["z"][cmp][w], np.median(r_dev), r_ref.max(), CC.F[name], cmp.sum(), len(cmp)))  # fmt: skip
    assert cmp.sum() >= 0.95 * len(cmp)
    assert CC.tiny_rows_ok(dev, cmp)
    assert r_dev.max() <= CC.F[name], {k: float(v[cmp][w]) for k, v in c.items()}
    # never further from the reference than the reference is from the truth, + F allowances
    gap = np.abs(dev - ref)[cmp] / allow[cmp]
    assert np.all(gap <= r_ref + CC.F[name]), float(np.max(gap - r_ref))


# ----------------------------------------------------------------------------------------------------------------------
# b. exact cases
# ----------------------------------------------------------------------------------------------------------------------
def test_guards_of_ei_and_mgfi(eng):
    for s2 in (1.0, 1e-8, 1e8):  # (1e8 is what k_forest passes)
        under, over = 0.999e-6 * np.sqrt(s2), 1.001e-6 * np.sqrt(s2)
        v = _value(eng, EI, 0.0, [0.0, 0.0, 2.0, 2.0], [under, over, under, over], 1.0, s2)
        assert v[0] == 0.0 and v[1] == 1.0 and v[2] == 0.0, (s2, v)  # xcr = 1 / sd ~ 1e6 / sqrt(s2): Phi = 1, phi = 0 above the guard
        assert v[3] == 0.0 or s2 == 1e8                             # xcr_ = -1: EI underflows unless sd = 0.01 lets it live
        v = _value(eng, EI, 0.0, 1.0 - 2.0 * over, [under, over], 1.0, s2)  # xcr = 2 at the guard's edge
        assert v[0] == 0.0 and v[1] > 2.0 * over and np.isfinite(v[1]), (s2, v)
        edge = below = 1e-6 * np.sqrt(s2)  # the guard is `<`: exactly 1e-6 is evaluated, the next quotient below it is not
        while below / np.sqrt(s2) >= 1e-6:
            below = np.nextafter(below, 0)
        assert edge / np.sqrt(s2) == 1e-6 and edge - below <= 2 * np.spacing(edge)
        v = _value(eng, EI, 0.0, 0.0, [edge, below], 1.0, s2)
        assert v[0] == 1.0 and v[1] == 0.0, (s2, v)
        mse_edge = mse_below = 1e-12 * s2  # feasibility has the same guard, on sqrt(mse)
        while np.sqrt(mse_below) / np.sqrt(s2) >= 1e-6:
            mse_below = np.nextafter(mse_below, 0)
        assert np.sqrt(mse_edge) / np.sqrt(s2) == 1e-6 and mse_edge - mse_below <= 4 * np.spacing(mse_edge)
        v = eng.selftest_criteria(_lib.CRITERIA_FEASIBILITY, 1.0, [mse_edge, mse_below], s2, -1.0, 1.0)
        assert v[0] == 0.5 and v[1] == 1.0, (s2, v)  # mu on hi: the probability is Phi(0) - Phi(-2 / sd), the indicator 1
    v = _value(eng, MGFI, 2.0, 0.0, [1e-8, -1e-8, np.nextafter(1e-8, 0), 1.0001e-8, np.nextafter(1e-8, 1)], 0.5, 1.0)
    assert np.all(v[:3] == 0.0) and np.all(v[3:] > 0.0) and v[3] == v[4], v
    np.testing.assert_allclose(v[3], np.exp(2.0 * (0.5 - 0.0 - 1.0)), rtol=1e-12)  # Phi(0.5 / 1e-8) = 1


def test_mgfi_clamps_its_parameter_and_selects_zero_on_overflow(eng):
    c = CC.draw("MGFI")
    args = (c["y_hat"], c["sd"], c["plugin"], 1.0)
    at_max = _value(eng, MGFI, CC.T_MAX, *args)
    assert _value(eng, MGFI, 30.0, *args).tobytes() == at_max.tobytes()
    assert _value(eng, MGFI, INF, *args).tobytes() == at_max.tobytes()
    assert np.count_nonzero(at_max) > 0.5 * len(at_max) and _value(eng, MGFI, 22.0, *args).tobytes() != at_max.tobytes()
    # exp overflows: 22 (0 + 40 - 1) = 858 > 709.78; and a product that is finite x inf never leaves
    v = _value(eng, MGFI, [22.0, 22.0, 30.0, 5.0], [-40.0, 5.0, -40.0, -150.0], [3.0, 30.0, 1.0, 1.0], 0.0, 1.0)
    assert np.array_equal(v, np.zeros(4)), v
    just_under = _value(eng, MGFI, 22.0, -31.0, 1.0, 0.0, 1.0)  # 22 x 30 + 242 = 902 > 709: still 0 ...
    assert just_under[0] == 0.0
    big = _value(eng, MGFI, 22.0, -20.0, 1.0, 0.0, 1.0)  # ... and 22 x 19 + 242 = 660: finite and huge
    assert np.isfinite(big[0]) and big[0] > 1e280


def test_epsilon_pi_at_zero_deviation(eng):
    v = _value(eng, PI, [0.0, 0.0, 0.0, 0.05, 0.05], [1.0, 3.0, 2.0, 1.0, -1.0], 0.0, [2.0, 2.0, 2.0, 0.95, -1.05], 1.0)
    assert v[0] == 1.0 and v[1] == 0.0 and np.isnan(v[2]), v  # num > 0, < 0, == 0
    assert np.isnan(v[3]) and np.isnan(v[4]), v                # coef = 1 - / + eps on either side of y_hat = 0: num == 0 again
    v = _value(eng, PI, 0.05, [1.0, -1.0], 0.0, [0.96, -1.04], 1.0)
    assert v[0] == 1.0 and v[1] == 1.0


def test_ndtr_at_its_ends(eng):
    v = eng.selftest_criteria(_lib.CRITERIA_NDTR, [INF, -INF, NAN, 0.0, 40.0, -40.0])
    assert v[0] == 1.0 and v[1] == 0.0 and np.isnan(v[2]) and v[3] == 0.5 and v[4] == 1.0 and v[5] == 0.0
    # The subnormal range.  Phi(-38) = 2.885e-316 and Phi(-38.4) = 6.6e-323 are subnormal doubles; Phi(-38.5) = 1.408e-324 lies under
    # half the smallest one (4.94e-324 / 2), so that its correctly rounded double is 0 and 4.94e-324 is the nearest alternative.
    v = eng.selftest_criteria(_lib.CRITERIA_NDTR, [-38.0, -38.4, -38.5, -37.5])
    print("T20 ndtr in the subnormal range: ndtr(-38) = %r, ndtr(-38.4) = %r, ndtr(-38.5) = %r, ndtr(-37.5) = %r" % tuple(v))
    assert v[3] > 0 and abs(v[3] / 4.605353009581954e-308 - 1.0) <= CC.F["ndtr"] * CC.EPS * (1 + 37.5**2)
    assert 0.0 < v[0] < 2.3e-308 and abs(v[0] - 2.88542835e-316) <= CC.F["ndtr"] * CC.EPS * (1 + 38.0**2) * 2.88542835e-316 + 5e-324, v
    assert 0.0 < v[1] <= 7.5e-323 and abs(v[1] - 6.6016e-323) <= 5e-324, v
    assert v[2] == 0.0 or v[2] == 5e-324, v


def test_bounds_for_nan_and_infinity_as_the_host_test_states_them(eng):
    s2 = 0.5
    b = lambda a, par, y, sd, pl: float(_bound(eng, a, par, y, sd, pl, s2)[0])  # noqa: E731
    assert b(PI, 0.0, 1.0, 0.3, 2.0) == 1.0
    assert b(PI, 0.0, 2.0, 0.3, 2.0) == INF
    assert np.isnan(_value(eng, PI, 0.0, 2.0, 0.0, 2.0, s2)[0])
    assert 0.0 < b(PI, 0.0, 2.5, 0.3, 2.0) < 0.05
    assert b(PI, 0.0, 2.5, 0.0, 2.0) == 0.0
    assert b(UCB, 2.0, 1.0, 0.25, 0.0) == 1.5 and b(UCB, -2.0, 1.0, 0.25, 0.0) == 1.0
    assert b(MGFI, -1.0, 0.0, 0.3, 0.0) == INF
    assert b(MGFI, 22.0, -40.0, 3.0, 0.0) == INF and b(MGFI, 22.0, 5.0, 30.0, 0.0) == INF
    assert b(MGFI, 2.0, 1.0, 1e-9, 0.0) == 0.0
    for a_id, par in ((EI, 0.0), (PI, 0.05), (UCB, 0.5), (UCB, -0.5), (MGFI, 2.0)):
        for y_hat, sd_ub in ((NAN, 0.3), (1.0, NAN), (NAN, NAN)):
            v = b(a_id, par, y_hat, sd_ub, 0.0)
            if a_id == UCB and par < 0 and not np.isnan(y_hat):
                assert v == y_hat
                continue
            assert np.isnan(v) or v == INF, (a_id, par, y_hat, sd_ub, v)
            assert np.array_equal(_below(eng, v, [1.0, INF]), [0.0, 0.0])
        for bad in (NAN, INF, -INF):  # the interval bound: nothing to bound, the row is kept
            v = np.r_[_interval(eng, a_id, par, bad, 0.1, 1.0, 0.0, 1.0), _interval(eng, a_id, par, 0.5, abs(bad), 1.0, 0.0, 1.0),
                      _interval(eng, a_id, par, 0.5, 0.1, bad, 0.0, 1.0), _interval(eng, a_id, par, 0.5, -0.1, 1.0, 0.0, 1.0)]  # fmt: skip
            assert np.all(v == INF), (a_id, par, bad, v)
            assert not np.any(_below(eng, v, 1.0))


def test_prune_test_margin_and_thresholds(eng):
    t = lambda bound, thr: bool(_below(eng, bound, thr)[0])  # noqa: E731
    assert t(1.0, 2.0) and t(-5.0, -3.0) and t(0.0, 1e-290)
    assert not t(2.0, 2.0) and not t(2.0 * (1 - 1e-12), 2.0)
    assert t(2.0 * (1 - 1e-8), 2.0)
    assert not t(0.0, 0.0) and not t(0.0, 5e-324) and not t(0.0, 1e-310) and not t(0.0, 1e-300)  # zero / subnormal thresholds
    assert not t(-INF, INF) and not t(0.0, NAN) and not t(0.0, -INF) and not t(NAN, 1.0) and not t(INF, 1.0)
    assert not t(-INF, 0.0)
    assert not t(1e-310, 1e-309) and not t(5e-324, 2.2e-308) and not t(0.0, -0.0)  # subnormal on both sides: the 1e-300 keeps the row


def test_feasibility_exact_cases(eng):
    f = lambda mu, mse, s2, lo, hi: eng.selftest_criteria(_lib.CRITERIA_FEASIBILITY, mu, mse, s2, lo, hi)  # noqa: E731
    assert f(0.3, 0.7, 1.0, -INF, INF)[0] == 1.0
    rng = np.random.default_rng(0)
    mu, mse = rng.normal(size=200), rng.uniform(1e-3, 2.0, size=200)
    assert np.all(f(mu, mse, 1.3, -INF, INF) == 1.0)   # every bound infinite: the base criterion is untouched
    assert np.all(f(mu, mse, 1.3, 0.25, 0.25) == 0.0)  # lo == hi
    assert f(0.1, 0.5, 1.0, 0.25, 0.25)[0] == 0.0
    x = np.array([-1.5, -1.0, 0.0, 1.0, 1.5])
    want = np.array([0.0, 1.0, 1.0, 1.0, 0.0])
    assert np.array_equal(f(x, 0.0, 1.0, -1.0, 1.0), want)
    assert np.array_equal(f(x, 1e-14, 1.0, -1.0, 1.0), want)  # sd / sqrt(sigma2) = 1e-7: under the guard
    assert np.array_equal(f(x, 0.998e-12 * 1e8, 1e8, -1.0, 1.0), want) and not np.array_equal(f(x, 1.002e-12 * 1e8, 1e8, -1.0, 1.0), want)
    assert np.array_equal(f([-2.0, 2.0], 0.0, 1.0, -INF, 0.0), [1.0, 0.0])
    assert np.array_equal(f([2.0, -2.0], 0.0, 1.0, 0.0, INF), [1.0, 0.0])
    # the host half returns the same on all of these
    for m, want_ in zip(x, want):
        assert _lib.feasibility(m, 0.0, 1.0, -1.0, 1.0) == want_


# ----------------------------------------------------------------------------------------------------------------------
# c. domination on the device
# ----------------------------------------------------------------------------------------------------------------------
def _compare_bounds(name, dev, host, allow):
    """device against host bound: the same class where not finite, equal where tiny, else within 2 F allowances -> worst ratio"""
    assert np.array_equal(np.isnan(dev), np.isnan(host)) and np.array_equal(dev == INF, host == INF)
    fin = np.isfinite(host) & (np.abs(host) >= CC.TINY)
    rest = np.isfinite(host) & ~fin
    assert np.all(np.abs(dev[rest]) <= 1e-289)
    same = dev[fin] == host[fin]
    with np.errstate(all="ignore"):
        r = np.where(same, 0.0, np.abs(dev[fin] - host[fin]) / allow[fin])
    assert np.all(np.isfinite(r))
    return float(r.max()) if len(r) else 0.0


@pytest.mark.parametrize("a_id", [EI, PI, UCB, MGFI])
def test_bound_dominates_the_criterion_on_the_whole_range_on_the_device(eng, a_id):
    """tests/test_prune_bounds_host.py's property, PC.domination_cases' rows (tail rows z in [-37, -20] and the rungs 1 and 2 ulp under
    sd_ub included): PRUNE_BELOW(ACQ_UPPER_BOUND(sd_ub), ACQ_VALUE(sd)) is 0 on every rung of [0, sd_ub], every value from the device."""
    lib = _lib.load()
    rows, heads = [], []
    for s2, plugin, y_hat, sd_ub in PC.domination_cases(a_id):
        for par in PC.DOMINATION_PARS[a_id]:
            heads.append((par, y_hat, sd_ub, plugin, s2))
            for sd in PC.sd_grid(sd_ub, s2):
                rows.append((par, y_hat, sd, plugin, s2, len(heads) - 1))
    rows, heads = np.array(rows), np.array(heads)
    k = rows[:, 5].astype(int)
    b_head = _bound(eng, a_id, heads[:, 0], heads[:, 1], heads[:, 2], heads[:, 3], heads[:, 4])
    v = _value(eng, a_id, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4])
    b = b_head[k]
    pruned = _below(eng, b, v)
    nan_v = np.isnan(v)
    assert np.all(np.isnan(b[nan_v]) | (b[nan_v] == INF))  # a NaN value only where the bound is +inf or NaN
    assert not np.any(pruned), rows[np.flatnonzero(pruned)[:3]]
    fin = np.isfinite(b) & ~nan_v
    assert fin.sum() > 0.5 * len(v) and np.count_nonzero(v[fin]) > 0.1 * len(v)  # not vacuous
    slack = v[fin] - (b[fin] + PC.prune_margin(b[fin], v[fin]))
    assert slack.max() <= 0.0  # the same statement in numpy
    # the device's bound against the host's
    host = np.array([lib.bogp_acq_upper_bound(int(a_id), *map(float, (h[0], h[1], h[2], h[3], h[4]))) for h in heads])
    allow = CC.bound_allowance(a_id, heads[:, 0], heads[:, 1], heads[:, 2], heads[:, 3], host)
    worst = _compare_bounds(NAME[a_id], b_head, host, allow)
    print("T20 acq_upper_bound %-4s device against host: worst %.4g allowances (2 F = %d) over %d bounds; %d rungs, %d with the largest sd_ub - sd <= 2 ulp"
          % (NAME[a_id], worst, 2 * CC.F[NAME[a_id]], len(heads), len(v), int(np.sum((heads[k, 2] - rows[:, 2] <= 2 * np.spacing(heads[k, 2])) & (rows[:, 2] < heads[k, 2])))))  # fmt: skip
    assert worst <= 2 * CC.F[NAME[a_id]]


@pytest.mark.parametrize("a_id", [EI, PI, UCB, MGFI])
def test_interval_bound_dominates_the_bound_on_the_whole_interval_on_the_device(eng, a_id):
    """tests/test_bound32_host.py's property, BC.interval_cases' rows: PRUNE_BELOW(ACQ_UPPER_BOUND_INTERVAL(y32, e), ACQ_UPPER_BOUND(y))
    is 0 at the 201 points of [y32 - e, y32 + e] (and at the ends and the centre as the bound forms them), every value from the device;
    the interval bound is +inf wherever the host test says it must be."""
    lib = _lib.load()
    heads, pts, owner = [], [], []
    for minimize in (True, False):
        for s2, plugin, y_hat, e, sd_ub in BC.interval_cases(a_id, minimize):
            ys = BC.interval_points(y_hat, e)
            for par in BC.INTERVAL_PARS[a_id]:
                heads.append((par, y_hat, e, sd_ub, plugin, s2))
                pts.append(ys)
    heads, pts = np.array(heads), np.array(pts)  # (H, 6), (H, 204)
    H, P = pts.shape
    b = _interval(eng, a_id, *heads.T)
    rep = lambda col: np.repeat(heads[:, col], P)  # noqa: E731
    inner = _bound(eng, a_id, rep(0), pts.ravel(), rep(3), rep(4), rep(5)).reshape(H, P)
    pruned = _below(eng, np.repeat(b, P), inner.ravel()).reshape(H, P)
    assert not np.any(np.isnan(b))
    must_inf = np.any(np.isnan(inner) | np.isinf(inner), axis=1)
    lo, hi = heads[:, 1] - heads[:, 2], heads[:, 1] + heads[:, 2]
    if a_id == MGFI:
        must_inf |= (lo <= heads[:, 4]) & (heads[:, 4] <= hi)
    if a_id == PI:
        must_inf |= (lo <= 0.0) & (0.0 <= hi)
    assert np.all(b[must_inf] == INF)
    if a_id in (PI, MGFI):
        assert np.count_nonzero(b == INF) > 0
    assert np.count_nonzero(np.isfinite(b)) > 0.4 * H
    assert not np.any(pruned), heads[np.flatnonzero(pruned.any(axis=1))[:3]]
    with np.errstate(invalid="ignore"):
        strict = np.isfinite(inner) & (inner > b[:, None])
    # the device's interval bound against the host's
    host = np.array([lib.bogp_acq_upper_bound_interval(int(a_id), *map(float, h)) for h in heads])
    with np.errstate(all="ignore"):
        allow = np.maximum(CC.bound_allowance(a_id, heads[:, 0], lo, heads[:, 3], heads[:, 4], host),
                           CC.bound_allowance(a_id, heads[:, 0], hi, heads[:, 3], heads[:, 4], host)) + 2 * CC.EPS * np.abs(host)  # fmt: skip
    worst = _compare_bounds(NAME[a_id], b, host, allow)
    print("T20 acq_upper_bound_interval %-4s device against host: worst %.4g allowances (2 F = %d) over %d intervals, %d finite; points above the bound itself: %d"
          % (NAME[a_id], worst, 2 * CC.F[NAME[a_id]], H, int(np.isfinite(b).sum()), int(strict.sum())))  # fmt: skip
    assert worst <= 2 * CC.F[NAME[a_id]]
    assert not np.any(strict)  # (the host test's form of the statement: no point above the raised bound at all)


# ----------------------------------------------------------------------------------------------------------------------
# d. the instrument measures what the sweeps run
# ----------------------------------------------------------------------------------------------------------------------
def _same_bytes(what, got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    diff = got.view(np.int64) != want.view(np.int64)
    if diff.any():
        with np.errstate(all="ignore"):
            ulps = np.abs(got[diff] - want[diff]) / np.spacing(np.abs(want[diff]))
        print("T20 (d) %s: %d of %d rows differ, by up to %.3g ulp" % (what, int(diff.sum()), diff.size, float(np.nanmax(ulps))))
    assert got.tobytes() == want.tobytes(), what


def _plugin(y, minimize):
    """a plugin inside the data's range -- with the best observed value every improvement criterion of these peaked models underflows to 0"""
    return float(np.quantile(y, 0.3) if minimize else -np.quantile(y, 0.7))


def _gp(eng, N, ordinary=True):
    X, y, par, st = BC.model(PC.KERNEL, ordinary, PC.DIM, n=N)
    eng.set_train(X, y)
    eng.commit(PC.KERNEL, _lib.MODE_NOISY, par, PC.NOISE, ordinary, 0.0)
    return y, float(eng.get_state(with_C=False)["sigma2"])


@pytest.mark.parametrize("N,M,chunk_mb,path", [(96, 20, None, "sweep_small_batch"), (96, 300, None, "sweep_one_launch"), (544, 300, "1", "sweep_chunks")])
def test_acq_value_returns_the_bytes_of_the_single_target_sweeps(eng, monkeypatch, N, M, chunk_mb, path):
    y, s2 = _gp(eng, N)
    eng.upload_candidates(PC.candidates(M=M))
    if chunk_mb:
        monkeypatch.setenv("BOGP_CHUNK_MB", chunk_mb)
    mu, mse = eng.predict()
    for minimize in (True, False):
        plugin = _plugin(y, minimize)
        best, idx, vals = eng.sweep(ACQ4, plugin, minimize, return_values=True)
        if chunk_mb:
            assert eng.last_timing()["n_chunks"] >= 2
        y_hat, sd = (mu if minimize else -1 * mu), np.sqrt(mse)
        for c, (a_id, par) in enumerate(ACQ4):
            _same_bytes("%s, %s, minimize %d" % (path, NAME[a_id], minimize), _value(eng, a_id, par, y_hat, sd, plugin, s2), vals[c])
        live = [int(np.count_nonzero((v != 0.0) & (v != 1.0))) for v in vals]  # rows outside the guards and not saturated, per criterion
        print("T20 (d) %s, minimize %d: the stored values are ACQ_VALUE's bytes; live rows per criterion %s of %d" % (path, minimize, live, M))
        assert np.all(np.isfinite(vals)) and min(live) >= 5 and live[0] >= M // 4


def test_acq_value_returns_the_bytes_of_point_eval_batch(eng):
    y, s2 = _gp(eng, 96)
    Xb = PC.candidates(M=64)
    for minimize in (True, False):
        plugin = _plugin(y, minimize)
        mu, mse, _, _, vals, _ = eng.point_eval_batch(Xb, ACQ4, plugin, minimize, return_dx=False)
        y_hat, sd = (mu if minimize else -1 * mu), np.sqrt(mse)
        for c, (a_id, par) in enumerate(ACQ4):
            _same_bytes("point_eval_batch, %s, minimize %d" % (NAME[a_id], minimize), _value(eng, a_id, par, y_hat, sd, plugin, s2), vals[:, c])


def test_acq_value_and_feasibility_return_the_bytes_of_the_constrained_sweep(eng):
    from test_gpu_ehvi import _model

    X, Y, _, _ = _model(eng, 2, 300, 5, _lib.KERNEL_MATERN52, True, seed=302)
    eng.upload_candidates(np.random.default_rng(1).uniform(-2.5, 2.5, size=(299, 5)))
    s2 = eng.get_state(with_C=False)["sigma2"]
    acq3 = [a for a in ACQ4 if a[0] != UCB]  # (the constrained sweep refuses UCB)
    for minimize in (True, False):
        plugin = float(Y[:, 0].min() if minimize else -Y[:, 0].max())
        _, _, vals, mu, mse = eng.sweep_constrained(acq3, plugin, minimize, [-INF], [INF], return_values=True, return_moments=True)
        y_hat, sd = (mu[:, 0] if minimize else -1 * mu[:, 0]), np.sqrt(mse[:, 0])
        for c, (a_id, par) in enumerate(acq3):
            _same_bytes("sweep_constrained, %s, minimize %d" % (NAME[a_id], minimize), _value(eng, a_id, par, y_hat, sd, plugin, s2[0]), vals[c])
    for lo, hi in ((-INF, float(np.median(Y[:, 1]))), (float(np.quantile(Y[:, 1], 0.25)), float(np.quantile(Y[:, 1], 0.75))), (float(np.median(Y[:, 1])), INF)):
        _, _, vals, pof, mu, mse = eng.sweep_constrained([(_lib.ACQ_NONE, 0.0)], 0.0, True, [lo], [hi], return_values=True, return_pof=True, return_moments=True)
        f = eng.selftest_criteria(_lib.CRITERIA_FEASIBILITY, mu[:, 1], mse[:, 1], s2[1], lo, hi)
        _same_bytes("sweep_constrained, feasibility only, [%g, %g]" % (lo, hi), f, vals[0])
        assert pof.tobytes() == vals[0].tobytes() and np.count_nonzero((f > 0) & (f < 1)) > len(f) // 10


def test_acq_value_returns_the_bytes_of_the_forest_sweep():
    rng = np.random.default_rng(5)
    T, d = 8, 3
    off, feat, thr, left, right, val = [0], [], [], [], [], []
    for t in range(T):  # depth-2 complete trees, 7 nodes each
        th, f = rng.uniform(-3, 3, size=3), rng.integers(0, d, size=3)
        feat += [f[0], f[1], -2, -2, f[2], -2, -2]
        thr += [th[0], th[1], -2, -2, th[2], -2, -2]
        left += [1, 2, -1, -1, 5, -1, -1]
        right += [4, 3, -1, -1, 6, -1, -1]
        val += list(rng.normal(size=7))
        off.append(off[-1] + 7)
    e = _lib.Engine(0)
    try:
        e.forest_set(d, off, feat, thr, left, right, val)
        e.upload_candidates(rng.uniform(-4, 4, size=(300, d)))
        mu, mse = e.forest_predict()
        assert len(np.unique(mse)) > 10
        for minimize in (True, False):
            plugin = float(mu.min() if minimize else -mu.max())
            _, _, vals = e.forest_sweep_topk(ACQ4, plugin, minimize, 1, return_values=True)
            y_hat, sd = (mu if minimize else -1 * mu), np.sqrt(mse)
            for c, (a_id, par) in enumerate(ACQ4):
                _same_bytes("forest sweep, %s, minimize %d" % (NAME[a_id], minimize), _value(e, a_id, par, y_hat, sd, plugin, 1e8), vals[c])
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------------------
# e. error returns
# ----------------------------------------------------------------------------------------------------------------------
def test_error_returns(eng):
    lib = _lib.load()
    rows, out = np.zeros((4, _lib.CRITERIA_COLUMNS)), np.zeros(4)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    assert lib.bogp_selftest_criteria(None, 0, p(rows), 4, p(out)) == _lib.ERR_INVALID
    assert lib.bogp_selftest_criteria(eng._h, 0, None, 4, p(out)) == _lib.ERR_INVALID
    assert lib.bogp_selftest_criteria(eng._h, 0, p(rows), 4, None) == _lib.ERR_INVALID
    assert lib.bogp_selftest_criteria(eng._h, 0, p(rows), 0, p(out)) == _lib.ERR_INVALID
    assert lib.bogp_selftest_criteria(eng._h, 0, p(rows), -3, p(out)) == _lib.ERR_INVALID
    for what in (-1, _lib.CRITERIA_PRUNE_BELOW + 1):
        with pytest.raises(_lib.BogpError, match="unknown selector") as err:
            eng.selftest_criteria(what, np.zeros(4))
        assert err.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.BogpError, match="null pointer or empty"):
        eng.selftest_criteria(_lib.CRITERIA_NDTR, np.zeros(0))
    with pytest.raises(ValueError):
        eng.selftest_criteria(_lib.CRITERIA_NDTR, *[np.zeros(2)] * 9)
    assert eng.selftest_criteria(_lib.CRITERIA_NDTR, 0.0)[0] == 0.5  # the handle still works
