"""The FP32 bounding stage of the one-pass pruned sweep on the host (no GPU; csrc/kernels_bound32.hip):
the exported margin (bogp_bound32_margin) covers the error of a float32 restatement of the stage on every row, the interval bound
(bogp_acq_upper_bound_interval) dominates bogp_acq_upper_bound over the whole interval, and the rows the restatement flags include
every row the exact test keeps."""
import numpy as np
import pytest

import bound32_cases as BC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
KERNELS = [O.KERNEL_SE, O.KERNEL_MATERN32, O.KERNEL_MATERN52]


@pytest.fixture(scope="module")
def restated():
    """the two models of prune_cases (d = 3, simple / ordinary kriging) and one with d = 5 (a padded k-step), each kernel: state, rows,
    restatement -- computed once"""
    out = {}
    for kernel in KERNELS:
        for name, ordinary, d in (("simple", False, 3), ("ordinary", True, 3), ("d5", True, 5)):
            X, y, par, st = BC.model(kernel, ordinary, d)
            Xs = np.vstack([np.random.default_rng(7).uniform(-5, 5, size=(400, d)), BC.special_rows(X, d)])
            out[kernel, name] = (st, Xs, BC.restate(st, Xs))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["simple", "ordinary", "d5"])
def test_margin_holds_on_every_row(restated, kernel, name):
    st, Xs, rs = restated[kernel, name]
    d = Xs.shape[1]
    e_mu, e_w = BC.margins(kernel, d, rs["na"], rs["nb_max"], rs["gamma_l1"], rs["w_l1"])
    err_mu, err_w = np.abs(rs["mu32"] - rs["mu64"]), np.abs(rs["wd32"] - rs["wd64"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.r_[e_mu / err_mu, (e_w / err_w)[err_w > 0]]
    print("kernel %d %-8s |gamma|_1 = %.4g, |w|_1 = %.4g; E_mu %.3g .. %.3g (row at 1e3: %.3g), max |mu32 - mu64| = %.3g, smallest margin / error = %.3g"
          % (kernel, name, rs["gamma_l1"], rs["w_l1"], e_mu[:-1].min(), e_mu[:-1].max(), e_mu[-1], err_mu.max(), np.nanmin(ratio)))  # fmt: skip
    assert np.all(err_mu <= e_mu) and np.all(err_w <= e_w)
    assert np.all(np.isfinite(e_mu)) and (st.estimate_trend or np.all(rs["wd32"] == 0.0))


def test_margin_is_infinite_where_fp32_cannot_bound():
    for na in (1e37, np.inf, np.nan, -1.0):
        e_mu, e_w = BC.margins(O.KERNEL_MATERN52, 3, np.array([na]), 4.0, 1000.0, 10.0)
        assert e_mu[0] == np.inf and e_w[0] == np.inf
    for kernel in (O.KERNEL_MATERN12, O.KERNEL_ABSEXP, O.KERNEL_CUBIC):  # no bounded slope in the squared distance: not served
        assert BC.margins(kernel, 3, np.array([1.0]), 4.0, 1000.0, 10.0)[0][0] == np.inf
    assert BC.margins(O.KERNEL_SE, 3, np.array([1.0]), 4.0, np.inf, 10.0)[0][0] == np.inf
    e1 = BC.margins(O.KERNEL_SE, 3, np.array([1.0]), 4.0, 1000.0, 10.0)[0][0]
    e2 = BC.margins(O.KERNEL_SE, 20, np.array([1.0]), 4.0, 1000.0, 10.0)[0][0]
    assert 0 < e1 < e2 < 1.0  # grows with the dimension, stays a small fraction of |gamma|_1


@pytest.mark.parametrize("a_id,pars", [(EI, (0.0,)), (PI, (0.0, 0.05, 0.5, 1.5)), (UCB, (0.5, 8.0, 50.0)), (MGFI, (0.5, 2.0, 10.0, 30.0))])
@pytest.mark.parametrize("minimize", [True, False])
def test_interval_bound_dominates_the_bound_on_the_whole_interval(a_id, pars, minimize):
    """Random (y_hat, plugin, sigma2, sd_ub, e), intervals straddling 0 and the plugin and intervals in the tail z in [-37, -20] among them
    (BC.interval_cases, shared with the device's run of the same property in tests/test_gpu_criteria.py): the interval bound is at least
    bogp_acq_upper_bound at 201 points of the interval, both ends included (minimize only decides the sign of y_hat the caller passes:
    both signs are drawn)."""
    assert pars == BC.INTERVAL_PARS[a_id]
    lib = _lib.load()
    n_inf = 0
    for s2, plugin, y_hat, e, sd_ub in BC.interval_cases(a_id, minimize):
        ys = BC.interval_points(y_hat, e)
        for par in pars:
            b = BC.interval_bound(a_id, par, y_hat, e, sd_ub, plugin, s2)
            inner = np.array([lib.bogp_acq_upper_bound(int(a_id), float(par), float(v), sd_ub, plugin, s2) for v in ys])
            if np.any(np.isnan(inner)) or np.any(np.isinf(inner)):
                assert b == np.inf
            n_inf += b == np.inf
            assert not np.isnan(b) and np.all(inner[np.isfinite(inner)] <= b), (a_id, par, y_hat, e, sd_ub, plugin, s2, b, float(np.nanmax(inner)))
            if a_id == MGFI and y_hat - e <= plugin <= y_hat + e:
                assert b == np.inf
            if a_id == PI and y_hat - e <= 0.0 <= y_hat + e:
                assert b == np.inf
    if a_id in (PI, MGFI):
        assert n_inf > 0
    for bad in (np.nan, np.inf, -np.inf):  # nothing to bound: the row is kept
        assert BC.interval_bound(a_id, pars[0], bad, 0.1, 1.0, 0.0, 1.0) == np.inf
        assert BC.interval_bound(a_id, pars[0], 0.5, abs(bad), 1.0, 0.0, 1.0) == np.inf
        assert BC.interval_bound(a_id, pars[0], 0.5, 0.1, bad, 0.0, 1.0) == np.inf
    assert BC.interval_bound(a_id, pars[0], 0.5, -0.1, 1.0, 0.0, 1.0) == np.inf


@pytest.fixture(scope="module")
def prune_models():
    out = {}
    Xs = PC.candidates()
    for ordinary in (False, True):
        X, y, par, st = PC.model(ordinary)
        out[ordinary] = (st, y, Xs, BC.restate(st, Xs))
    return out


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("acq", [[(UCB, 0.5)], [(UCB, 8.0)], [(UCB, 10.0)], [(UCB, 15.0)], [(MGFI, 2.0), (EI, 0.0)]], ids=lambda a: "-".join("%d_%g" % t for t in a))
def test_stage1_flags_are_a_superset_of_the_exact_survivors(prune_models, ordinary, acq):
    st, y, Xs, rs = prune_models[ordinary]
    pl = float(y.min())
    f32, f64 = BC.stage1_flags(st, Xs, acq, pl, True, PC.CHUNK_ROWS, rs)
    behind = slice(PC.CHUNK_ROWS, None)
    n64 = int(np.count_nonzero(f64[behind]))
    assert n64 == int(round(PC.surviving_fraction(st, Xs, acq, pl) * len(Xs)))
    n32 = int(np.count_nonzero(f32[behind]))
    print("ordinary %d %s: exact survivors %d, stage 1 keeps %d of %d rows" % (ordinary, acq, n64, n32, len(Xs) - PC.CHUNK_ROWS))
    assert not np.any(f64[behind] & ~f32[behind])
    if acq in ([(UCB, 0.5)], [(UCB, 8.0)]):  # (what tests/test_gpu_bound32.py expects of the route: the exact stage runs on S1 alone)
        assert 4 * n32 <= len(Xs) - PC.CHUNK_ROWS
