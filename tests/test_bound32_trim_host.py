"""k_bound32_sums up to d = 32 on the host (no GPU; csrc/kernels_bound32.hip): the exported margin covers the
error of a float32 restatement of the NEW operation sequence (tests/bound32_trim_cases.py) on every row, the rows that restatement
flags include every row the exact test keeps, and the criterion tests/test_gpu_bound32_trim.py sweeps each model with lets the pilot
estimate choose the one-pass path -- so that the stage runs there."""
import numpy as np
import pytest

import bound32_cases as BC
import bound32_trim_cases as TC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

EI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_UCB, _lib.ACQ_MGFI


@pytest.mark.parametrize("d", TC.DIMS_REG)
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("kernel", TC.KERNELS)
def test_margin_holds_on_every_row_of_the_new_sequence(kernel, ordinary, d):
    X, y, par, st = BC.model(kernel, ordinary, d)
    Xs = np.vstack([np.random.default_rng(7).uniform(-5, 5, size=(400, d)), BC.special_rows(X, d)])
    rs = TC.restate(st, Xs)
    e_mu, e_w = BC.margins(kernel, d, rs["na"], rs["nb_max"], rs["gamma_l1"], rs["w_l1"])
    err_mu, err_w = np.abs(rs["mu32"] - rs["mu64"]), np.abs(rs["wd32"] - rs["wd64"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.r_[e_mu / err_mu, (e_w / err_w)[err_w > 0]]
    print("kernel %d ordinary %d d %2d: |gamma|_1 = %.4g, |w|_1 = %.4g; E_mu %.3g .. %.3g (row at 1e3: %.3g), max |mu32 - mu64| = %.3g, "
          "smallest margin / error = %.3g" % (kernel, ordinary, d, rs["gamma_l1"], rs["w_l1"], e_mu[:-1].min(), e_mu[:-1].max(), e_mu[-1],
                                               err_mu.max(), np.nanmin(ratio)))  # fmt: skip
    assert np.all(err_mu <= e_mu) and np.all(err_w <= e_w)
    assert np.all(np.isfinite(e_mu)) and np.all(np.isfinite(rs["mu32"]))
    assert st.estimate_trend or (np.all(rs["wd32"] == 0.0) and np.all(rs["wd64"] == 0.0))  # nothing to sum under simple kriging: w = 0


def test_the_scaled_operands_stay_below_fp32s_maximum_up_to_the_margins_guard():
    """na + nb < 1e37 is what bound32_margin serves: the accumulator starts at kappa^2 (na + nb) and no partial sum of the chain exceeds
    twice that (2 |a_k b_k| <= a_k^2 + b_k^2), with kappa^2 <= 5 log2(e)^2 = 10.41 and rounding room of d + 2 roundings"""
    k2 = max(TC.KAPPA.values()) ** 2
    assert abs(k2 - 5 * TC.LOG2E**2) < 1e-12 and abs(TC.KAPPA[O.KERNEL_SE] ** 2 - TC.LOG2E) < 1e-15
    assert abs(TC.KAPPA[O.KERNEL_MATERN32] ** 2 - 3 * TC.LOG2E**2) < 1e-14
    assert 2 * k2 * 1e37 * (1 + 40 * 2.0**-24) < float(np.finfo(np.float32).max)
    for na in (1e37, np.inf):
        assert BC.margins(O.KERNEL_MATERN52, 20, np.array([na]), 4.0, 1000.0, 10.0)[0][0] == np.inf
    e20 = BC.margins(O.KERNEL_MATERN52, 20, np.array([1.0]), 4.0, 1000.0, 10.0)[0][0]
    e32 = BC.margins(O.KERNEL_MATERN52, 32, np.array([1.0]), 4.0, 1000.0, 10.0)[0][0]
    assert 0 < e20 < e32 < 1.0


@pytest.fixture(scope="module")
def prune_models():
    out = {}
    Xs = PC.candidates()
    for ordinary in (False, True):
        X, y, par, st = PC.model(ordinary)
        out[ordinary] = (st, y, Xs, TC.restate(st, Xs))
    return out


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("acq", [[(UCB, 0.5)], [(UCB, 8.0)], [(UCB, 10.0)], [(UCB, 15.0)], [(MGFI, 2.0), (EI, 0.0)]], ids=lambda a: "-".join("%d_%g" % t for t in a))
def test_restated_flags_are_a_superset_of_the_exact_survivors(prune_models, ordinary, acq):
    st, y, Xs, rs = prune_models[ordinary]
    pl = float(y.min())
    f32, f64 = BC.stage1_flags(st, Xs, acq, pl, True, PC.CHUNK_ROWS, rs)
    behind = slice(PC.CHUNK_ROWS, None)
    n64, n32 = int(np.count_nonzero(f64[behind])), int(np.count_nonzero(f32[behind]))
    assert n64 == int(round(PC.surviving_fraction(st, Xs, acq, pl) * len(Xs)))
    print("ordinary %d %s: exact survivors %d, stage 1 keeps %d of %d rows" % (ordinary, acq, n64, n32, len(Xs) - PC.CHUNK_ROWS))
    assert not np.any(f64[behind] & ~f32[behind])


@pytest.mark.parametrize("d", TC.DIMS_REG + [TC.DIM_ANY])
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("kernel", TC.KERNELS)
def test_the_device_tests_criterion_lets_one_pass_through(kernel, ordinary, d):
    """the pilot rule of tests/test_gpu_bound32.py's fall-back test: 8 x survivors in the pilot <= pilot, and the library's own decision"""
    X, y, par, st = BC.model(kernel, ordinary, d)
    Xs = TC.candidates(d)
    acq = TC.criterion(kernel, ordinary, d)
    keep = TC.exact_flags(st, Xs, acq, float(y.min()))
    n_pilot, n_behind = int(keep[: PC.CHUNK_ROWS].sum()), int(keep[PC.CHUNK_ROWS :].sum())
    assert n_behind == int(round(PC.surviving_fraction(st, Xs, acq, float(y.min())) * len(Xs)))
    print("kernel %d ordinary %d d %2d %s: %d of the pilot's %d rows survive, %d of the %d behind it"
          % (kernel, ordinary, d, acq, n_pilot, PC.CHUNK_ROWS, n_behind, len(Xs) - PC.CHUNK_ROWS))
    assert 8 * n_pilot <= PC.CHUNK_ROWS
    assert _lib.load().bogp_prune_decide(PC.CHUNK_ROWS, n_pilot, 1, 0) != _lib.PRUNE_PATH_CHUNKS
