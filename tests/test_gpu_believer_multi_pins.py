"""Pins on the steps the three multi-target believer kernels have in common (the downdate, the clamp, the tail that takes earlier
winners out of the argmax and leaves one record per 256 rows: csrc/bogp_believer_multi.h for the two constrained families,
k_believer_ehvi's own text for EHVI), at N = 24, d = 2, q = 3 with one pending point, against each family's restatement in
tests/support:
  (a) M = 257: the second workgroup has ONE valid row.  The candidates are ordered so that this row wins step 0; it must then be
      the record of its workgroup, and in steps 1 and 2 -- a winner now -- keep its value but leave the argmax to workgroup 0.
  (b) a pending point given twice under modelled constraints: the second is guarded (no update) and, as the last pending point,
      stands in front of step 0, whose pass evaluates the variances exactly as the pass before left them.  (The EHVI and the
      constrained-EHVI families have this case in their own test_pivot_guard.)
  (c) all values equal under EHVI -- a front point far above every posterior makes every cell's improvement underflow to 0 -- on
      257 rows: the winners leave in row order 0, 1, 2, the first maximum among the rows that compete, over both workgroups.  (The
      two constrained families have this case, on 300 rows, in their test_every_row_becomes_a_winner_and_degenerate_bounds.)

Tolerances: the MSE per target under T2 (rtol 1e-6, atol 1e-12 sigma2_k) against the restatement; indices exactly, where the
restatement's winner leads its runner-up by more than 1e-9 of its value; and, bit for bit on the device's own values, every step's
winner is the first maximum among the rows no earlier step took."""
import numpy as np
import pytest

from bogp import _lib
from believer_constrained_cases import ACQ_MIXED
from support.believer_constrained_ehvi_ref import BelieverConstrainedEhviRef
from support.believer_constrained_ref import BelieverConstrainedRef
from support.believer_ehvi_ref import BelieverEhviRef

pytestmark = pytest.mark.gpu
INF = float("inf")
N, D, Q, M = 24, 2, 3, 257
THETA = np.array([3.0, 4.0])


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def commit(eng, m, seed):
    """(X, Y, candidates (M, D), one pending row off the candidates) of a noiseless Matern-5/2 model with m targets of distinct scales"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    eng.set_train(X, Y)
    eng.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, THETA, 0.0, False, 0.1)
    return X, Y, rng.uniform(-2.2, 2.2, size=(M, D)), rng.uniform(-2, 2, size=(1, D))


def families(eng):
    """name -> (targets, seed, key of the values, run(pending, Xs or None) -> (device dict, restatement dict or None))"""

    def ehvi(X, Y):
        front, rp = Y[:8], Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
        dev = lambda p: eng.sweep_believer_ehvi(front, rp, Q, pending=p, return_values=True)  # noqa: E731
        ref = lambda p, Xs: BelieverEhviRef(X, THETA, _lib.KERNEL_MATERN52, eng.get_state()).run(Xs, front, rp, Q, pending=p)  # noqa: E731
        return dev, ref

    def constrained(X, Y):
        lo, hi = np.quantile(Y[:, 1:], 0.2, axis=0), np.full(Y.shape[1] - 1, INF)
        plugin = float(Y[:, 0].min())
        dev = lambda p: eng.sweep_believer_constrained(ACQ_MIXED[:Q], plugin, True, lo, hi, pending=p, believe_plugin=False, return_values=True)  # noqa: E731
        ref = lambda p, Xs: BelieverConstrainedRef(X, THETA, _lib.KERNEL_MATERN52, eng.get_state()).run(  # noqa: E731
            Xs, ACQ_MIXED[:Q], plugin, True, lo, hi, pending=p, believe_plugin=False)
        return dev, ref

    def constrained_ehvi(X, Y):
        lo, hi = np.quantile(Y[:, 2:], 0.2, axis=0), np.full(Y.shape[1] - 2, INF)
        feasible = np.all((lo <= Y[:, 2:]) & (Y[:, 2:] <= hi), axis=1)
        front, rp = Y[feasible, :2], Y[:, :2].min(axis=0) - 0.1 * np.abs(Y[:, :2].min(axis=0))
        dev = lambda p: eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=p, return_values=True)  # noqa: E731
        ref = lambda p, Xs: BelieverConstrainedEhviRef(X, THETA, _lib.KERNEL_MATERN52, eng.get_state()).run(Xs, front, rp, Q, lo, hi, pending=p)  # noqa: E731
        return dev, ref

    return {"ehvi": (2, 11, "ehvi", ehvi), "constrained": (3, 12, "acq", constrained), "constrained_ehvi": (3, 13, "val", constrained_ehvi)}


@pytest.mark.parametrize("family", ["ehvi", "constrained", "constrained_ehvi"])
def test_one_valid_row_in_the_last_workgroup(eng, family):
    """(a)"""
    m, seed, key, make = families(eng)[family]
    X, Y, Xs, pend = commit(eng, m, seed)
    dev, ref = make(X, Y)
    eng.upload_candidates(Xs)
    w = int(dev(pend)["best_idx"][0])
    Xs[[w, M - 1]] = Xs[[M - 1, w]]  # the values are functions of the row alone: step 0's winner now stands in row 256
    eng.upload_candidates(Xs)
    out, r = dev(pend), ref(pend, Xs)
    rel = (r["best_val"] - r["second"]) / np.abs(r["best_val"])
    print(family, "winners", out["best_idx"], "values", out["best_val"], "winner / runner-up gaps", rel)
    assert np.all(rel > 1e-9), rel  # the restatement's winner is no tie: a wrong index cannot hide
    assert out["best_idx"][0] == M - 1
    np.testing.assert_array_equal(out["best_idx"], r["best_idx"])
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])
    sigma2 = np.atleast_1d(eng.get_state(with_C=False)["sigma2"])
    for j in range(Q):
        for t in range(m):
            np.testing.assert_allclose(out["mse"][j][:, t], r["mse"][j][:, t], rtol=1e-6, atol=1e-12 * sigma2[t], err_msg="mse step %d target %d" % (j, t))
        v = out[key][j]
        assert not np.any(np.isneginf(v))  # a winner's row keeps its value in the outputs
        free = np.ones(M, bool)
        free[out["best_idx"][:j]] = False
        assert out["best_idx"][j] == int(np.flatnonzero(free)[np.argmax(v[free])]) and out["best_val"][j] == v[out["best_idx"][j]]
    assert np.all(out["best_idx"][1:] < 256)  # workgroup 1's record is (-inf, no row) from step 1 on: workgroup 0's stands


def test_duplicate_pending_point_in_front_of_step_0_constrained(eng):
    """(b)"""
    m, seed, key, make = families(eng)["constrained"]
    X, Y, Xs, pend = commit(eng, m, seed)
    dev, _ = make(X, Y)
    eng.upload_candidates(Xs)
    base, rep = dev(pend), dev(np.vstack([pend, pend]))
    assert rep["pivots"][1] <= 1e-12
    np.testing.assert_array_equal(np.delete(rep["pivots"], 1), base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "best_mu", "plugins", "acq", "pof", "mse"):
        np.testing.assert_array_equal(rep[k], base[k], err_msg=k)
    assert eng.believer_constrained_last()["n_passes"] == 2 + Q - 1  # the guarded last pending point still runs step 0's pass


def test_equal_values_leave_in_row_order_ehvi(eng):
    """(c)"""
    X, Y, Xs, pend = commit(eng, 2, 11)
    eng.upload_candidates(Xs)
    rp = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    out = eng.sweep_believer_ehvi(np.array([[1e6, 1e6]]), rp, Q, pending=pend, return_values=True)
    assert np.all(out["ehvi"] == 0.0) and np.all(out["best_val"] == 0.0)
    assert out["best_idx"].tolist() == [0, 1, 2]
    np.testing.assert_array_equal(out["best_x"], Xs[:3])
