"""Kriging-believer batches on the device (`bogp_sweep_believer`, kernels_believer.hip): the golden G43 recorded from the
reference's own models rebuilt on X + the believed points; the dense NumPy restatement of the recursion
(tests/support/believer_ref.py) over sizes, kernels, modes, trends, criteria, pending points and the plugin rule; step 0
against the plain sweep bit for bit; chunk invariance; the pivot guard; candidate sources; no leakage into later plain
sweeps; the ABI's error returns.

Tolerances: MSE under T2 (rtol 1e-6, atol 1e-12 sigma2), mu under T1, criteria at rtol 1e-6 with T3 (EpsilonPI / MGFI not
compared on rows whose restated MSE <= 1e-12 sigma2 -- here exactly the rows believed so far, asserted); EI and UCB on every row.
The models are well conditioned on purpose (cond(R) ~ 1e2 .. 2e3): the recursion is compared, not the factorisation."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import gp_oracle as O

from bogp import _lib
from support.believer_ref import BelieverRef

pytestmark = pytest.mark.gpu

M, D = 1500, 3
ACQ = [(O.ACQ_EI, 0.0), (O.ACQ_UCB, 2.0), (O.ACQ_MGFI, 2.0), (O.ACQ_EPSILON_PI, 0.05)]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def problem(N, kernel, noisy, est):
    """(X, y, commit arguments, candidates, two pending rows off the candidates): N = 70 pads to 96 rows and takes the fused
    small sweep at step 0, N = 530 the chunked path.  Short length scales keep R well conditioned (see the module docstring)."""
    rng = np.random.default_rng(100 + N)
    X = rng.uniform(-2, 2, size=(N, D))
    y = 4 * (np.sin(X @ np.array([0.9, -0.6, 0.4])) + 0.25 * np.sum(X**2, axis=1) + 0.1 * rng.normal(size=N))
    theta = np.array([1.0, 0.8, 1.3]) * (4.0 if N < 100 else 8.0)
    if noisy:
        args = (kernel, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, est, 0.5)
    else:
        args = (kernel, _lib.MODE_NOISELESS, theta, 0.0, est, 0.5)
    Xs = rng.uniform(-2.2, 2.2, size=(M, D))
    pend = rng.uniform(-2, 2, size=(2, D))
    return X, y, args, Xs, pend


def commit(eng, N, kernel, noisy, est):
    X, y, args, Xs, pend = problem(N, kernel, noisy, est)
    eng.set_train(X, y)
    eng.commit(*args)
    return X, y, args, Xs, pend


def restatement(eng, X, args):
    n_theta = D + (1 if args[0] in (_lib.KERNEL_GENEXP, _lib.KERNEL_MATERN_NU) else 0)
    return BelieverRef(X, args[2][:n_theta], args[0], eng.get_state(), args[4])


def check_against(out, ref, sigma2, n_pend, noiseless):
    """device outputs `out` against the restatement's `ref` (both dicts); returns nothing, asserts everything"""
    q = len(ACQ)
    rel = (ref["best_val"] - ref["second"]) / np.abs(ref["best_val"])
    assert np.all(rel > 1e-9), rel  # the restatement's winner is no tie: a wrong index cannot hide
    np.testing.assert_allclose(out["pivots"], ref["pivots"], rtol=1e-6, atol=1e-12)
    for j, (a, par) in enumerate(ACQ):
        np.testing.assert_allclose(out["mse"][j], ref["mse"][j], rtol=1e-6, atol=1e-12 * sigma2, err_msg="mse step %d" % j)
        noise = ref["mse"][j] <= 1e-12 * sigma2
        assert set(np.flatnonzero(noise).tolist()) == set(ref["best_idx"][:j].tolist()), (j, np.flatnonzero(noise))  # T3's rows: the believed ones only
        ok = ~noise if a in (O.ACQ_EPSILON_PI, O.ACQ_MGFI) else np.ones(M, bool)
        np.testing.assert_allclose(out["acq"][j][ok], ref["acq"][j][ok], rtol=1e-6, atol=1e-300, equal_nan=True, err_msg="criterion step %d" % j)
        assert out["best_idx"][j] == ref["best_idx"][j], j
        free = np.ones(M, bool)
        free[out["best_idx"][:j]] = False  # the winners before keep their value but do not compete
        assert out["best_idx"][j] == int(np.flatnonzero(free)[np.argmax(out["acq"][j][free])]) and out["best_val"][j] == out["acq"][j][out["best_idx"][j]]
        if noiseless:  # every candidate row believed so far is determined
            assert np.all(out["mse"][j][out["best_idx"][:j]] <= 1e-12 * sigma2)
    assert len(set(out["best_idx"].tolist())) == q
    assert len(out["pivots"]) == n_pend + q
    assert np.all(np.abs(ref["s_own"]) <= 1e-12), ref["s_own"]  # the recursion itself determines a believed row, before any override


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference's rebuilt models
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["m32ok", "sesk"])
def test_g43_reference_golden(eng, state):
    """G43 (tests/support/make_believer_golden.py): for each prefix of four believed rows -- two pending points off the
    candidates, then two candidate rows -- the device's MSE_j / sigma2 against the reference's own predict of a reference
    model REBUILT on X + {p_1 .. p_j} with y = mu(p) at the same theta, divided by THAT model's sigma2 (T2); the mean, which
    must not move, against the rebuilt model's (T1)."""
    g = {k[len(state) + 1 :]: v for k, v in load_golden("G43_believer").items() if k.startswith(state + "_")}
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], 0.0, bool(g["estimate_trend"]), float(g["beta"]))
    sigma2 = eng.get_state(with_C=False)["sigma2"]
    np.testing.assert_allclose(sigma2, g["sigma2"][0], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    mu, mse0 = eng.predict()
    np.testing.assert_allclose(mse0, g["mse"], rtol=1e-6, atol=1e-12 * sigma2)
    for j in range(1, 5):
        out = eng.sweep_believer([(O.ACQ_EI, 0.0)], float(g["y"].min()), True, pending=g["believed"][:j], return_values=True)
        print("G43 %s prefix %d: max |d(MSE/sigma2)| = %.3g, pivots %s" % (state, j, np.abs(out["mse"][0] / sigma2 - g["mse_j"][j - 1] / g["sigma2_j"][j - 1]).max(), out["pivots"][:j]))
        np.testing.assert_allclose(out["mse"][0] / sigma2, g["mse_j"][j - 1] / g["sigma2_j"][j - 1], rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(mu, g["mu_j"][j - 1], rtol=1e-6, atol=1e-9)
        assert np.all(out["pivots"][:j] > 1e-3)
    assert np.all(out["mse"][0][g["believed_rows"]] <= 1e-12 * sigma2)  # the believed candidate rows are determined


# ----------------------------------------------------------------------------------------------------------------------
# 2. the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("believe_plugin", [True, False], ids=["plugin", "fixedplugin"])
@pytest.mark.parametrize("est", [False, True], ids=["sk", "ok"])
@pytest.mark.parametrize("noisy", [False, True], ids=["noiseless", "noisy"])
@pytest.mark.parametrize("kernel", [_lib.KERNEL_MATERN52, _lib.KERNEL_SE], ids=["m52", "se"])
@pytest.mark.parametrize("n_pend", [0, 2])
@pytest.mark.parametrize("N", [70, 530])
def test_restatement_parity(eng, N, n_pend, kernel, noisy, est, believe_plugin):
    X, y, args, Xs, pend = commit(eng, N, kernel, noisy, est)
    eng.upload_candidates(Xs)
    plugin = float(y.min())
    out = eng.sweep_believer(ACQ, plugin, True, pending=pend[:n_pend], believe_plugin=believe_plugin, return_values=True)
    r = restatement(eng, X, args)
    ref = r.run(Xs, ACQ, plugin, True, pending=pend[:n_pend], believe_plugin=believe_plugin)
    check_against(out, ref, r.sigma2, n_pend, not noisy)
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])


@pytest.mark.parametrize("believe_plugin", [True, False], ids=["plugin", "fixedplugin"])
@pytest.mark.parametrize("crit", [(O.ACQ_EPSILON_PI, 0.05), (O.ACQ_MGFI, 2.0), (O.ACQ_UCB, 2.0), (O.ACQ_EI, 0.0)], ids=["epsilonpi", "mgfi", "ucb", "ei"])
def test_one_criterion_q_times_gives_distinct_winners(eng, crit, believe_plugin):
    """One criterion replicated q = 4 times, each of the four: the winners are four distinct rows and the restatement's.  On a
    believed row the variance is zero, where EpsilonPI is Phi(+-inf) -- exactly 1 once the row's mean has become the plugin --
    and UCB is the bare mean: such a row keeps that value in the outputs but does not compete again."""
    X, y, args, Xs, pend = commit(eng, 530, _lib.KERNEL_MATERN52, False, True)
    eng.upload_candidates(Xs)
    acq = [crit] * 4
    out = eng.sweep_believer(acq, float(y.min()), True, believe_plugin=believe_plugin, return_values=True)
    ref = restatement(eng, X, args).run(Xs, acq, float(y.min()), True, believe_plugin=believe_plugin)
    assert len(set(out["best_idx"].tolist())) == 4
    assert np.all((ref["best_val"] - ref["second"]) / np.abs(ref["best_val"]) > 1e-9)
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])
    np.testing.assert_allclose(out["best_val"], ref["best_val"], rtol=1e-6)
    for j in range(1, 4):  # the believed rows: determined, and still reported with their own criterion value
        assert np.all(out["mse"][j][out["best_idx"][:j]] == 0.0)
        if crit[0] == O.ACQ_UCB:
            np.testing.assert_allclose(out["acq"][j][out["best_idx"][:j]], ref["mu"][out["best_idx"][:j]], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kernel,extra", [(_lib.KERNEL_GENEXP, 1.5), (_lib.KERNEL_MATERN_NU, 1.7), (_lib.KERNEL_ABSEXP, None)], ids=["genexp", "matern_nu", "absexp"])
def test_other_correlations(eng, kernel, extra):
    """The correlations that carry an extra theta entry (the exponent of generalized_exponential, the order of the general
    Matern kernel) and one that is no function of the squared distance, through pass 0, the solve and k_believer."""
    N = 530
    X, y, args, Xs, pend = problem(N, kernel, False, True)
    theta = args[2] if extra is None else np.r_[args[2], extra]
    args = (kernel, _lib.MODE_NOISELESS, theta, 0.0, True, 0.5)
    eng.set_train(X, y)
    eng.commit(*args)
    eng.upload_candidates(Xs)
    acq = ACQ[:3]
    out = eng.sweep_believer(acq, float(y.min()), True, pending=pend[:1], return_values=True)
    r = restatement(eng, X, args)
    ref = r.run(Xs, acq, float(y.min()), True, pending=pend[:1])
    assert np.all((ref["best_val"] - ref["second"]) / np.abs(ref["best_val"]) > 1e-9)
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])
    np.testing.assert_allclose(out["pivots"], ref["pivots"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(out["mse"], ref["mse"], rtol=1e-6, atol=1e-12 * r.sigma2)


def test_maximising_and_a_single_repeated_criterion(eng):
    """minimize = 0 (y_hat = -mu, the plugin arrives negated and follows the LARGEST believed mean) and one criterion given q
    times: the believer alone keeps the winners apart."""
    X, y, args, Xs, pend = commit(eng, 530, _lib.KERNEL_MATERN52, False, True)
    eng.upload_candidates(Xs)
    acq = [(O.ACQ_EI, 0.0)] * 4
    out = eng.sweep_believer(acq, -float(y.max()), False, pending=pend[:1], return_values=True)
    ref = restatement(eng, X, args).run(Xs, acq, -float(y.max()), False, pending=pend[:1])
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])
    assert np.all((ref["best_val"] - ref["second"]) / np.abs(ref["best_val"]) > 1e-9)
    np.testing.assert_allclose(out["acq"], ref["acq"], rtol=1e-6, atol=1e-300)
    assert len(set(out["best_idx"].tolist())) == 4 and np.all(np.diff(out["best_val"]) < 0)


# ----------------------------------------------------------------------------------------------------------------------
# 3. step 0 is the plain sweep; 8. nothing leaks into a later plain sweep
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_step0_is_the_plain_sweep_and_nothing_leaks(eng, N):
    X, y, args, Xs, pend = commit(eng, N, _lib.KERNEL_MATERN52, False, True)
    eng.upload_candidates(Xs)
    plugin = float(y.min())
    before = eng.sweep(ACQ, plugin, True, return_values=True)
    mu_b, mse_b = eng.predict()
    out = eng.sweep_believer(ACQ[2:] + ACQ[:2], plugin, True, return_values=True)  # criterion 0 = MGFI
    one = eng.sweep(ACQ[2:3], plugin, True, return_values=True)
    assert out["best_val"][0] == one[0][0] and out["best_idx"][0] == one[1][0]
    np.testing.assert_array_equal(out["acq"][0], one[2][0])
    np.testing.assert_array_equal(out["mse"][0], mse_b)
    eng.sweep_believer(ACQ, plugin, True, pending=pend)
    after = eng.sweep(ACQ, plugin, True, return_values=True)
    mu_a, mse_a = eng.predict()
    for b, a in zip(before + (mu_b, mse_b), after + (mu_a, mse_a)):
        np.testing.assert_array_equal(b, a)


# ----------------------------------------------------------------------------------------------------------------------
# 4. chunk invariance
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
def test_chunk_invariance(eng, n_pend):
    """BOGP_CHUNK_MB=1 at N = 530 (544 padded rows: 192 candidates a chunk, 8 chunks of 1500): every output bit for bit the
    one-chunk run's."""
    X, y, args, Xs, pend = commit(eng, 530, _lib.KERNEL_SE, True, True)
    eng.upload_candidates(Xs)
    plugin = float(y.min())
    whole = eng.sweep_believer(ACQ, plugin, True, pending=pend[:n_pend], return_values=True)
    old = os.environ.get("BOGP_CHUNK_MB")
    os.environ["BOGP_CHUNK_MB"] = "1"
    try:
        parts = eng.sweep_believer(ACQ, plugin, True, pending=pend[:n_pend], return_values=True)
        assert eng.last_timing()["n_chunks"] >= 4
    finally:
        if old is None:
            del os.environ["BOGP_CHUNK_MB"]
        else:
            os.environ["BOGP_CHUNK_MB"] = old
    for k in whole:
        np.testing.assert_array_equal(whole[k], parts[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the pivot guard
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_pivot_guard(eng, N):
    """A pending point equal to a training point of a noiseless model, and a pending point given twice, are already determined:
    pivot <= 1e-12, c = 0, and every output is the one of the run without them (the plugin kept as given for the training
    point, whose mean would otherwise join it)."""
    X, y, args, Xs, pend = commit(eng, N, _lib.KERNEL_MATERN52, False, True)
    eng.upload_candidates(Xs)
    plugin = float(y.min())
    base = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], believe_plugin=False, return_values=True)
    trn = eng.sweep_believer(ACQ, plugin, True, pending=np.vstack([X[3], pend[:1]]), believe_plugin=False, return_values=True)
    assert trn["pivots"][0] <= 1e-12
    np.testing.assert_array_equal(trn["pivots"][1:], base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "acq", "mse"):
        np.testing.assert_array_equal(trn[k], base[k], err_msg=k)
    base = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], return_values=True)
    rep = eng.sweep_believer(ACQ, plugin, True, pending=np.vstack([pend[:1], pend[:1]]), return_values=True)
    assert rep["pivots"][1] <= 1e-12
    np.testing.assert_array_equal(np.delete(rep["pivots"], 1), base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "acq", "mse"):
        np.testing.assert_array_equal(rep[k], base[k], err_msg=k)
    # the last pending point guarded: step 0 is then evaluated by a criterion-only pass
    last = eng.sweep_believer(ACQ, plugin, True, pending=np.vstack([pend[:1], X[5]]), believe_plugin=False, return_values=True)
    base = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], believe_plugin=False, return_values=True)
    assert last["pivots"][1] <= 1e-12
    for k in ("best_val", "best_idx", "acq", "mse"):
        np.testing.assert_array_equal(last[k], base[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 7. candidate sources
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_candidate_sources(eng, N):
    X, y, args, _, pend = commit(eng, N, _lib.KERNEL_MATERN52, True, False)
    plugin = float(y.min())
    eng.generate_candidates(np.full(D, -2.2), np.full(D, 2.2), M, seed=17)
    gen = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], return_values=True)
    Xs = eng.read_candidates(np.arange(M))
    eng.upload_candidates(Xs)
    up = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy = eng.sweep_believer(ACQ, plugin, True, pending=pend[:1], return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy0 = eng.sweep_believer(ACQ, plugin, True, return_values=True)
    eng.upload_candidates(Xs)
    up0 = eng.sweep_believer(ACQ, plugin, True, return_values=True)
    for k in up:
        np.testing.assert_array_equal(gen[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy0[k], up0[k], err_msg=k)
    np.testing.assert_array_equal(up["best_x"], Xs[up["best_idx"]])
    # fewer candidates than one workgroup serves, and the small-batch posterior of pass 0 (M <= 32)
    eng.upload_candidates(Xs[:20])
    few = eng.sweep_believer(ACQ[:3], plugin, True, pending=pend[:1], return_values=True)
    r = restatement(eng, X, args)
    ref = r.run(Xs[:20], ACQ[:3], plugin, True, pending=pend[:1])
    np.testing.assert_array_equal(few["best_idx"], ref["best_idx"])
    np.testing.assert_allclose(few["mse"], ref["mse"], rtol=1e-6, atol=1e-12 * r.sigma2)


# ----------------------------------------------------------------------------------------------------------------------
# 9. error returns
# ----------------------------------------------------------------------------------------------------------------------
def _call(eng, q=2, ids=(0, 0), pars=(0.0, 0.0), pending=None, n_pend=0, best=True, idx=True):
    lib = _lib.load()
    ids_ = np.ascontiguousarray(ids if ids is not None else [0], dtype=np.int32)
    pars_ = np.ascontiguousarray(pars, dtype=np.float64)
    bv, bi = np.empty(max(q, 1)), np.empty(max(q, 1), dtype=np.int64)
    pend = None if pending is None else np.ascontiguousarray(pending, dtype=np.float64)
    rc = lib.bogp_sweep_believer(eng._h, q, ids_.ctypes.data_as(C.POINTER(C.c_int)) if ids is not None else None, _lib._ptr(pars_), 0.0, 1, 1,
                                 _lib._ptr(pend), n_pend, _lib._ptr(bv) if best else None, bi.ctypes.data_as(C.POINTER(C.c_int64)) if idx else None,
                                 None, None, None, None)  # fmt: skip
    return rc, lib.bogp_last_error(eng._h).decode()


def test_error_returns():
    """Every error return of bogp_sweep_believer but one: a communicator of more than one rank cannot be built on one device
    (its refusal is a comparison of the handle's world size, exercised by the Python layer's own refusal on the host)."""
    lib = _lib.load()
    assert lib.bogp_sweep_believer(None, 1, None, None, 0.0, 1, 1, None, 0, None, None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, y, args, Xs, pend = problem(70, _lib.KERNEL_SE, False, True)
        e.set_train(X, y)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no committed model" in msg
        e.commit(*args)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no candidates" in msg
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK
        assert _call(e, q=0)[0] == _lib.ERR_INVALID
        e.upload_candidates(Xs[:1])  # more proposals than candidates: every step takes a row no step before it took
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "proposals from 1 candidates" in msg
        e.upload_candidates(Xs)
        rc, msg = _call(e, q=31, ids=[0] * 31, pars=[0.0] * 31, pending=pend, n_pend=2)
        assert rc == _lib.ERR_INVALID and "<= 32" in msg
        assert _call(e, ids=None)[0] == _lib.ERR_INVALID
        assert _call(e, best=False)[0] == _lib.ERR_INVALID and _call(e, idx=False)[0] == _lib.ERR_INVALID
        assert _call(e, pending=None, n_pend=1)[0] == _lib.ERR_INVALID
        assert _call(e, n_pend=-1)[0] == _lib.ERR_INVALID
        bad = pend.copy()
        bad[1, 2] = np.nan
        rc, msg = _call(e, pending=bad, n_pend=2)
        assert rc == _lib.ERR_INVALID and "not finite" in msg
        assert _call(e, ids=(0, 7))[0] == _lib.ERR_INVALID and _call(e, ids=(0, 2), pars=(0.0, 0.0))[0] == _lib.ERR_INVALID
        with pytest.raises(_lib.BogpError) as ei:
            e.sweep_believer([(O.ACQ_EI, 0.0)] * 33, 0.0)
        assert ei.value.code == _lib.ERR_INVALID
        # a lift on the handle
        e.set_lift(np.eye(D), np.zeros(D), None, -np.ones(D), np.ones(D))
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "lift" in msg
        e.clear_lift()
        assert _call(e)[0] == _lib.OK
        # a polynomial trend basis
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "constant trend" in msg
        # several targets
        e.set_train(X, np.column_stack([y, 2 * y + 1]))
        e.commit(args[0], args[1], args[2], 0.0, False, 0.0)
        e.upload_candidates(Xs)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "one target" in msg
    finally:
        e.close()
