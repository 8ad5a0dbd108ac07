"""Kriging-believer batches under modelled constraints on the device (`bogp_sweep_believer_constrained`,
kernels_believer_constrained.hip): the reference's rebuilt models of golden G44 with their columns 1 .. read as constraints; every shared
case (tests/believer_constrained_cases.py, whose conditions tests/test_believer_constrained_host.py asserts without a GPU) against the
dense restatement (tests/support/believer_constrained_ref.py); step 0 against `sweep_constrained` bit for bit and no leakage into later
sweeps; chunk invariance in fresh processes; the edges of the pivot guard, of q = M and of lo == hi; candidate sources; the ABI's error
returns; the timing spans.

Tolerances: pivots rtol 1e-6, atol 1e-12; means under T1 (rtol 1e-6, atol 1e-9); MSE per target under T2 (rtol 1e-6, atol 1e-12
sigma2_k); values and PoF under T24 -- T19's form, |d| <= 1e-6 |ref| + 1e-12 max |ref| on every row, against the restatement evaluated on
the device's own moments (on the reference's for G44).  The models are well conditioned on purpose: the recursion is compared."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden

from bogp import _lib
from believer_constrained_cases import ACQ_FEASIBILITY, ACQ_MIXED, CASES, IDS, Q, D, M, plugin_of, problem, quantile_bounds
from support import constrained_ref as R
from support.believer_constrained_ref import BelieverConstrainedRef

pytestmark = pytest.mark.gpu
INF = float("inf")
KEYS = ("best_val", "best_idx", "best_x", "best_mu", "pivots", "plugins", "acq", "pof", "mse")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def t24(v, ref, what=""):
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    # NaN propagates (include/bogp.h): PI on a believed row -- sd = 0 -- whose mean IS the believed plugin is 0 / 0 in the restatement and
    # on the device alike; such a row is a winner already and does not compete.  The NaNs must stand on the same rows.
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(v), nan), (what, np.flatnonzero(np.isnan(v) != nan))
    v, ref = v[~nan], ref[~nan]
    err = np.abs(v - ref)
    print("T24 %s: max |v - ref| = %.3g, max |ref| = %.3g, NaN rows %d" % (what, err.max(), np.abs(ref).max(), nan.sum()))
    assert np.all(err <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()), (what, err.max())


def commit(eng, N, m, kernel, noisy, seed=0, rows=M):
    p = problem(N, m, kernel, noisy, seed, rows)
    eng.set_train(p[0], p[1])
    eng.commit(*p[2])
    return p


def restatement(eng, X, args):
    return BelieverConstrainedRef(X, args[2][:D], args[0], eng.get_state())


def check_against(eng, out, ref, r, acq, minimize, lo, hi, n_pend, Xs):
    """the device's outputs `out` against the restatement's `ref`"""
    q = len(acq)
    rel = (ref["best_val"] - ref["second"]) / np.abs(ref["best_val"])
    print("winner / runner-up gaps", rel, "plugins", out["plugins"], "pivots", out["pivots"])
    np.testing.assert_allclose(out["pivots"], ref["pivots"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(out["best_mu"], ref["best_mu"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(out["plugins"], ref["plugins"], rtol=1e-6, atol=1e-9)
    mu = eng.sweep_constrained(acq[:1], 0.0, minimize, lo, hi, return_moments=True)[2]  # the device's own means (no step moves them)
    np.testing.assert_allclose(mu, ref["mu"], rtol=1e-6, atol=1e-9)
    for j in range(q):
        for t in range(r.m):
            np.testing.assert_allclose(out["mse"][j][:, t], ref["mse"][j][:, t], rtol=1e-6, atol=1e-12 * r.sigma2[t], err_msg="mse step %d target %d" % (j, t))
        vals, pof = R.constrained(mu, out["mse"][j], r.sigma2, lo, hi, [acq[j]], out["plugins"][j], minimize)
        t24(out["acq"][j], vals[0], "values step %d" % j)
        t24(out["pof"][j], pof, "PoF step %d" % j)
        assert out["best_idx"][j] == ref["best_idx"][j], j
        free = np.ones(len(Xs), bool)
        free[out["best_idx"][:j]] = False  # the winners before keep their value but do not compete
        assert out["best_idx"][j] == int(np.flatnonzero(free)[np.argmax(out["acq"][j][free])]) and out["best_val"][j] == out["acq"][j][out["best_idx"][j]]
    assert len(set(out["best_idx"].tolist())) == q
    assert len(out["pivots"]) == n_pend + q
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference's rebuilt models
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["m2", "m3"])
def test_g44_reference_golden(eng, state):
    """G44's two states (tests/support/make_believer_ehvi_golden.py): for each prefix of four believed rows -- two pending points off the
    candidates, then two candidate rows -- a reference model REBUILT on X + {p_1 .. p_j} with y = mu(p) at the same theta.  Columns 1 ..
    are read as constraints under the quantile bounds.  With q = 1 and pending = believed[:j]: the device's MSE / sigma2 against the
    rebuilt model's mse_j / sigma2_j (rtol 1e-6, atol 1e-12), the means, which must not move, under T1, and EI, PI, MGFI and the
    probability of feasibility against the restatement on the reference's moments -- its bracket mse_j / sigma2_j in units of the
    committed sigma2, which the believer keeps fixed while the rebuilt model's concentrated sigma2_j shrinks by N / (N + j) -- under T24."""
    g = {k[len(state) + 1 :]: v for k, v in load_golden("G44_believer_ehvi").items() if k.startswith(state + "_")}
    m = g["y"].shape[1]
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], 0.0, False, float(g["beta"]))
    sigma2 = eng.get_state(with_C=False)["sigma2"]
    np.testing.assert_allclose(sigma2, g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    lo, hi = quantile_bounds(g["y"])
    plugin = plugin_of(g["y"], lo, hi, True)
    mu = eng.sweep_constrained(ACQ_MIXED[:1], plugin, True, lo, hi, return_moments=True)[2]
    for j in range(1, 5):
        mse_ref = g["mse_j"][j - 1] / g["sigma2_j"][j - 1] * sigma2
        for one in ACQ_MIXED[:3] + ACQ_FEASIBILITY[:1]:
            out = eng.sweep_believer_constrained([one], plugin, True, lo, hi, pending=g["believed"][:j], believe_plugin=False, return_values=True)
            vals, pof = R.constrained(g["mu_j"][j - 1], mse_ref, sigma2, lo, hi, [one], plugin, True)
            t24(out["acq"][0], vals[0], "G44 %s prefix %d criterion %d values" % (state, j, one[0]))
            t24(out["pof"][0], pof, "G44 %s prefix %d PoF" % (state, j))
            assert out["plugins"][0] == plugin
        print("G44 %s prefix %d: max |d(MSE/sigma2)| = %.3g" % (state, j, np.abs(out["mse"][0] / sigma2 - g["mse_j"][j - 1] / g["sigma2_j"][j - 1]).max()))
        for t in range(m):
            np.testing.assert_allclose(out["mse"][0][:, t] / sigma2[t], g["mse_j"][j - 1][:, t] / g["sigma2_j"][j - 1][t], rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(mu[:, t], g["mu_j"][j - 1][:, t], rtol=1e-6, atol=1e-9)
        assert np.all(out["pivots"][:j] > 1e-3)
    assert np.all(out["mse"][0][g["believed_rows"]] <= 1e-12 * sigma2)  # the believed candidate rows are determined


# ----------------------------------------------------------------------------------------------------------------------
# 2. the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_parity(eng, case):
    X, Y, args, Xs, pend, lo, hi, plugin = case.build()
    eng.set_train(X, Y)
    eng.commit(*args)
    eng.upload_candidates(Xs)
    out = eng.sweep_believer_constrained(case.acq, plugin, case.minimize, lo, hi, pending=pend, return_values=True)
    r = restatement(eng, X, args)
    assert len(set(np.round(r.sigma2, 12))) == case.m  # distinct sigma2_k
    ref = r.run(Xs, case.acq, plugin, case.minimize, lo, hi, pending=pend)
    check_against(eng, out, ref, r, case.acq, case.minimize, lo, hi, case.n_pend, Xs)
    if not case.noisy:  # every candidate row believed so far is determined
        for j in range(1, len(case.acq)):
            assert np.all(out["mse"][j][out["best_idx"][:j]] == 0.0)
    if case.acq is ACQ_FEASIBILITY:
        for j in range(len(case.acq)):
            np.testing.assert_array_equal(out["acq"][j], out["pof"][j])  # a feasibility-only step stays feasibility-only


# ----------------------------------------------------------------------------------------------------------------------
# 3. bit identities
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_step0_is_sweep_constrained_and_nothing_leaks(eng, N):
    X, Y, args, Xs, pend = commit(eng, N, 3, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    for acq in (ACQ_MIXED, ACQ_FEASIBILITY):
        before = eng.sweep_constrained(acq[:1], plugin, True, lo, hi, return_values=True, return_pof=True, return_moments=True)
        out = eng.sweep_believer_constrained(acq, plugin, True, lo, hi, return_values=True)
        assert out["best_val"][0] == before[0][0, 0] and out["best_idx"][0] == before[1][0, 0] and out["plugins"][0] == plugin
        assert out["acq"][0].tobytes() == before[2][0].tobytes() and out["pof"][0].tobytes() == before[3].tobytes()
        assert out["mse"][0].tobytes() == before[5].tobytes()
        np.testing.assert_array_equal(out["best_mu"][0], before[4][out["best_idx"][0]])
    topk = eng.sweep_constrained(ACQ_MIXED, plugin, True, lo, hi, k=3, return_values=True, return_pof=True, return_moments=True)
    eng.sweep_believer_constrained(ACQ_MIXED, plugin, True, lo, hi, pending=pend)
    after = eng.sweep_constrained(ACQ_MIXED, plugin, True, lo, hi, k=3, return_values=True, return_pof=True, return_moments=True)
    for b, a in zip(topk, after):
        assert b.tobytes() == a.tobytes()
    # a single-target model on the same handle: its plain sweep and its believer, before and after a constrained batch of another model
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 2.0)]

    def single():
        eng.set_train(X, Y[:, 0])
        eng.commit(args[0], args[1], args[2], args[3], True, 0.0)
        eng.upload_candidates(Xs)
        p1 = float(Y[:, 0].min())
        return eng.sweep(acq, p1, True, return_values=True), eng.sweep_believer(acq, p1, True, pending=pend[:1], return_values=True)

    s_before, b_before = single()
    eng.set_train(X, Y)
    eng.commit(*args)
    eng.upload_candidates(Xs)
    eng.sweep_believer_constrained(ACQ_MIXED, plugin, True, lo, hi, pending=pend)
    s_after, b_after = single()
    for b, a in zip(s_before, s_after):
        np.testing.assert_array_equal(b, a)
    for k in b_before:
        np.testing.assert_array_equal(b_before[k], b_after[k], err_msg=k)


def test_families_share_one_handle():
    """`sweep_believer_ehvi`, `sweep_believer_constrained` and `sweep_believer_ehvi` again on ONE engine: the two families lay out the
    handle's shared believer arrays (running variances, row buffers, columns, the solve's scratch, the cells) differently, and every
    array of every call must equal the same call's on a freshly created engine -- nothing is sized or offset from the call before."""
    X, Y, args, Xs, pend = problem(70, 2, _lib.KERNEL_MATERN52, False, rows=300)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    rp = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    ehvi = lambda e: e.sweep_believer_ehvi(Y[:24], rp, 3, pending=pend[:1], return_values=True)  # noqa: E731
    constrained = lambda e: e.sweep_believer_constrained(ACQ_MIXED[:3], plugin, True, lo, hi, pending=pend[:1], return_values=True)  # noqa: E731

    def engine():
        e = _lib.Engine(0)
        e.set_train(X, Y)
        e.commit(*args)
        e.upload_candidates(Xs)
        return e

    fresh = []
    for call in (ehvi, constrained):
        e = engine()
        try:
            fresh.append(call(e))
        finally:
            e.close()
    e = engine()
    try:
        shared = [ehvi(e), constrained(e), ehvi(e)]
    finally:
        e.close()
    for got, want in zip(shared, fresh + fresh[:1]):
        assert sorted(got) == sorted(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("minimize", [True, False], ids=["min", "max"])
def test_infinite_bounds_give_the_single_target_believer(eng, minimize):
    """Every bound infinite and no feasibility-only step: P is exactly 1.0 on every row, so a value is its base criterion's bits on the
    m-target sweep's moments of target 0, and every believed point is feasible, so the plugin follows `sweep_believer`'s rule.  Against
    `sweep_believer` on the single-target model of column 0 -- another summation order of the mean and of the downdate -- the values
    agree as `k_constrained` promises for P == 1.0 (T19's form; tests/test_gpu_constrained.py), the winners exactly."""
    X, Y, args, Xs, pend = commit(eng, 70, 3, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    plugin = float(Y[:, 0].min() if minimize else -Y[:, 0].max())
    out = eng.sweep_believer_constrained(ACQ_MIXED, plugin, minimize, [-INF, -INF], [INF, INF], pending=pend, return_values=True)
    assert np.all(out["pof"] == 1.0)
    r = restatement(eng, X, args)
    mu = eng.sweep_constrained(ACQ_MIXED[:1], plugin, minimize, [-INF, -INF], [INF, INF], return_moments=True)[2]
    for j in range(Q):  # the base criterion alone on the device's own moments: multiplying by 1.0 changes no bit
        base = R.constrained(mu[:, :1], out["mse"][j][:, :1], r.sigma2[:1], [], [], [ACQ_MIXED[j]], out["plugins"][j], minimize)[0][0]
        t24(out["acq"][j], base, "base step %d" % j)
    eng.set_train(X, Y[:, 0])
    eng.commit(*args)
    eng.upload_candidates(Xs)
    one = eng.sweep_believer(ACQ_MIXED, plugin, minimize, pending=pend, return_values=True)
    np.testing.assert_array_equal(out["best_idx"], one["best_idx"])
    np.testing.assert_allclose(out["pivots"], one["pivots"], rtol=1e-6, atol=1e-12)
    for j in range(Q):
        t24(out["acq"][j], one["acq"][j], "single-target step %d" % j)
        np.testing.assert_allclose(out["mse"][j][:, 0], one["mse"][j], rtol=1e-6, atol=1e-12 * r.sigma2[0])


# ----------------------------------------------------------------------------------------------------------------------
# 4. chunk invariance, in fresh processes
# ----------------------------------------------------------------------------------------------------------------------
def chunk_digests():
    """{n_pend: [sha1 over every output of one call at N = 530, n_chunks of its pass 0, n_passes]} (run in a child process)"""
    res = {}
    e = _lib.Engine(0)
    try:
        X, Y, args, Xs, pend = commit(e, 530, 3, _lib.KERNEL_SE, True)
        e.upload_candidates(Xs)
        lo, hi = quantile_bounds(Y)
        for n_pend in (0, 2):
            out = e.sweep_believer_constrained(ACQ_MIXED, plugin_of(Y, lo, hi, True), True, lo, hi, pending=pend[:n_pend], return_values=True)
            h = hashlib.sha1()
            for k in KEYS:
                h.update(np.ascontiguousarray(out[k]).tobytes())
            res[str(n_pend)] = [h.hexdigest(), e.last_timing()["n_chunks"], e.believer_constrained_last()["n_passes"]]
    finally:
        e.close()
    return res


CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import conftest
from test_gpu_believer_constrained import chunk_digests
print("RESULT " + json.dumps(chunk_digests()))
'''


def _child(chunk_mb):
    e = dict(os.environ)
    e.pop("BOGP_CHUNK_MB", None)
    if chunk_mb is not None:
        e["BOGP_CHUNK_MB"] = chunk_mb
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], cwd=ROOT, env=e,
                       capture_output=True, text=True, timeout=300)  # fmt: skip
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])


def test_chunk_invariance():
    """BOGP_CHUNK_MB=1 at N = 530 (544 padded rows: 192 candidates a chunk, 8 chunks of 1500) against the default, each in a fresh
    child process: every output byte for byte the one-chunk run's, with and without pending points."""
    whole, parts = _child(None), _child("1")
    for n_pend in ("0", "2"):
        assert parts[n_pend][1] >= 4 > whole[n_pend][1], (whole, parts)
        assert whole[n_pend][0] == parts[n_pend][0], (n_pend, whole, parts)
        assert whole[n_pend][2] == parts[n_pend][2] == int(n_pend) + Q - 1


# ----------------------------------------------------------------------------------------------------------------------
# 5. edges
# ----------------------------------------------------------------------------------------------------------------------
def test_pivot_guard(eng):
    """A pending point equal to a training point of a noiseless model is already determined: pivot <= 1e-12, c = 0, and with a fixed
    plugin every output is the one of the run without it; as the last pending point it leaves step 0 to a criterion-only pass."""
    X, Y, args, Xs, pend = commit(eng, 70, 3, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    run = lambda p: eng.sweep_believer_constrained(ACQ_MIXED[:3], plugin, True, lo, hi, pending=p, believe_plugin=False, return_values=True)  # noqa: E731
    base = run(pend[:1])
    trn = run(np.vstack([X[3], pend[:1]]))
    assert trn["pivots"][0] <= 1e-12
    np.testing.assert_array_equal(trn["pivots"][1:], base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "best_mu", "plugins", "acq", "pof", "mse"):
        np.testing.assert_array_equal(trn[k], base[k], err_msg=k)
    last = run(np.vstack([pend[:1], X[5]]))
    assert last["pivots"][1] <= 1e-12
    for k in ("best_val", "best_idx", "acq", "pof", "mse"):
        np.testing.assert_array_equal(last[k], base[k], err_msg=k)
    assert eng.believer_constrained_last()["n_passes"] == 2 + 3 - 1  # the guarded last pending point still runs step 0's pass


def test_every_row_becomes_a_winner_and_degenerate_bounds(eng):
    """q = M = 3: the last step has one row left.  lo == hi: a constraint that no posterior with a variance satisfies -- every value is
    0, and the steps still return q distinct rows, in index order (the first maximum among the rows that compete)."""
    X, Y, args, Xs, pend = commit(eng, 70, 3, _lib.KERNEL_SE, True)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    eng.upload_candidates(Xs[:3])
    out = eng.sweep_believer_constrained(ACQ_MIXED[:3], plugin, True, lo, hi, return_values=True)
    assert sorted(out["best_idx"].tolist()) == [0, 1, 2]
    ref = restatement(eng, X, args).run(Xs[:3], ACQ_MIXED[:3], plugin, True, lo, hi)
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])
    eng.upload_candidates(Xs[:300])
    for acq in (ACQ_MIXED, ACQ_FEASIBILITY):
        zero = eng.sweep_believer_constrained(acq, plugin, True, [0.25, -INF], [0.25, INF], pending=pend[:1], return_values=True)
        assert np.all(zero["acq"] == 0.0) and np.all(zero["pof"] == 0.0) and np.all(zero["best_val"] == 0.0)
        assert zero["best_idx"].tolist() == [0, 1, 2, 3]
        np.testing.assert_array_equal(zero["best_x"], Xs[:4])


def test_candidate_sources(eng):
    X, Y, args, _, pend = commit(eng, 530, 2, _lib.KERNEL_MATERN52, True)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    run = lambda p: eng.sweep_believer_constrained(ACQ_MIXED, plugin, True, lo, hi, pending=p, return_values=True)  # noqa: E731
    eng.generate_candidates(np.full(D, -2.2), np.full(D, 2.2), M, seed=17)
    gen = run(pend[:1])
    Xs = eng.read_candidates(np.arange(M))
    eng.upload_candidates(Xs)
    up = run(pend[:1])
    eng.upload_candidates(Xs, lazy=True)
    lazy = run(pend[:1])
    eng.upload_candidates(Xs, lazy=True)
    lazy0 = run(None)
    eng.upload_candidates(Xs)
    up0 = run(None)
    for k in up:
        np.testing.assert_array_equal(gen[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy0[k], up0[k], err_msg=k)
    np.testing.assert_array_equal(up["best_x"], Xs[up["best_idx"]])


# ----------------------------------------------------------------------------------------------------------------------
# 6. error returns
# ----------------------------------------------------------------------------------------------------------------------
def test_error_returns():
    """Every error return of bogp_sweep_believer_constrained but one: a communicator of more than one rank cannot be built on one device
    (its refusal is a comparison of the handle's world size, exercised by the Python layer's own refusal on the host).  After every
    refusal the handle is usable and answers as before."""
    lib = _lib.load()
    assert lib.bogp_sweep_believer_constrained(None, 1, None, None, 0.0, 1, 1, 1, None, None, None, 0, None, None, None, None, None, None, None,
                                               None, None) == _lib.ERR_INVALID  # fmt: skip
    assert lib.bogp_believer_constrained_last(None, None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, Y, args, Xs, pend = problem(70, 3, _lib.KERNEL_SE, False)
        lo, hi = quantile_bounds(Y)
        e.set_train(X, Y)
        call = lambda acq=ACQ_MIXED, lo=lo, hi=hi, **kw: e.sweep_believer_constrained(acq, 0.0, True, lo, hi, return_values=True, **kw)  # noqa: E731
        with pytest.raises(_lib.BogpError, match="no committed model") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.commit(*args)
        with pytest.raises(_lib.BogpError, match="no candidates") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.upload_candidates(Xs[:200])
        good = call(pending=pend)

        def refused(match, code=_lib.ERR_INVALID, exc=_lib.BogpError, **kw):
            with pytest.raises(exc, match=match) as ei:
                call(**kw)
            if exc is _lib.BogpError:
                assert ei.value.code == code
            again = call(pending=pend)  # the handle is usable afterwards, and answers as before
            assert all(good[k].tobytes() == again[k].tobytes() for k in good)

        refused("n_con = 1", lo=lo[:1], hi=hi[:1])
        refused("q = 0", acq=[])
        refused("<= 32", acq=ACQ_MIXED[:1] * 33)
        refused("<= 32", acq=ACQ_MIXED[:1] * 31, pending=pend)
        refused("UCB", acq=[(_lib.ACQ_UCB, 0.5)])
        refused("unknown acquisition id", acq=[(7, 0.5)])
        refused("must be > 0", acq=[(_lib.ACQ_MGFI, 0.0)])
        refused("must be >= 0", acq=[(_lib.ACQ_EPSILON_PI, -1.0)])
        refused("NaN", lo=[np.nan, -INF])
        refused("below its lower", lo=[1.0, -INF], hi=[0.5, INF])
        bad = pend.copy()
        bad[1, 2] = np.nan
        refused("not finite", pending=bad)
        bv, bi = np.empty(1), np.empty(1, dtype=np.int64)
        ids = np.array([_lib.ACQ_EI], dtype=np.int32)
        ip, lp = ids.ctypes.data_as(_lib._ip), bi.ctypes.data_as(_lib._lp)
        raw = lambda a, l, h, p, n_p, v, i: lib.bogp_sweep_believer_constrained(e._h, 1, a, None, 0.0, 1, 1, 2, l, h, p, n_p, v, i, None, None, None,
                                                                                None, None, None, None)  # noqa: E731  # fmt: skip
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, 0, _lib._ptr(bv), lp) == _lib.OK
        assert raw(None, _lib._ptr(lo), _lib._ptr(hi), None, 0, _lib._ptr(bv), lp) == _lib.ERR_INVALID
        assert raw(ip, None, _lib._ptr(hi), None, 0, _lib._ptr(bv), lp) == _lib.ERR_INVALID
        assert raw(ip, _lib._ptr(lo), None, None, 0, _lib._ptr(bv), lp) == _lib.ERR_INVALID
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, 0, None, lp) == _lib.ERR_INVALID
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, 0, _lib._ptr(bv), None) == _lib.ERR_INVALID
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, 1, _lib._ptr(bv), lp) == _lib.ERR_INVALID  # pending missing
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, -1, _lib._ptr(bv), lp) == _lib.ERR_INVALID
        assert all(good[k].tobytes() == v.tobytes() for k, v in call(pending=pend).items())
        e.upload_candidates(Xs[:3])  # more proposals than candidates
        with pytest.raises(_lib.BogpError, match="proposals from 3 candidates") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.upload_candidates(Xs[:200])
        # a lift on the handle: NotImplementedError from the binding, BOGP_ERR_UNSUPPORTED underneath
        e.set_lift(np.eye(D), np.zeros(D), None, -np.ones(D), np.ones(D))
        with pytest.raises(NotImplementedError, match="lift"):
            call()
        assert raw(ip, _lib._ptr(lo), _lib._ptr(hi), None, 0, _lib._ptr(bv), lp) == _lib.ERR_UNSUPPORTED
        e.clear_lift()
        assert all(good[k].tobytes() == v.tobytes() for k, v in call(pending=pend).items())
        # one target; a polynomial trend basis
        e.set_train(X, Y[:, 0])
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0)
        e.upload_candidates(Xs[:200])
        with pytest.raises(_lib.BogpError, match="1 target") as ei:
            call(lo=lo[:1], hi=hi[:1])
        assert ei.value.code == _lib.ERR_INVALID
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        with pytest.raises(NotImplementedError, match="constant trend"):
            call(lo=lo[:1], hi=hi[:1])
        e.set_train(X, Y)
        e.commit(*args)
        e.upload_candidates(Xs[:200])
        assert all(good[k].tobytes() == v.tobytes() for k, v in call(pending=pend).items())
    finally:
        e.close()


def test_a_forest_handle_is_refused():
    """A handle that holds a forest has no posterior correlation to condition on: BOGP_ERR_UNSUPPORTED, by name."""
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])  # two trees of three nodes over two columns, two values a node
    e = _lib.Engine(0)
    try:
        e.forest_set_multi(d=2, m=2, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                           left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=np.stack([v, v + 1], axis=1))
        e.upload_candidates(np.random.default_rng(0).uniform(size=(10, 2)))
        with pytest.raises(NotImplementedError, match="forest"):
            e.sweep_believer_constrained(ACQ_MIXED[:1], 0.0, True, [-INF], [0.0])
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------------------
# 7. timing spans
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
def test_timing_spans(eng, n_pend):
    """The spans of the passes behind pass 0: producer + solves + k_believer + k_believer_constrained fit inside the call's wall time,
    every kind ran, and n_passes counts one candidate pass per believed point that stands before a step."""
    X, Y, args, Xs, pend = commit(eng, 530, 3, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    lo, hi = quantile_bounds(Y)
    plugin = plugin_of(Y, lo, hi, True)
    eng.sweep_believer_constrained(ACQ_MIXED, plugin, True, lo, hi, pending=pend[:n_pend])  # (allocations, first launches)
    t0 = time.perf_counter()
    eng.sweep_believer_constrained(ACQ_MIXED, plugin, True, lo, hi, pending=pend[:n_pend])
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.believer_constrained_last()
    print("wall %.3f ms" % wall, t)
    assert t["n_passes"] == n_pend + Q - 1
    assert t["corr_ms"] > 0 and t["solve_ms"] > 0 and t["update_ms"] > 0 and t["criterion_ms"] > 0
    assert t["corr_ms"] + t["solve_ms"] + t["update_ms"] + t["criterion_ms"] <= wall
