"""Kriging-believer batches for constrained EHVI on the device (`bogp_sweep_believer_ehvi_constrained`,
kernels_believer_ehvi_constrained.hip): the reference's rebuilt models of golden G44 read as two objectives and one constraint; every
shared case (tests/believer_constrained_ehvi_cases.py, whose conditions tests/test_believer_constrained_ehvi_host.py asserts without
a GPU) against the dense restatement (tests/support/believer_constrained_ehvi_ref.py); the bit identities with the plain constrained
EHVI sweep, with the constrained and the EHVI believer; chunk invariance in fresh processes; the wavefront skip; the edges of the
pivot guard, of q = M, of lo == hi and of the cell limit; candidate sources; the ABI's error returns; the timing spans.

Tolerances: pivots rtol 1e-6, atol 1e-12; means under T1 (rtol 1e-6, atol 1e-9); MSE per target under T2 (rtol 1e-6, atol 1e-12
sigma2_k); values and P under T28 -- T24's / T25's form, |d| <= 1e-6 |ref| + 1e-12 max |ref| on every row with the NaNs on the same
rows, against the restatement's rule evaluated on the device's own moments (on the reference's for G44) with the cells rebuilt from the
device's own believed means.  The models are well conditioned on purpose: the recursion is compared."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT, load_golden

from bogp import _lib, pareto
from believer_constrained_cases import ACQ_FEASIBILITY
from believer_constrained_ehvi_cases import CASES, IDS, D, M, Q, constraint_bounds, feasible_rows, low_ref, narrow_bounds, problem
from support import constrained_ehvi_ref as R
from support.believer_constrained_ehvi_ref import BelieverConstrainedEhviRef, cells_of

pytestmark = pytest.mark.gpu
ENTRY = _lib.SIGNATURES["bogp_sweep_believer_ehvi_constrained"]  # what this module is about: without the entry nothing here can run
INF = float("inf")
KEYS = ("best_val", "best_idx", "best_x", "best_mu", "pivots", "n_cells", "val", "pof", "mse")
NO_CELLS = np.zeros((0, 2))


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def t28(v, ref, what=""):
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(v), nan), (what, np.flatnonzero(np.isnan(v) != nan))  # the NaNs stand on the same rows
    v, ref = v[~nan], ref[~nan]
    err = np.abs(v - ref)
    allow = 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()
    with np.errstate(all="ignore"):
        worst = np.nanmax(np.where(allow > 0, err / allow, np.where(err > 0, np.inf, 0.0))) if err.size else 0.0
    print("T28 %s: max |v - ref| = %.3g, max |ref| = %.3g, largest error over the allowance %.3g, NaN rows %d" % (what, err.max(), np.abs(ref).max(), worst, nan.sum()))
    assert np.all(err <= allow), (what, err.max())


def commit(eng, N, m, kernel, noisy, seed=0, rows=M):
    p = problem(N, m, kernel, noisy, seed, rows)
    eng.set_train(p[0], p[1])
    eng.commit(*p[2])
    return p


def setup(eng, N, m_obj, c, kernel=_lib.KERNEL_MATERN52, noisy=False, rows=M, bounds=None):
    """commit, upload and the pieces of a call: (X, Y, args, Xs, pend, lo, hi, ref_point, front)"""
    X, Y, args, Xs, pend = commit(eng, N, m_obj + c, kernel, noisy, rows=rows)
    eng.upload_candidates(Xs)
    lo, hi = constraint_bounds(Y, m_obj) if bounds is None else constraint_bounds(Y, m_obj, bounds)
    return X, Y, args, Xs, pend, lo, hi, low_ref(Y, m_obj), Y[feasible_rows(Y, m_obj, lo, hi), :m_obj].copy()


def restatement(eng, X, args):
    return BelieverConstrainedEhviRef(X, args[2][:D], args[0], eng.get_state())


def device_moments(eng, m_obj, lo, hi):
    """the device's own means (no step moves them): bogp_sweep_ehvi_constrained over no cells"""
    z = np.zeros((0, m_obj))
    return eng.sweep_ehvi_constrained(z, z, lo, hi, return_moments=True)[2]


def check_values(out, mu, sigma2, m_obj, lo, hi, rp, front, n_pend, believe_front, feasibility_only, pend_mu, what=""):
    """values and P of every step under T28 against the restatement's rule on the device's own moments, with the cells rebuilt from the
    device's own believed means (`pend_mu`: the pending points' means, which the device does not return, from the restatement)"""
    believed = np.vstack([np.asarray(pend_mu, float).reshape(-1, mu.shape[1]), out["best_mu"]])
    for j in range(len(out["best_val"])):
        F = np.asarray(front, float).reshape(-1, m_obj)
        if believe_front and not feasibility_only:
            for mu_p in believed[: n_pend + j]:
                if np.all((lo <= mu_p[m_obj:]) & (mu_p[m_obj:] <= hi)):
                    F = np.vstack([F, mu_p[None, :m_obj]])
        lower, upper = cells_of(pareto.pareto_front(F, rp), rp, feasibility_only)
        assert out["n_cells"][j] == len(lower), (what, j)
        v, P = R.values(mu, out["mse"][j], sigma2, m_obj, lower, upper, lo, hi)
        t28(out["val"][j], v, "%s values step %d" % (what, j))
        t28(out["pof"][j], P, "%s P step %d" % (what, j))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference's rebuilt models
# ----------------------------------------------------------------------------------------------------------------------
def test_g44_reference_golden(eng):
    """G44's `m3` state (tests/support/make_believer_ehvi_golden.py) read as two objectives and one constraint under the quantile
    bounds: for each prefix of four believed rows a reference model REBUILT on X + {p_1 .. p_j} with y = mu(p) at the same theta.  With
    q = 1, pending = believed[:j] and believe_front=False: the device's MSE / sigma2 against the rebuilt model's mse_j / sigma2_j (rtol
    1e-6, atol 1e-12), the means, which must not move, under T1, and the value and P against the restatement on the reference's moments
    -- its bracket in units of the committed sigma2, which the believer keeps fixed -- under T28."""
    g = {k[3:]: v for k, v in load_golden("G44_believer_ehvi").items() if k.startswith("m3_")}
    m = g["y"].shape[1]
    assert m == 3
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], 0.0, False, float(g["beta"]))
    sigma2 = eng.get_state(with_C=False)["sigma2"]
    np.testing.assert_allclose(sigma2, g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    lo, hi = constraint_bounds(g["y"], 2)
    rp = low_ref(g["y"], 2)
    front = g["y"][feasible_rows(g["y"], 2, lo, hi), :2]
    lower, upper = cells_of(pareto.pareto_front(front, rp), rp)
    mu = device_moments(eng, 2, lo, hi)
    for j in range(1, 5):
        mse_ref = g["mse_j"][j - 1] / g["sigma2_j"][j - 1] * sigma2
        out = eng.sweep_believer_ehvi_constrained(front, rp, 1, lo, hi, pending=g["believed"][:j], believe_front=False, return_values=True)
        assert out["n_cells"][0] == len(lower)
        v, P = R.values(g["mu_j"][j - 1], mse_ref, sigma2, 2, lower, upper, lo, hi)
        t28(out["val"][0], v, "G44 m3 prefix %d values" % j)
        t28(out["pof"][0], P, "G44 m3 prefix %d P" % j)
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
    X, Y, args, Xs, pend, lo, hi, rp, front = case.build()
    eng.set_train(X, Y)
    eng.commit(*args)
    eng.upload_candidates(Xs)
    kw = dict(pending=pend, believe_front=case.believe_front, feasibility_only=case.feasibility_only)
    out = eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, return_values=True, **kw)
    r = restatement(eng, X, args)
    assert len(set(np.round(r.sigma2, 12))) == case.m  # distinct sigma2_k
    ref = r.run(Xs, front, rp, Q, lo, hi, **kw)
    rel = (ref["best_val"] - ref["second"]) / np.abs(ref["best_val"])
    print("winner / runner-up gaps", rel, "n_cells", out["n_cells"], "pivots", out["pivots"])
    np.testing.assert_allclose(out["pivots"], ref["pivots"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(out["best_mu"], ref["best_mu"], rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(out["n_cells"], ref["n_cells"])
    mu = device_moments(eng, case.m_obj, lo, hi)
    np.testing.assert_allclose(mu, ref["mu"], rtol=1e-6, atol=1e-9)
    for j in range(Q):
        for t in range(case.m):
            np.testing.assert_allclose(out["mse"][j][:, t], ref["mse"][j][:, t], rtol=1e-6, atol=1e-12 * r.sigma2[t], err_msg="mse step %d target %d" % (j, t))
    check_values(out, mu, r.sigma2, case.m_obj, lo, hi, rp, front, case.n_pend, case.believe_front, case.feasibility_only,
                 ref["believed_mu"][: case.n_pend], case.id)  # fmt: skip
    for j in range(Q):
        assert out["best_idx"][j] == ref["best_idx"][j], j
        free = np.ones(len(Xs), bool)
        free[out["best_idx"][:j]] = False  # the winners before keep their value but do not compete
        assert out["best_idx"][j] == int(np.flatnonzero(free)[np.argmax(out["val"][j][free])]) and out["best_val"][j] == out["val"][j][out["best_idx"][j]]
    assert len(set(out["best_idx"].tolist())) == Q and len(out["pivots"]) == case.n_pend + Q
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])
    if not case.noisy:  # every candidate row believed so far is determined
        for j in range(1, Q):
            assert np.all(out["mse"][j][out["best_idx"][:j]] == 0.0)
    if case.feasibility_only:
        assert out["val"].tobytes() == out["pof"].tobytes() and np.all(out["n_cells"] == 0)


# ----------------------------------------------------------------------------------------------------------------------
# 3. bit identities
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_step0_is_sweep_ehvi_constrained_and_nothing_leaks(eng, N):
    X, Y, args, Xs, pend, lo, hi, rp, front = setup(eng, N, 2, 1)
    lower, upper = cells_of(pareto.pareto_front(front, rp), rp)
    for cells, kw in (((lower, upper), {}), ((NO_CELLS, NO_CELLS), dict(feasibility_only=True))):
        before = eng.sweep_ehvi_constrained(cells[0], cells[1], lo, hi, return_values=True, return_pof=True, return_moments=True)
        out = eng.sweep_believer_ehvi_constrained(NO_CELLS if kw else front, rp, Q, lo, hi, return_values=True, **kw)
        assert out["best_val"][0] == before[0][0] and out["best_idx"][0] == before[1][0] and out["n_cells"][0] == len(cells[0])
        assert out["val"][0].tobytes() == before[2].tobytes() and out["pof"][0].tobytes() == before[3].tobytes()
        assert out["mse"][0].tobytes() == before[5].tobytes()
        np.testing.assert_array_equal(out["best_mu"][0], before[4][out["best_idx"][0]])
    topk = eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=3, return_values=True, return_pof=True, return_moments=True)
    eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=pend)
    after = eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=3, return_values=True, return_pof=True, return_moments=True)
    for b, a in zip(topk, after):
        assert b.tobytes() == a.tobytes()


@pytest.mark.parametrize("m_obj,c", [(2, 1), (2, 2), (3, 1)])
def test_a_feasibility_only_batch_is_the_constrained_believer_with_no_criterion(eng, m_obj, c):
    """Feasibility only: `sweep_believer_constrained` with ACQ_NONE x q on the same model, infinite bounds on columns 1 .. m_obj - 1
    (factors of exactly 1.0 change no bit) and the same bounds on the constraint columns: P, MSE, winners and pivots byte for byte."""
    X, Y, args, Xs, pend, lo, hi, rp, _ = setup(eng, 70, m_obj, c, bounds=narrow_bounds)
    for p in (None, pend):
        out = eng.sweep_believer_ehvi_constrained(None, rp, Q, lo, hi, pending=p, feasibility_only=True, return_values=True)
        lo1, hi1 = np.r_[np.full(m_obj - 1, -INF), lo], np.r_[np.full(m_obj - 1, INF), hi]
        one = eng.sweep_believer_constrained(ACQ_FEASIBILITY, 0.0, True, lo1, hi1, pending=p, return_values=True)
        for k in ("pof", "mse", "best_idx", "pivots"):
            assert out[k].tobytes() == one[k].tobytes(), k
        assert out["val"].tobytes() == one["acq"].tobytes() == out["pof"].tobytes()
        assert np.all(out["n_cells"] == 0)


def test_infinite_bounds_give_the_ehvi_believer(eng):
    """Every bound infinite: P == 1.0 exactly on every row, every believed point is feasible by belief, so the front follows
    `sweep_believer_ehvi`'s rule.  Against `sweep_believer_ehvi` on the model of the objective columns -- the same bracket, its own
    kernel -- the winners and n_cells are equal and the values agree under T28."""
    X, Y, args, Xs, pend, lo, hi, rp, _ = setup(eng, 70, 2, 1)
    front = Y[:, :2]
    out = eng.sweep_believer_ehvi_constrained(front, rp, Q, [-INF], [INF], pending=pend, return_values=True)
    assert np.all(out["pof"] == 1.0)
    eng.set_train(X, Y[:, :2])
    eng.commit(*args)
    eng.upload_candidates(Xs)
    two = eng.sweep_believer_ehvi(front, rp, Q, pending=pend, return_values=True)
    np.testing.assert_array_equal(out["best_idx"], two["best_idx"])
    np.testing.assert_array_equal(out["n_cells"], two["n_cells"])
    np.testing.assert_allclose(out["pivots"], two["pivots"], rtol=1e-6, atol=1e-12)
    for j in range(Q):
        t28(out["val"][j], two["ehvi"][j], "EHVI believer step %d" % j)


def test_families_share_one_handle():
    """`sweep_believer_ehvi`, `sweep_believer_constrained`, `sweep_believer_ehvi_constrained` and `sweep_believer_ehvi` again on ONE
    engine: the families lay out the handle's shared believer arrays differently, and every array of every call must equal the same
    call's on a freshly created engine -- nothing is sized or offset from the call before."""
    X, Y, args, Xs, pend = problem(70, 3, _lib.KERNEL_MATERN52, False, rows=300)
    lo, hi = constraint_bounds(Y, 2)
    lo1, hi1 = np.r_[-INF, lo], np.r_[INF, hi]
    rp3, rp = Y.min(axis=0) - 0.1, low_ref(Y, 2)
    front = Y[feasible_rows(Y, 2, lo, hi), :2]
    acq = [(_lib.ACQ_EI, 0.0)] * 3
    ehvi = lambda e: e.sweep_believer_ehvi(Y[:6], rp3, 3, pending=pend[:1], return_values=True)  # noqa: E731
    constrained = lambda e: e.sweep_believer_constrained(acq, float(Y[:, 0].min()), True, lo1, hi1, pending=pend[:1], return_values=True)  # noqa: E731
    new = lambda e: e.sweep_believer_ehvi_constrained(front, rp, 3, lo, hi, pending=pend[:1], return_values=True)  # noqa: E731

    def engine():
        e = _lib.Engine(0)
        e.set_train(X, Y)
        e.commit(*args)
        e.upload_candidates(Xs)
        return e

    fresh = []
    for call in (ehvi, constrained, new):
        e = engine()
        try:
            fresh.append(call(e))
        finally:
            e.close()
    e = engine()
    try:
        shared = [ehvi(e), constrained(e), new(e), ehvi(e)]
    finally:
        e.close()
    for got, want in zip(shared, fresh + fresh[:1]):
        assert sorted(got) == sorted(want)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 4. chunk invariance, in fresh processes
# ----------------------------------------------------------------------------------------------------------------------
def chunk_digests():
    """{n_pend: [sha1 over every output of one call at N = 530, n_chunks of its pass 0, n_passes]} (run in a child process)"""
    res = {}
    e = _lib.Engine(0)
    try:
        X, Y, args, Xs, pend, lo, hi, rp, front = setup(e, 530, 2, 1, _lib.KERNEL_SE, True)
        for n_pend in (0, 2):
            out = e.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=pend[:n_pend], return_values=True)
            h = hashlib.sha1()
            for k in KEYS:
                h.update(np.ascontiguousarray(out[k]).tobytes())
            res[str(n_pend)] = [h.hexdigest(), e.last_timing()["n_chunks"], e.believer_ehvi_constrained_last()["n_passes"]]
    finally:
        e.close()
    return res


CHILD = r'''
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import conftest
from test_gpu_believer_constrained_ehvi import chunk_digests
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
    """BOGP_CHUNK_MB=1 at N = 530 against the default, each in a fresh child process (one at a time): every output byte for byte the
    one-chunk run's, with and without pending points."""
    whole, parts = _child(None), _child("1")
    for n_pend in ("0", "2"):
        assert parts[n_pend][1] > 1 >= whole[n_pend][1], (whole, parts)
        assert whole[n_pend][0] == parts[n_pend][0], (n_pend, whole, parts)
        assert whole[n_pend][2] == parts[n_pend][2] == int(n_pend) + Q - 1


# ----------------------------------------------------------------------------------------------------------------------
# 5. the skip path
# ----------------------------------------------------------------------------------------------------------------------
def test_wavefronts_without_a_feasible_row_skip_the_cells(eng):
    """A noiseless model whose candidates' first rows are infeasible training rows (their constraint value at least 0.05 off its
    interval): the constraint is determined there, P == 0.0 and the value exactly +0.0 in every step -- the first wavefronts have no
    live lane and skip the cell loop -- and the rest agrees with the rule under T28."""
    X, Y, args, Xs, pend = commit(eng, 530, 3, _lib.KERNEL_MATERN52, False)
    lo, hi = constraint_bounds(Y, 2)
    rows = np.flatnonzero(np.maximum(lo[0] - Y[:, 2], Y[:, 2] - hi[0]) > 0.05)  # infeasible, by this much
    n = len(rows) // 64 * 64
    assert n >= 128
    Xc = np.vstack([X[rows[:n]], Xs[: 700 - n]])
    eng.upload_candidates(Xc)
    rp, front = low_ref(Y, 2), Y[feasible_rows(Y, 2, lo, hi), :2]
    out = eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=pend[:1], return_values=True)
    assert np.all(out["pof"][:, :n] == 0.0) and np.all(out["val"][:, :n] == 0.0) and not np.any(np.signbit(out["val"][:, :n]))
    assert np.all(out["best_idx"] >= n)
    r = restatement(eng, X, args)
    ref = r.run(Xc, front, rp, Q, lo, hi, pending=pend[:1])
    check_values(out, device_moments(eng, 2, lo, hi), r.sigma2, 2, lo, hi, rp, front, 1, True, False, ref["believed_mu"][:1], "skip")
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])


# ----------------------------------------------------------------------------------------------------------------------
# 6. edges
# ----------------------------------------------------------------------------------------------------------------------
def test_pivot_guard(eng):
    """A pending point equal to a training point of a noiseless model, and a pending point given twice, are already determined:
    pivot <= 1e-12, c = 0, the step is evaluated without an update and -- with a fixed front -- every output is the one of the run
    without the point; as the last pending point it leaves step 0 to a criterion-only launch."""
    X, Y, args, Xs, pend, lo, hi, rp, front = setup(eng, 70, 2, 1)
    run = lambda p: eng.sweep_believer_ehvi_constrained(front, rp, 3, lo, hi, pending=p, believe_front=False, return_values=True)  # noqa: E731
    base = run(pend[:1])
    trn = run(np.vstack([X[3], pend[:1]]))
    assert trn["pivots"][0] <= 1e-12
    np.testing.assert_array_equal(trn["pivots"][1:], base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "best_mu", "n_cells", "val", "pof", "mse"):
        np.testing.assert_array_equal(trn[k], base[k], err_msg=k)
    for last in (np.vstack([pend[:1], X[5]]), np.vstack([pend[:1], pend[:1]])):
        got = run(last)
        assert got["pivots"][1] <= 1e-12
        for k in ("best_val", "best_idx", "n_cells", "val", "pof", "mse"):
            np.testing.assert_array_equal(got[k], base[k], err_msg=k)
        assert eng.believer_ehvi_constrained_last()["n_passes"] == 2 + 3 - 1  # the guarded last pending point still runs step 0's launch


def test_every_row_becomes_a_winner_and_degenerate_bounds(eng):
    """q = M = 4: the last step has one row left.  lo == hi: a constraint that no posterior with a variance satisfies -- every value is
    +0.0, and the steps still return q distinct rows, in index order (the first maximum among the rows that compete)."""
    X, Y, args, Xs, pend, lo, hi, rp, front = setup(eng, 70, 2, 2, _lib.KERNEL_SE, True)
    eng.upload_candidates(Xs[:Q])
    out = eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, return_values=True)
    assert sorted(out["best_idx"].tolist()) == list(range(Q))
    ref = restatement(eng, X, args).run(Xs[:Q], front, rp, Q, lo, hi)
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])
    eng.upload_candidates(Xs[:300])
    for kw in ({}, dict(feasibility_only=True)):
        zero = eng.sweep_believer_ehvi_constrained(None if kw else front, rp, Q, [0.25, -INF], [0.25, INF], pending=pend[:1], return_values=True, **kw)
        assert np.all(zero["val"] == 0.0) and not np.any(np.signbit(zero["val"])) and np.all(zero["pof"] == 0.0) and np.all(zero["best_val"] == 0.0)
        assert zero["best_idx"].tolist() == [0, 1, 2, 3]
        np.testing.assert_array_equal(zero["best_x"], Xs[:4])


def test_the_cell_limit_names_the_step(eng):
    """A front of 255 points in three objectives fills the limit at step 0 (256 x 256 cells); the first believed mean -- feasible under
    infinite bounds, and neither dominated by nor dominating a front whose points each have two huge coordinates -- adds a grid line on
    both axes: BOGP_ERR_INVALID at step 1, by name.  One point more and step 0 itself is refused, before any device work.  64 candidates."""
    X, Y, args, Xs, pend, lo, hi, _, _ = setup(eng, 70, 3, 1, rows=64)
    n = 255
    assert (n + 1) ** 2 == _lib.MAX_EHVI_CELLS
    rp = np.full(3, -100.0)
    i = np.arange(n)
    front = np.c_[rp[0] + 1e-3 * (i + 1), 1e3 + i, 2e3 - i]  # an anti-chain: the second coordinate rises as the third falls
    assert len(pareto.pareto_front(front, rp)) == n
    ok = eng.sweep_believer_ehvi_constrained(front, rp, 1, [-INF], [INF])
    assert ok["n_cells"][0] == _lib.MAX_EHVI_CELLS
    with pytest.raises(_lib.BogpError, match="step 1: the front of %d points" % (n + 1)) as ei:
        eng.sweep_believer_ehvi_constrained(front, rp, 2, [-INF], [INF])
    assert ei.value.code == _lib.ERR_INVALID
    held = eng.sweep_believer_ehvi_constrained(front, rp, 2, [-INF], [INF], believe_front=False)  # a fixed front stays inside the limit
    assert held["n_cells"].tolist() == [_lib.MAX_EHVI_CELLS] * 2 and held["best_idx"][0] == ok["best_idx"][0]
    more = np.vstack([front, [[rp[0] + 0.5e-3, 999.0, 3e3]]])
    with pytest.raises(_lib.BogpError, match="step 0: the front of %d points" % (n + 1)) as ei:
        eng.sweep_believer_ehvi_constrained(more, rp, 1, [-INF], [INF])
    assert ei.value.code == _lib.ERR_INVALID


def test_candidate_sources(eng):
    X, Y, args, _, pend, lo, hi, rp, front = setup(eng, 530, 2, 1, _lib.KERNEL_MATERN52, True)
    run = lambda p: eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=p, return_values=True)  # noqa: E731
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
# 7. error returns
# ----------------------------------------------------------------------------------------------------------------------
def test_error_returns():
    """Every error return of bogp_sweep_believer_ehvi_constrained but one: a communicator of more than one rank cannot be built on one
    device (its refusal is a comparison of the handle's world size, exercised by the Python layer's own refusal on the host).  After
    every refusal the handle is usable and answers as before."""
    lib = _lib.load()
    assert len(ENTRY[1]) == 22
    assert lib.bogp_sweep_believer_ehvi_constrained(None, 2, 1, None, None, 0, 0, 1, 1, None, None, None, 0, None, None, None, None, None, None,
                                                    None, None, None) == _lib.ERR_INVALID  # fmt: skip
    assert lib.bogp_believer_ehvi_constrained_last(None, None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, Y, args, Xs, pend = problem(70, 3, _lib.KERNEL_SE, False)
        lo, hi = constraint_bounds(Y, 2)
        rp, front = low_ref(Y, 2), Y[feasible_rows(Y, 2, lo, hi), :2]
        e.set_train(X, Y)
        call = lambda front=front, rp=rp, q=Q, lo=lo, hi=hi, **kw: e.sweep_believer_ehvi_constrained(front, rp, q, lo, hi, return_values=True, **kw)  # noqa: E731
        with pytest.raises(_lib.BogpError, match="no committed model") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.commit(*args)
        with pytest.raises(_lib.BogpError, match="no candidates") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.upload_candidates(Xs[:200])
        good = call(pending=pend)

        def refused(match, code=_lib.ERR_INVALID, **kw):
            with pytest.raises(_lib.BogpError, match=match) as ei:
                call(**kw)
            assert ei.value.code == code
            again = call(pending=pend)  # the handle is usable afterwards, and answers as before
            assert all(good[k].tobytes() == again[k].tobytes() for k in good)

        refused("m_obj = 1", rp=rp[:1], front=front[:, :1], lo=np.r_[-INF, lo], hi=np.r_[INF, hi])
        refused("n_con = 0", lo=[], hi=[])
        refused("m_obj \\+ n_con = 2 \\+ 2", lo=np.r_[lo, lo], hi=np.r_[hi, hi])
        refused("m_obj \\+ n_con = 3 \\+ 1", rp=np.r_[rp, 0.0], front=None)
        refused("q = 0", q=0)
        refused("<= 32", q=33)
        refused("<= 32", q=31, pending=pend)
        refused("feasibility_only", feasibility_only=True)
        refused("ref_point entry 1 is not finite", rp=np.array([rp[0], INF]))
        bad = front.copy()
        bad[1, 0] = np.nan
        refused("front entry 2 is not finite", front=bad)
        bad = pend.copy()
        bad[1, 2] = np.nan
        refused("pending entry 5 is not finite", pending=bad)
        refused("NaN", lo=[np.nan])
        refused("below its lower", lo=[1.0], hi=[0.5])
        bv, bi = np.empty(1), np.empty(1, dtype=np.int64)
        lp = bi.ctypes.data_as(_lib._lp)
        P = _lib._ptr
        raw = lambda r, f, n_f, n_c, l, h, p, n_p, v, i: lib.bogp_sweep_believer_ehvi_constrained(e._h, 2, 1, r, f, n_f, 0, 1, n_c, l, h, p, n_p, v, i,
                                                                                                  None, None, None, None, None, None, None)  # noqa: E731  # fmt: skip
        fr = np.ascontiguousarray(front)
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.OK
        assert raw(P(rp), None, 0, 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.OK
        assert raw(P(rp), P(fr), len(fr), 0, P(lo), P(hi), None, 0, P(bv), lp) == _lib.ERR_INVALID  # n_con < 1
        assert raw(None, P(fr), len(fr), 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.ERR_INVALID
        assert raw(P(rp), None, len(fr), 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.ERR_INVALID  # front missing
        assert raw(P(rp), P(fr), -1, 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.ERR_INVALID
        assert raw(P(rp), P(fr), len(fr), 1, None, P(hi), None, 0, P(bv), lp) == _lib.ERR_INVALID
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), None, None, 0, P(bv), lp) == _lib.ERR_INVALID
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, 0, None, lp) == _lib.ERR_INVALID
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, 0, P(bv), None) == _lib.ERR_INVALID
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, 1, P(bv), lp) == _lib.ERR_INVALID  # pending missing
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, -1, P(bv), lp) == _lib.ERR_INVALID
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
        assert raw(P(rp), P(fr), len(fr), 1, P(lo), P(hi), None, 0, P(bv), lp) == _lib.ERR_UNSUPPORTED
        e.clear_lift()
        assert all(good[k].tobytes() == v.tobytes() for k, v in call(pending=pend).items())
        # a polynomial trend basis (one target: several take the constant trend only)
        e.set_train(X, Y[:, 0])
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        e.upload_candidates(Xs[:200])
        with pytest.raises(NotImplementedError, match="constant trend"):
            call()
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0)
        with pytest.raises(_lib.BogpError, match="has 1 targets") as ei:
            call()
        assert ei.value.code == _lib.ERR_INVALID
        e.set_train(X, Y)
        e.commit(*args)
        e.upload_candidates(Xs[:200])
        assert all(good[k].tobytes() == v.tobytes() for k, v in call(pending=pend).items())
    finally:
        e.close()


def test_a_forest_handle_is_refused():
    """A handle that holds a forest has no posterior correlation to condition on: BOGP_ERR_UNSUPPORTED, by name."""
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])  # two trees of three nodes over two columns, three values a node
    e = _lib.Engine(0)
    try:
        e.forest_set_multi(d=2, m=3, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                           left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=np.stack([v, v + 1, v + 2], axis=1))
        e.upload_candidates(np.random.default_rng(0).uniform(size=(10, 2)))
        with pytest.raises(NotImplementedError, match="forest"):
            e.sweep_believer_ehvi_constrained(None, [0.0, 0.0], 1, [-INF], [0.0])
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------------------
# 8. timing spans
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
def test_timing_spans(eng, n_pend):
    """The spans of the passes behind pass 0: every field finite and >= 0, the criterion kernel ran, the four kinds fit inside the
    call's wall time, and n_passes counts one candidate pass per believed point that stands before a step."""
    X, Y, args, Xs, pend, lo, hi, rp, front = setup(eng, 530, 2, 1)
    eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=pend[:n_pend])  # (allocations, first launches)
    t0 = time.perf_counter()
    eng.sweep_believer_ehvi_constrained(front, rp, Q, lo, hi, pending=pend[:n_pend])
    wall = (time.perf_counter() - t0) * 1e3
    t = eng.believer_ehvi_constrained_last()
    print("wall %.3f ms" % wall, t)
    assert sorted(t) == ["corr_ms", "criterion_ms", "n_passes", "solve_ms", "update_ms"]
    assert all(np.isfinite(v) and v >= 0 for v in t.values())
    assert t["n_passes"] == n_pend + Q - 1
    assert t["criterion_ms"] > 0 and t["corr_ms"] > 0 and t["solve_ms"] > 0 and t["update_ms"] > 0
    assert t["corr_ms"] + t["solve_ms"] + t["update_ms"] + t["criterion_ms"] <= wall
