"""Kriging-believer batches under EHVI on the device (`bogp_sweep_believer_ehvi`, kernels_believer_ehvi.hip): the golden G44
recorded from the reference's own models rebuilt on X + the believed points; the dense NumPy restatement
(tests/support/believer_ehvi_ref.py) over sizes, targets, kernels, modes, pending points and the front rule; step 0 against
`sweep_ehvi` bit for bit and no leakage into later sweeps; chunk invariance; the edges of the front and of the pivot guard;
candidate sources; the ABI's error returns.

Tolerances: MSE per target under T2 (rtol 1e-6, atol 1e-12 sigma2_k), means under T1 (rtol 1e-6, atol 1e-9), EHVI under T12
(|d| <= 1e-6 |ref| + 1e-12 max |ref|) against the float64 restatement of the reference's algebra evaluated on the device's own
moments (as tests/test_gpu_ehvi.py compares it), against the reference's float32 values by G39's rule (1e-5 of the batch maximum).
The models are well conditioned on purpose: the recursion is compared, not the factorisation."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden

from bogp import _lib
from bogp import pareto
from support.believer_ehvi_ref import BelieverEhviRef
from support.ehvi_ref64 import ehvi as ehvi_ref

pytestmark = pytest.mark.gpu

M, D, Q = 1500, 3, 4


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def problem(N, m, kernel, noisy, seed=0):
    """(X, Y, commit arguments, candidates, two pending rows off the candidates, front rows, ref_point): N = 70 pads to 96 rows
    (a partial 32-row slice), N = 530 is chunked under BOGP_CHUNK_MB=1.  Distinct per-target scales, so that the sigma2_k differ;
    short length scales keep R well conditioned.  The front is formed from a few of the observed rows: a small grid."""
    rng = np.random.default_rng(1000 * seed + 10 * N + m)
    X = rng.uniform(-2, 2, size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    theta = np.array([1.0, 0.8, 1.3]) * (4.0 if N < 100 else 8.0)
    if noisy:
        args = (kernel, _lib.MODE_NOISE_ESTIM, np.r_[theta, 0.9], 0.0, False, 0.1)
    else:
        args = (kernel, _lib.MODE_NOISELESS, theta, 0.0, False, 0.1)
    Xs = rng.uniform(-2.2, 2.2, size=(M, D))
    pend = rng.uniform(-2, 2, size=(2, D))
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    front = Y[: (24 if m == 2 else 10)]
    return X, Y, args, Xs, pend, front, ref


def commit(eng, N, m, kernel, noisy, seed=0):
    p = problem(N, m, kernel, noisy, seed)
    eng.set_train(p[0], p[1])
    eng.commit(*p[2])
    return p


def restatement(eng, X, args):
    return BelieverEhviRef(X, args[2][:D], args[0], eng.get_state())


def t12(vals, ref):
    assert np.all(np.abs(vals - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()), np.abs(vals - ref).max()


def check_against(eng, out, ref, r, n_pend, Xs, lo0, hi0):
    """the device's outputs `out` against the restatement's `ref`"""
    rel = (ref["best_val"] - ref["second"]) / np.abs(ref["best_val"])
    print("winner / runner-up gaps", rel, "n_cells", out["n_cells"], "pivots", out["pivots"])
    assert np.all(rel > 1e-9), rel  # the restatement's winner is no tie: a wrong index cannot hide
    np.testing.assert_allclose(out["pivots"], ref["pivots"], rtol=1e-6, atol=1e-12)
    np.testing.assert_array_equal(out["n_cells"], ref["n_cells"])
    np.testing.assert_allclose(out["best_mu"], ref["best_mu"], rtol=1e-6, atol=1e-9)
    mu = eng.sweep_ehvi(lo0, hi0, return_moments=True)[2]  # the device's own means (no step moves them)
    np.testing.assert_allclose(mu, ref["mu"], rtol=1e-6, atol=1e-9)
    for j in range(len(out["best_idx"])):
        for t in range(r.m):
            np.testing.assert_allclose(out["mse"][j][:, t], ref["mse"][j][:, t], rtol=1e-6, atol=1e-12 * r.sigma2[t], err_msg="mse step %d target %d" % (j, t))
        t12(out["ehvi"][j], ehvi_ref(mu, out["mse"][j], *ref["cells"][j]))
        assert out["best_idx"][j] == ref["best_idx"][j], j
        free = np.ones(len(Xs), bool)
        free[out["best_idx"][:j]] = False  # the winners before keep their value but do not compete
        assert out["best_idx"][j] == int(np.flatnonzero(free)[np.argmax(out["ehvi"][j][free])]) and out["best_val"][j] == out["ehvi"][j][out["best_idx"][j]]
    assert len(set(out["best_idx"].tolist())) == len(out["best_idx"])
    assert len(out["pivots"]) == n_pend + len(out["best_idx"])
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])


# ----------------------------------------------------------------------------------------------------------------------
# 1. the reference's rebuilt models
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["m2", "m3"])
def test_g44_reference_golden(eng, state):
    """G44 (tests/support/make_believer_ehvi_golden.py): for each prefix of four believed rows -- two pending points off the
    candidates, then two candidate rows -- a reference model REBUILT on X + {p_1 .. p_j} with y = mu(p) at the same theta and
    sigma2.  The device's MSE_j / sigma2 against the rebuilt model's predict (rtol 1e-6, atol 1e-12), the mean, which must not
    move, under T1; the device's EHVI over its own grid cells of y u mu(p_1 .. p_j) against the reference's per-row float32 EHVI
    by G39's rule, and against the float64 restatement on the reference's moments and the reference's OWN cells (T12): the grid
    and the reference's partition give the same EHVI."""
    g = {k[len(state) + 1 :]: v for k, v in load_golden("G44_believer_ehvi").items() if k.startswith(state + "_")}
    m = g["y"].shape[1]
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], 0.0, False, float(g["beta"]))
    sigma2 = eng.get_state(with_C=False)["sigma2"]
    np.testing.assert_allclose(sigma2, g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    lo0, hi0 = _lib.grid_cells(g["y"], g["ref_point"])
    mu = eng.sweep_ehvi(lo0, hi0, return_moments=True)[2]
    for j in range(1, 5):
        out = eng.sweep_believer_ehvi(g["y"], g["ref_point"], 1, pending=g["believed"][:j], return_values=True)
        lo, hi = g["lower_%d" % j], g["upper_%d" % j]
        ref64 = ehvi_ref(g["mu_j"][j - 1], g["mse_j"][j - 1], lo, hi)
        d32 = np.abs(out["ehvi"][0] - g["ehvi32_j"][j - 1]).max() / np.abs(g["ehvi32_j"][j - 1]).max()
        print("G44 %s prefix %d: max |d(MSE/sigma2)| = %.3g, EHVI vs float32 %.3g of the maximum, vs float64 max |d| %.3g (max %.3g), cells %d (reference's %d)"
              % (state, j, np.abs(out["mse"][0] / sigma2 - g["mse_j"][j - 1] / g["sigma2_j"][j - 1]).max(), d32,
                 np.abs(out["ehvi"][0] - ref64).max(), np.abs(ref64).max(), out["n_cells"][0], len(lo)))  # fmt: skip
        for t in range(m):
            np.testing.assert_allclose(out["mse"][0][:, t] / sigma2[t], g["mse_j"][j - 1][:, t] / g["sigma2_j"][j - 1][t], rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(mu[:, t], g["mu_j"][j - 1][:, t], rtol=1e-6, atol=1e-9)
        assert d32 <= 1e-5
        t12(out["ehvi"][0], ref64)
        assert np.all(out["pivots"][:j] > 1e-3)
    assert np.all(out["mse"][0][g["believed_rows"]] <= 1e-12 * sigma2)  # the believed candidate rows are determined


# ----------------------------------------------------------------------------------------------------------------------
# 2. the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("believe_front", [True, False], ids=["front", "fixedfront"])
@pytest.mark.parametrize("noisy", [False, True], ids=["noiseless", "noisy"])
@pytest.mark.parametrize("kernel", [_lib.KERNEL_MATERN52, _lib.KERNEL_SE], ids=["m52", "se"])
@pytest.mark.parametrize("n_pend", [0, 2])
@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("N", [70, 530])
def test_restatement_parity(eng, N, m, n_pend, kernel, noisy, believe_front):
    X, Y, args, Xs, pend, front, rp = commit(eng, N, m, kernel, noisy)
    eng.upload_candidates(Xs)
    out = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:n_pend], believe_front=believe_front, return_values=True)
    r = restatement(eng, X, args)
    assert len(set(np.round(r.sigma2, 12))) == m  # distinct sigma2_k
    ref = r.run(Xs, front, rp, Q, pending=pend[:n_pend], believe_front=believe_front)
    check_against(eng, out, ref, r, n_pend, Xs, *pareto.hypercell_bounds(front, rp))
    if not noisy:  # every candidate row believed so far is determined
        for j in range(1, Q):
            assert np.all(out["mse"][j][out["best_idx"][:j]] == 0.0)
    if not believe_front:
        assert len(set(out["n_cells"].tolist())) == 1


# ----------------------------------------------------------------------------------------------------------------------
# 3. step 0 is sweep_ehvi with the grid cells; nothing leaks into later sweeps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [70, 530])
def test_step0_is_sweep_ehvi_and_nothing_leaks(eng, N):
    X, Y, args, Xs, pend, front, rp = commit(eng, N, 3, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    lo, hi = _lib.grid_cells(front, rp)
    np.testing.assert_array_equal(lo, pareto.hypercell_bounds(front, rp)[0])
    np.testing.assert_array_equal(hi, pareto.hypercell_bounds(front, rp)[1])
    before = eng.sweep_ehvi(lo, hi, k=3, return_values=True, return_moments=True)
    out = eng.sweep_believer_ehvi(front, rp, Q, return_values=True)
    assert out["best_val"][0] == before[0][0] and out["best_idx"][0] == before[1][0] and out["n_cells"][0] == len(lo)
    np.testing.assert_array_equal(out["ehvi"][0], before[2])
    np.testing.assert_array_equal(out["mse"][0], before[4])
    np.testing.assert_array_equal(out["best_mu"][0], before[3][out["best_idx"][0]])
    eng.sweep_believer_ehvi(front, rp, Q, pending=pend)
    after = eng.sweep_ehvi(lo, hi, k=3, return_values=True, return_moments=True)
    for b, a in zip(before, after):
        np.testing.assert_array_equal(b, a)
    # a single-target model on the same handle: its plain sweep and its believer, before and after an EHVI batch of another model
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 2.0)]

    def single():
        eng.set_train(X, Y[:, 0])
        eng.commit(args[0], args[1], args[2], args[3], True, 0.0)
        eng.upload_candidates(Xs)
        plugin = float(Y[:, 0].min())
        return eng.sweep(acq, plugin, True, return_values=True), eng.sweep_believer(acq, plugin, True, pending=pend[:1], return_values=True)

    s_before, b_before = single()
    eng.set_train(X, Y)
    eng.commit(*args)
    eng.upload_candidates(Xs)
    eng.sweep_believer_ehvi(front, rp, Q, pending=pend)
    s_after, b_after = single()
    for b, a in zip(s_before, s_after):
        np.testing.assert_array_equal(b, a)
    for k in b_before:
        np.testing.assert_array_equal(b_before[k], b_after[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------------
# 4. chunk invariance
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pend", [0, 2])
def test_chunk_invariance(eng, n_pend):
    """BOGP_CHUNK_MB=1 at N = 530 (544 padded rows: 192 candidates a chunk, 8 chunks of 1500): every output bit for bit the
    one-chunk run's."""
    X, Y, args, Xs, pend, front, rp = commit(eng, 530, 3, _lib.KERNEL_SE, True)
    eng.upload_candidates(Xs)
    whole = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:n_pend], return_values=True)
    old = os.environ.get("BOGP_CHUNK_MB")
    os.environ["BOGP_CHUNK_MB"] = "1"
    try:
        parts = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:n_pend], return_values=True)
        assert eng.last_timing()["n_chunks"] >= 4
    finally:
        if old is None:
            del os.environ["BOGP_CHUNK_MB"]
        else:
            os.environ["BOGP_CHUNK_MB"] = old
    for k in whole:
        np.testing.assert_array_equal(whole[k], parts[k], err_msg=k)
    t = eng.believer_ehvi_last()
    assert t["n_passes"] == n_pend + Q - 1 and t["ehvi_ms"] > 0 and t["update_ms"] > 0 and t["solve_ms"] > 0


# ----------------------------------------------------------------------------------------------------------------------
# 5. edges
# ----------------------------------------------------------------------------------------------------------------------
def test_eight_targets(eng):
    """m = 8 (BOGP_MAX_TARGETS).  A front of one point keeps the grid at 2^7 cells while the front is fixed; with the believed mean
    joining it, step 1 sees the grid of two points (up to 3^7 cells) -- over 32 candidates only, because the restatement's 2^m terms a
    cell cost host time."""
    rng = np.random.default_rng(8)
    N, m = 70, 8
    X = rng.uniform(-2, 2, size=(N, D))
    Y = np.sin(X @ rng.normal(size=(D, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    args = (_lib.KERNEL_MATERN52, _lib.MODE_NOISELESS, np.array([4.0, 3.2, 5.2]), 0.0, False, 0.0)
    eng.set_train(X, Y)
    eng.commit(*args)
    Xs = rng.uniform(-2.2, 2.2, size=(300, D))
    rp = Y.min(axis=0) - 0.5
    front = Y[:1]
    r = restatement(eng, X, args)
    for rows, believe_front in ((150, False), (32, True)):
        eng.upload_candidates(Xs[:rows])
        out = eng.sweep_believer_ehvi(front, rp, 2, believe_front=believe_front, return_values=True)
        ref = r.run(Xs[:rows], front, rp, 2, believe_front=believe_front)
        check_against(eng, out, ref, r, 0, Xs[:rows], *pareto.hypercell_bounds(front, rp))
        assert out["n_cells"][0] == 128 and (out["n_cells"][1] > 128) == believe_front


@pytest.mark.parametrize("Mx", [1, 63, 64, 65])
def test_few_candidates(eng, Mx):
    """Fewer rows than a workgroup serves, exactly one wavefront, one more; q = min(2, M) (M = 1: q = M, the only row)."""
    X, Y, args, Xs, pend, front, rp = commit(eng, 70, 2, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs[:Mx])
    r = restatement(eng, X, args)
    q = min(2, Mx)
    out = eng.sweep_believer_ehvi(front, rp, q, pending=pend[:1], return_values=True)
    ref = r.run(Xs[:Mx], front, rp, q, pending=pend[:1])
    check_against(eng, out, ref, r, 1, Xs[:Mx], *pareto.hypercell_bounds(front, rp))


def test_every_row_becomes_a_winner(eng):
    """q = M: the last step has one row left to take."""
    X, Y, args, Xs, pend, front, rp = commit(eng, 70, 2, _lib.KERNEL_MATERN52, True)
    eng.upload_candidates(Xs[:5])
    out = eng.sweep_believer_ehvi(front, rp, 5, return_values=True)
    assert sorted(out["best_idx"].tolist()) == [0, 1, 2, 3, 4]
    ref = restatement(eng, X, args).run(Xs[:5], front, rp, 5)
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])


def test_fronts(eng):
    """An empty initial front (one cell [ref, +inf)); a believed mean that is dominated (n_cells unchanged), one that dominates the
    whole front (n_cells drops to the grid of one point), one that is not above the reference point (n_cells unchanged)."""
    X, Y, args, Xs, pend, front, rp = commit(eng, 70, 2, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    r = restatement(eng, X, args)
    out = eng.sweep_believer_ehvi(None, rp, 3, return_values=True)
    ref = r.run(Xs, np.empty((0, 2)), rp, 3)
    assert out["n_cells"][0] == 1
    check_against(eng, out, ref, r, 0, Xs, *pareto.hypercell_bounds(np.empty((0, 2)), rp))
    mu_p = r.mean(pend[:1])[0]
    # dominated: a front point above the believed mean in both objectives
    dom = np.vstack([front, mu_p + 1.0])
    n0 = len(pareto.hypercell_bounds(dom, rp)[0])
    out = eng.sweep_believer_ehvi(dom, rp, 1, pending=pend[:1])
    assert out["n_cells"][0] == n0
    # dominating: every front point below the believed mean
    low = mu_p - np.array([[0.1, 0.3], [0.2, 0.2], [0.3, 0.1]])
    assert np.all(low > rp) and len(pareto.pareto_front(low, rp)) == 3
    out = eng.sweep_believer_ehvi(low, rp, 1, pending=pend[:1])
    assert out["n_cells"][0] == 2 < len(pareto.hypercell_bounds(low, rp)[0])
    # not above the reference point: the mean does not join the front
    rp_hi = np.array([mu_p[0] + 0.5, rp[1]])
    n0 = len(pareto.hypercell_bounds(front, rp_hi)[0])
    out = eng.sweep_believer_ehvi(front, rp_hi, 1, pending=pend[:1], return_values=True)
    assert out["n_cells"][0] == n0
    ref = r.run(Xs, front, rp_hi, 1, pending=pend[:1])
    np.testing.assert_array_equal(out["best_idx"], ref["best_idx"])


@pytest.mark.parametrize("N", [70, 530])
def test_pivot_guard(eng, N):
    """A pending point equal to a training point of a noiseless model, and a pending point given twice, are already determined:
    pivot <= 1e-12, c = 0, and with a fixed front every output is the one of the run without them."""
    X, Y, args, Xs, pend, front, rp = commit(eng, N, 2, _lib.KERNEL_MATERN52, False)
    eng.upload_candidates(Xs)
    base = eng.sweep_believer_ehvi(front, rp, 3, pending=pend[:1], believe_front=False, return_values=True)
    trn = eng.sweep_believer_ehvi(front, rp, 3, pending=np.vstack([X[3], pend[:1]]), believe_front=False, return_values=True)
    assert trn["pivots"][0] <= 1e-12
    np.testing.assert_array_equal(trn["pivots"][1:], base["pivots"])
    for k in ("best_val", "best_idx", "best_x", "best_mu", "n_cells", "ehvi", "mse"):
        np.testing.assert_array_equal(trn[k], base[k], err_msg=k)
    rep = eng.sweep_believer_ehvi(front, rp, 3, pending=np.vstack([pend[:1], pend[:1]]), believe_front=True, return_values=True)
    base_f = eng.sweep_believer_ehvi(front, rp, 3, pending=pend[:1], believe_front=True, return_values=True)
    assert rep["pivots"][1] <= 1e-12
    np.testing.assert_array_equal(np.delete(rep["pivots"], 1), base_f["pivots"])
    for k in ("best_val", "best_idx", "best_x", "best_mu", "n_cells", "ehvi", "mse"):  # (the repeated mean is identical to the first: it does not join the front)
        np.testing.assert_array_equal(rep[k], base_f[k], err_msg=k)
    # the last pending point guarded: step 0 is then evaluated by a criterion-only pass
    last = eng.sweep_believer_ehvi(front, rp, 3, pending=np.vstack([pend[:1], X[5]]), believe_front=False, return_values=True)
    assert last["pivots"][1] <= 1e-12
    for k in ("best_val", "best_idx", "ehvi", "mse"):
        np.testing.assert_array_equal(last[k], base[k], err_msg=k)


def test_candidate_sources(eng):
    X, Y, args, _, pend, front, rp = commit(eng, 530, 2, _lib.KERNEL_MATERN52, True)
    eng.generate_candidates(np.full(D, -2.2), np.full(D, 2.2), M, seed=17)
    gen = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:1], return_values=True)
    Xs = eng.read_candidates(np.arange(M))
    eng.upload_candidates(Xs)
    up = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:1], return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy = eng.sweep_believer_ehvi(front, rp, Q, pending=pend[:1], return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy0 = eng.sweep_believer_ehvi(front, rp, Q, return_values=True)
    eng.upload_candidates(Xs)
    up0 = eng.sweep_believer_ehvi(front, rp, Q, return_values=True)
    for k in up:
        np.testing.assert_array_equal(gen[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy[k], up[k], err_msg=k)
        np.testing.assert_array_equal(lazy0[k], up0[k], err_msg=k)
    np.testing.assert_array_equal(up["best_x"], Xs[up["best_idx"]])


# ----------------------------------------------------------------------------------------------------------------------
# 6. error returns
# ----------------------------------------------------------------------------------------------------------------------
def _call(eng, m=2, q=2, ref=(-9.0, -9.0), front=None, n_front=0, pending=None, n_pend=0, best=True, idx=True):
    lib = _lib.load()
    bv, bi = np.empty(max(q, 1)), np.empty(max(q, 1), dtype=np.int64)
    ref_ = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64)
    fr = None if front is None else np.ascontiguousarray(front, dtype=np.float64)
    pend = None if pending is None else np.ascontiguousarray(pending, dtype=np.float64)
    rc = lib.bogp_sweep_believer_ehvi(eng._h, m, q, _lib._ptr(ref_), _lib._ptr(fr), n_front, 1, _lib._ptr(pend), n_pend,
                                      _lib._ptr(bv) if best else None, bi.ctypes.data_as(C.POINTER(C.c_int64)) if idx else None,
                                      None, None, None, None, None, None)  # fmt: skip
    return rc, lib.bogp_last_error(eng._h).decode()


def staircase(n, m):
    """n mutually non-dominated points with distinct coordinates in every objective, all above 0: the first m - 1 rise, the last falls"""
    t = np.arange(1, n + 1, dtype=float)
    return np.column_stack([t] * (m - 1) + [n + 1 - t])


def test_error_returns():
    """Every error return of bogp_sweep_believer_ehvi but one: a communicator of more than one rank cannot be built on one device
    (its refusal is a comparison of the handle's world size, exercised by the Python layer's own refusal on the host).  After the
    cell-limit error a valid call on the same handle succeeds."""
    lib = _lib.load()
    assert lib.bogp_sweep_believer_ehvi(None, 2, 1, None, None, 0, 1, None, 0, None, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, Y, args, Xs, pend, front, rp = problem(70, 2, _lib.KERNEL_SE, False)
        e.set_train(X, Y)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no committed model" in msg
        e.commit(*args)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no candidates" in msg
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK
        assert _call(e, front=front, n_front=len(front), pending=pend, n_pend=2)[0] == _lib.OK
        rc, msg = _call(e, m=3, ref=(-9.0, -9.0, -9.0))
        assert rc == _lib.ERR_INVALID and "2 target" in msg
        assert _call(e, q=0)[0] == _lib.ERR_INVALID
        e.upload_candidates(Xs[:1])  # more proposals than candidates
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "proposals from 1 candidates" in msg
        e.upload_candidates(Xs)
        rc, msg = _call(e, q=31, pending=pend, n_pend=2)
        assert rc == _lib.ERR_INVALID and "<= 32" in msg
        assert _call(e, ref=None)[0] == _lib.ERR_INVALID
        assert _call(e, best=False)[0] == _lib.ERR_INVALID and _call(e, idx=False)[0] == _lib.ERR_INVALID
        assert _call(e, front=None, n_front=3)[0] == _lib.ERR_INVALID and _call(e, n_front=-1)[0] == _lib.ERR_INVALID
        assert _call(e, pending=None, n_pend=1)[0] == _lib.ERR_INVALID and _call(e, n_pend=-1)[0] == _lib.ERR_INVALID
        bad = pend.copy()
        bad[1, 2] = np.nan
        rc, msg = _call(e, pending=bad, n_pend=2)
        assert rc == _lib.ERR_INVALID and "not finite" in msg
        bad = front.copy()
        bad[0, 1] = np.inf
        rc, msg = _call(e, front=bad, n_front=len(bad))
        assert rc == _lib.ERR_INVALID and "not finite" in msg
        rc, msg = _call(e, ref=(0.0, np.nan))
        assert rc == _lib.ERR_INVALID and "not finite" in msg
        with pytest.raises(_lib.BogpError) as ei:
            e.sweep_believer_ehvi(front, rp, 33)
        assert ei.value.code == _lib.ERR_INVALID
        # a lift on the handle
        e.set_lift(np.eye(D), np.zeros(D), None, -np.ones(D), np.ones(D))
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "lift" in msg
        e.clear_lift()
        assert _call(e)[0] == _lib.OK
        # one target; a polynomial trend basis
        e.set_train(X, Y[:, 0])
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0)
        e.upload_candidates(Xs)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "1 target" in msg
        assert _call(e, m=1, ref=(-9.0,))[0] == _lib.ERR_INVALID
        e.commit(args[0], args[1], args[2], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "constant trend" in msg
        # the cell limit: m = 4 and 41 mutually non-dominated points with distinct coordinates give 42^3 = 74 088 > 65 536 cells
        e.set_train(X, np.column_stack([Y, Y[:, 0] + Y[:, 1], Y[:, 0] - Y[:, 1]]))
        e.commit(*args)
        e.upload_candidates(Xs)
        big = staircase(41, 4)
        assert len(pareto.pareto_front(big, np.zeros(4))) == 41
        rc, msg = _call(e, m=4, ref=np.zeros(4), front=big, n_front=41)
        assert rc == _lib.ERR_INVALID and "step 0" in msg and "74088 cells" in msg, msg
        assert _call(e, m=4, ref=np.full(4, -50.0), front=big[:5], n_front=5)[0] == _lib.OK
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
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "forest" in msg
    finally:
        e.close()
