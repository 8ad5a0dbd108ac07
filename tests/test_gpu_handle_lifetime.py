"""What a handle holds on the device goes back when it is closed (`bogp_debug_live`: live device + mapped pinned allocations, their
bytes, live events of the process, counted by the three owning types of csrc/bogp_handle.h).  Every count is compared with the one
read before the test created anything -- not with zero: engines of other modules may be alive -- and exactly, since they are integers.
Shapes are the smallest that reach each buffer family; the re-used buffers must also return the bits of a fresh engine."""
import gc

import numpy as np
import pytest

from bogp import _lib, thompson

pytestmark = pytest.mark.gpu

KERNEL, MODE = _lib.KERNEL_MATERN52, _lib.MODE_NOISELESS
EI, ACQ2 = [(_lib.ACQ_EI, 0.0)], [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 2.0)]


def live():
    gc.collect()  # an engine another test dropped without close() goes now, not in the middle of a comparison
    return _lib.debug_live()


def problem(N, d=3, m=1, seed=0):
    """(X, y (N, m), theta): the length scale at which nearest neighbours correlate at about exp(-1), so that R stays well conditioned;
    y on a scale of 5, where every likelihood below is negative (the reference rejects a positive one: BOGP_ERR_LLF_POSITIVE)."""
    rng = np.random.default_rng(100 * N + seed)
    X = rng.uniform(-2, 2, size=(N, d))
    Y = 5.0 * (np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.1 * rng.normal(size=(N, m)))
    nn = 4.0 / N ** (1.0 / d)
    return X, Y, np.full(d, 1.0 / (d * nn * nn))


def candidates(M, d=3, seed=7):
    return np.random.default_rng(seed).uniform(-2.2, 2.2, size=(M, d))


def tiny_forest(m=1):
    """Two trees of three nodes over two columns, m values a node."""
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])
    return dict(d=2, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=v if m == 1 else np.stack([v + k for k in range(m)], axis=1))  # fmt: skip


def test_every_buffer_family_returns_to_the_baseline():
    base = live()
    eng = _lib.Engine(0)
    # one target, N = 40: likelihood, commit, the sweeps, the one-point family and the polish
    X, y, theta = problem(40)
    Xs = candidates(300)
    eng.set_train(X, y)
    assert np.isfinite(eng.nll(KERNEL, MODE, theta, 0.0, True, 0.0, eval_grad=True)[0])
    eng.commit(KERNEL, MODE, theta, 0.0, True, 0.0)
    eng.upload_candidates(Xs)
    plugin = float(y.min())
    best, idx = eng.sweep(ACQ2, plugin, True)
    assert np.all(np.isfinite(best)) and np.all((idx >= 0) & (idx < 300))
    eng.sweep_topk(ACQ2, plugin, True, k=4)
    eng.predict()
    eng.gradient(Xs[0])
    eng.point_eval_batch(Xs[:3], ACQ2, plugin, True)
    eng.polish(Xs[:3], np.full(3, -2.2), np.full(3, 2.2), EI[0], plugin, True, max_evals=5)
    out = eng.sweep_believer(ACQ2 + EI, plugin, True, pending=Xs[5:6])
    assert len(set(out["best_idx"].tolist())) == 3
    st = thompson.dense_state(X, y.ravel(), theta, KERNEL, True)
    eng.sweep_thompson(thompson.draw(st, 2, 16, seed=1))
    # a lift of the three reduced coordinates into five
    A = np.linalg.qr(np.random.default_rng(3).normal(size=(5, 3)))[0].T
    eng.set_lift(A, np.zeros(5), None, np.full(5, -1.5), np.full(5, 1.5))
    assert 0 < eng.lift_sweep_topk(EI, plugin, True, k=2)[2] < 300  # some rows feasible, some not: filter, compaction and merge all run
    eng.clear_lift()
    # batched likelihood: the one-launch path, the elimination workspaces (N = 200), helper handles (N = 192 under a linear trend)
    pars = np.vstack([theta, theta * 1.3, theta * 0.7])
    assert np.all(eng.nll_batch(KERNEL, MODE, pars, 0.0, True, 0.0, eval_grad=True)[2] == 0)
    X2, y2, th2 = problem(200)
    eng.set_train(X2, y2)
    assert np.all(eng.nll_batch(KERNEL, MODE, np.vstack([th2, th2 * 1.3, th2 * 0.7]), 0.0, True, 0.0, eval_grad=True)[2] == 0)
    X3, y3, th3 = problem(192)
    eng.set_train(X3, y3)
    pars3 = np.vstack([th3, th3 * 1.3, th3 * 0.7])
    assert np.all(eng.nll_batch(KERNEL, MODE, pars3, 0.0, True, 0.0, eval_grad=True, trend=_lib.TREND_LINEAR)[2] == 0)
    eng.commit(KERNEL, MODE, th3, 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    best, idx = eng.sweep(ACQ2, float(y3.min()), True)  # (the candidates stay: same width)
    assert np.all(np.isfinite(best))
    # two targets: EHVI sweep, believer batches under EHVI, the one-point EHVI
    X4, Y4, th4 = problem(40, m=2)
    eng.set_train(X4, Y4)
    eng.commit(KERNEL, MODE, th4, 0.0, False, 0.0)
    ref = Y4.max(axis=0) + 0.1
    front = Y4[np.argsort(Y4[:, 0])[:1]]
    lower, upper = _lib.grid_cells(front, ref)
    eng.sweep_ehvi(lower, upper, k=2)
    eng.sweep_believer_ehvi(front, ref, 2)
    assert np.all(np.isfinite(eng.point_eval_ehvi(Xs[:2], lower, upper)[0]))
    eng.upload_candidates(candidates(500, seed=8), lazy=True)
    eng.predict()
    # a second engine: a forest and its sweep, a two-output forest and its EHVI sweep
    fe = _lib.Engine(0)
    fe.forest_set(**tiny_forest())
    fe.upload_candidates(np.random.default_rng(2).uniform(0, 1, size=(300, 2)))
    fe.forest_sweep_topk(ACQ2, 1.0, True, k=2)
    fe.forest_set_multi(m=2, **tiny_forest(2))
    fl, fu = _lib.grid_cells(np.array([[2.0, 3.0]]), np.array([6.0, 7.0]))
    fe.forest_sweep_ehvi(fl, fu, k=2)
    alive = live()
    assert all(a > b for a, b in zip(alive, base)), (alive, base)
    eng.close()
    fe.close()
    assert live() == base


def test_training_buffers_grow_are_reused_and_return_the_fresh_bits():
    base = live()
    X, y, theta = problem(60)
    Xs = candidates(300)
    plugin = float(y.min())

    def at60(e):
        e.set_train(X, y)
        llf, g = e.nll(KERNEL, MODE, theta, 0.0, True, 0.0, eval_grad=True)
        e.commit(KERNEL, MODE, theta, 0.0, True, 0.0)
        e.upload_candidates(Xs)
        return (llf, g) + e.sweep(ACQ2, plugin, True, return_values=True)

    eng = _lib.Engine(0)
    Xa, ya, _ = problem(40)
    eng.set_train(Xa, ya)
    bytes40 = live()[1]
    Xb, yb, _ = problem(70)
    eng.set_train(Xb, yb)
    bytes70 = live()[1]
    assert bytes70 > bytes40  # re-allocated
    got = at60(eng)
    fresh = _lib.Engine(0)
    want = at60(fresh)
    fresh.close()
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        np.testing.assert_array_equal(a, b)
    eng.close()
    assert live() == base


def test_ensure_neither_shrinks_nor_copies():
    base = live()
    X, y, theta = problem(40)
    eng = _lib.Engine(0)
    eng.set_train(X, y)
    eng.commit(KERNEL, MODE, theta, 0.0, True, 0.0)
    small, large = candidates(300), candidates(1000, seed=9)
    plugin = float(y.min())

    def sweep(Xs):
        eng.upload_candidates(Xs)
        return eng.sweep(ACQ2, plugin, True, return_values=True), live()

    first, n1 = sweep(small)
    _, n2 = sweep(large)
    third, n3 = sweep(small)
    for a, b in zip(first, third):
        np.testing.assert_array_equal(a, b)
    assert n2[1] > n1[1] and n3 == n2  # grown for 1000 rows, kept for 300
    eng.close()
    assert live() == base
