"""The lifted sweep on the device (`bogp_lift_set` / `bogp_lift_sweep_topk`, kernels_lift.hip): the golden G41 recorded from the
reference's own PCA-BO wrapper; bit-identity with the plain sweep (identity lift; every feasible row against the feasible rows
swept on their own; chunk size; repeat runs); both sweep paths, several criteria, no / all rows feasible, ragged M, ties,
generated and lazily uploaded candidates; the error returns; the plain sweep untouched by a lift that was set and cleared."""
import numpy as np
import pytest

from conftest import load_golden

import bogp
from bogp import _lib, optim
from support.lift_engine import rank_rows

pytestmark = pytest.mark.gpu

Q4 = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_EPSILON_PI, 0.05), (_lib.ACQ_UCB, 1.5), (_lib.ACQ_MGFI, 2.0)]


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _model(eng, N, r, seed=0):
    """A model of the reduced space committed at fixed hyper-parameters (Matern-3/2, ordinary kriging, noisy mode with the
    nugget 1e-6: what PCABO.update_model builds); returns the plugin (min y)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, size=(N, r))
    y = np.sum((np.arange(1, r + 1) * X) ** 2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    eng.set_train(X, y)
    eng.commit(_lib.KERNEL_MATERN32, _lib.MODE_NOISY, np.r_[np.full(r, 2.0 / r), 0.9], 1e-6, True, 0.0)
    return float(y.min())


def _lift(r, D, seed=1, half=0.45):
    """r orthonormal rows in D dimensions, a small offset, the box [-half, half]^D: of uniform rows of [-1, 1]^r a few per cent
    to a few ten per cent are feasible"""
    rng = np.random.default_rng(seed)
    A = np.linalg.qr(rng.normal(size=(D, r)))[0].T
    return bogp.Lift(A, 0.02 * rng.normal(size=D), 0.02 * rng.normal(size=D), np.full(D, -half), np.full(D, half))


def _set(eng, lift):
    eng.set_lift(lift.A, lift.mean, lift.center, lift.lo, lift.hi)


def _check_ranking(best, idx, vals):
    """best / idx are exactly the ranking of the device's own q x M values under bogp_sweep_topk's rules"""
    for c in range(len(vals)):
        rv, ri = rank_rows(vals[c], best.shape[1])
        assert np.array_equal(idx[c], ri), (c, idx[c], ri)
        assert np.array_equal(best[c], rv, equal_nan=True)


# ----------------------------------------------------------------------------------------------------------------------
# 4. the golden: the reference's own wrapper, row by row
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", ["d5_", "d20_"])
def test_golden_pcabo_states(eng, prefix):
    g = load_golden("G41_pcabo")
    s = {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}
    lift = bogp.Lift(s["A"], s["mean"], s["center"], s["bounds"][:, 0], s["bounds"][:, 1])
    width = float(np.max(lift.hi - lift.lo))
    eng.set_train(s["X"], s["y"])
    eng.commit(int(s["kernel"]), int(s["mode"]), s["par"], float(s["noise_var"]), bool(s["estimate_trend"]), 0.0)
    eng.upload_candidates(s["Z"])
    _set(eng, lift)
    try:
        best, idx, nf, vals, pen = eng.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], float(s["plugin"]), True, k=16, return_values=True,
                                                       return_penalty=True)  # fmt: skip
    finally:
        eng.clear_lift()
    feas = s["penalty"] == 0
    print("%s M_f = %d of %d; max |penalty - ref| = %.3e; max rel EI error on feasible rows = %.3e" % (
        prefix, nf, len(feas), np.abs(pen - s["penalty"]).max(),
        np.max(np.abs(vals[0][feas] - s["value"][feas]) / np.maximum(np.abs(s["value"][feas]), 1e-300))))  # fmt: skip
    np.testing.assert_allclose(pen, s["penalty"], rtol=1e-6, atol=1e-12 * width)  # ledger T13
    assert np.array_equal(pen == 0, feas) and nf == int(feas.sum())
    assert np.array_equal(pen, lift.penalty(s["Z"]))  # the NumPy restatement follows the kernel operation by operation
    np.testing.assert_allclose(vals[0][feas], s["value"][feas], rtol=1e-6, atol=1e-300)  # EI on every feasible row
    assert np.array_equal(vals[0][~feas], pen[~feas])
    _check_ranking(best, idx, vals)
    assert int(idx[0, 0]) == int(s["argmax"])
    for rank, (mine, ref) in enumerate(zip(idx[0], s["top16"])):  # exact, or T10: the reference's own two values tie to 1e-9
        assert mine == ref or abs(s["value"][mine] - s["value"][ref]) <= 1e-9 * abs(s["value"][ref]), rank


# ----------------------------------------------------------------------------------------------------------------------
# 5. bit-identity with the plain sweep
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [300, 1024])  # the one-launch path (N <= 512) and the chunked path
@pytest.mark.parametrize("acq", [[(_lib.ACQ_EI, 0.0)], Q4], ids=["q1", "q4"])
def test_identity_lift_is_the_plain_sweep(eng, N, acq):
    r, M = 4, 5003  # (M is no multiple of 64 or 256)
    plugin = _model(eng, N, r)
    Z = np.random.default_rng(7).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    tb, ti = eng.sweep_topk(acq, plugin, True, k=16)
    sb, si, sv = eng.sweep(acq, plugin, True, return_values=True)
    eng.set_lift(np.eye(r), np.zeros(r), None, np.full(r, -1e6), np.full(r, 1e6))
    try:
        best, idx, nf, vals, pen = eng.lift_sweep_topk(acq, plugin, True, k=16, return_values=True, return_penalty=True)
    finally:
        eng.clear_lift()
    assert nf == M and np.all(pen == 0)
    assert np.array_equal(vals, sv) and np.array_equal(best, tb) and np.array_equal(idx, ti)
    assert np.array_equal(best[:, 0], sb) and np.array_equal(idx[:, 0], si)


@pytest.mark.parametrize("N", [300, 1024])
@pytest.mark.parametrize("acq", [[(_lib.ACQ_EI, 0.0)], Q4], ids=["q1", "q4"])
def test_feasible_rows_get_the_plain_sweeps_bits(eng, N, acq):
    r, D, M = 3, 20, 20011
    plugin = _model(eng, N, r, seed=3)
    lift = _lift(r, D)
    Z = np.random.default_rng(8).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    _set(eng, lift)
    try:
        best, idx, nf, vals, pen = eng.lift_sweep_topk(acq, plugin, True, k=16, return_values=True, return_penalty=True)
        again = eng.lift_sweep_topk(acq, plugin, True, k=16, return_values=True, return_penalty=True)
    finally:
        eng.clear_lift()
    feas = pen == 0
    print("N = %d: M_f = %d of %d" % (N, nf, M))
    assert np.array_equal(pen, lift.penalty(Z)) and nf == int(feas.sum()) and 100 < nf < M // 2
    for a, b in zip((best, idx, nf, vals, pen), again):  # two consecutive runs
        assert np.array_equal(a, b)
    eng.upload_candidates(Z[feas])  # the feasible rows on their own, through the plain sweep
    sv = eng.sweep(acq, plugin, True, return_values=True)[2]
    assert np.array_equal(vals[:, feas], sv)
    assert np.array_equal(vals[:, ~feas], np.tile(pen[~feas], (len(acq), 1)))
    _check_ranking(best, idx, vals)


def test_chunk_size_does_not_change_a_bit(eng, monkeypatch):
    r, D, M, N = 3, 20, 60007, 1024
    plugin = _model(eng, N, r, seed=4)
    lift = _lift(r, D, half=0.3)  # (about a tenth of the rows feasible: some fifty chunks of 128)
    Z = np.random.default_rng(9).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    _set(eng, lift)
    try:
        ref = eng.lift_sweep_topk(Q4, plugin, True, k=16, return_values=True, return_penalty=True)
        chunks_default = eng.last_timing()["n_chunks"]
        monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 rows a chunk at N = 1024
        small = eng.lift_sweep_topk(Q4, plugin, True, k=16, return_values=True, return_penalty=True)
        chunks_small = eng.last_timing()["n_chunks"]
    finally:
        eng.clear_lift()
    assert chunks_default == 1 and chunks_small == (ref[2] + 127) // 128 and ref[2] > 1000
    for a, b in zip(ref, small):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# 6. edges of the filter
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 63, 257, 4099])
def test_no_feasible_row_means_the_least_penalised_wins(eng, M):
    r, D = 3, 7
    plugin = _model(eng, 120, r, seed=5)
    lift = _lift(r, D)
    lift = bogp.Lift(lift.A, lift.mean + 10.0, lift.center, lift.lo, lift.hi)  # the whole reduced box maps outside
    Z = np.random.default_rng(10).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    _set(eng, lift)
    try:
        best, idx, nf, vals, pen = eng.lift_sweep_topk(Q4, plugin, True, k=4, return_values=True, return_penalty=True)
    finally:
        eng.clear_lift()
    assert nf == 0 and np.all(pen < 0) and np.array_equal(pen, lift.penalty(Z))
    assert eng.last_timing()["n_chunks"] == 0 and eng.lift_last()["n_feasible"] == 0
    assert np.array_equal(vals, np.tile(pen, (4, 1)))
    _check_ranking(best, idx, vals)
    assert np.all(idx[:, 0] == int(np.argmax(pen)))
    if M < 4:
        assert np.all(idx[:, M:] == -1) and np.all(np.isneginf(best[:, M:]))


@pytest.mark.parametrize("M", [1, 31, 33, 255, 256, 1025])
def test_ragged_sizes_and_few_survivors(eng, M):
    """M_f from 0 up through the small-batch path (<= 32 rows), on M that is no multiple of the workgroup"""
    r, D = 3, 12
    plugin = _model(eng, 200, r, seed=6)
    lift = _lift(r, D, half=0.3)  # (0, 2, 2, 18, 14, 61 feasible rows)
    Z = np.random.default_rng(M).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    _set(eng, lift)
    try:
        best, idx, nf, vals, pen = eng.lift_sweep_topk(Q4, plugin, True, k=8, return_values=True, return_penalty=True)
    finally:
        eng.clear_lift()
    feas = pen == 0
    assert np.array_equal(pen, lift.penalty(Z)) and nf == int(feas.sum())
    if nf:
        eng.upload_candidates(Z[feas])
        assert np.array_equal(vals[:, feas], eng.sweep(Q4, plugin, True, return_values=True)[2])
    assert np.array_equal(vals[:, ~feas], np.tile(pen[~feas], (4, 1)))
    _check_ranking(best, idx, vals)


def test_ties_go_to_the_lower_index(eng):
    r, D, M = 3, 12, 3001
    plugin = _model(eng, 200, r, seed=6)
    lift = _lift(r, D, half=0.5)
    Z = np.random.default_rng(12).uniform(-1, 1, size=(M, r))
    Z2 = np.vstack([Z, Z])  # every row twice: rows i and i + M tie
    eng.upload_candidates(Z2)
    _set(eng, lift)
    try:
        best, idx, nf, vals = eng.lift_sweep_topk(Q4, plugin, True, k=16, return_values=True)
    finally:
        eng.clear_lift()
    assert np.array_equal(vals[:, :M], vals[:, M:]) and nf % 2 == 0 and nf > 0
    _check_ranking(best, idx, vals)
    assert np.all(idx[:, 0::2] < M) and np.array_equal(idx[:, 1::2], idx[:, 0::2] + M)
    assert np.array_equal(best[:, 0::2], best[:, 1::2])


class _Model:
    """what optim's sweeps need of a fitted surrogate"""

    _committed_par = np.ones(1)

    def __init__(self, engine):
        self.engine = engine

    def _check_X(self, X):
        return np.ascontiguousarray(X, dtype=float)


def _ei(model, plugin):
    ei = bogp.acquisition.EI.__new__(bogp.acquisition.EI)
    ei._model, ei.minimize, ei._plugin = model, True, plugin
    return ei


@pytest.mark.parametrize("method", ["uniform", "LHS", "sobol"])
def test_generated_candidates_equal_the_host_path(eng, method):
    r, D, M = 3, 20, 30001
    plugin = _model(eng, 300, r, seed=3)
    lift = _lift(r, D)
    ei = _ei(_Model(eng), plugin)
    box = optim.Box([(-1, 1)] * r)
    gb, gi, gx = optim.sweep_generated([ei], box, M, seed=77, method=method, lift=lift)
    Zg = eng.read_candidates(np.arange(M))
    assert np.array_equal(gx[0], Zg[gi[0]]) and np.all(np.abs(Zg) <= 1)
    tv, ti, tx = optim.sweep_topk_generated([ei], box, M, 8, seed=77, method=method, lift=lift)
    hb, hi, hx = optim.sweep_argmax([ei], Zg, lift=lift)  # the same rows through the (lazy) host upload
    hv, hti, htx = optim.sweep_topk([ei], Zg, 8, lift=lift)
    assert np.array_equal(gb, hb) and np.array_equal(gi, hi) and np.array_equal(gx, hx)
    assert np.array_equal(tv, hv) and np.array_equal(ti, hti) and np.array_equal(tx, htx)
    assert tv[0, 0] == gb[0] and ti[0, 0] == gi[0]
    assert np.all(lift.penalty(gx) == 0) and gb[0] >= 0  # a feasible row wins: EI >= 0 > any penalty
    # the lift is off the engine again: a plain sweep returns every row's criterion value, no row's penalty
    pen = lift.penalty(Zg)
    plain = eng.sweep([(_lib.ACQ_EI, 0.0)], plugin, True, return_values=True)[2][0]
    assert 0 < int((pen != 0).sum()) < M and not np.any(plain[pen != 0] == pen[pen != 0])


def test_lazy_upload_is_finished_first(eng):
    r, D, M = 3, 20, 700001  # 16.8 MB of candidates: a lazy upload copies only the first 8 MB at once
    plugin = _model(eng, 300, r, seed=3)
    lift = _lift(r, D)
    Z = np.random.default_rng(13).uniform(-1, 1, size=(M, r))
    _set(eng, lift)
    try:
        eng.upload_candidates(Z)
        ref = eng.lift_sweep_topk(Q4, plugin, True, k=16, return_penalty=True)
        eng.upload_candidates(Z, lazy=True)
        lazy = eng.lift_sweep_topk(Q4, plugin, True, k=16, return_penalty=True)
        info = eng.lift_last()
    finally:
        eng.clear_lift()
    for a, b in zip(ref, lazy):
        assert np.array_equal(a, b)
    assert np.array_equal(ref[3], lift.penalty(Z)) and info["n_feasible"] == ref[2] and info["filter_ms"] > 0 and info["merge_ms"] > 0
    assert np.array_equal(eng.read_candidates(np.array([0, M - 1])), Z[[0, M - 1]])  # the handle's candidates are the M rows again


# ----------------------------------------------------------------------------------------------------------------------
# 7. error returns; the plain sweep before bogp_lift_set and after bogp_lift_clear
# ----------------------------------------------------------------------------------------------------------------------
def _code(call):
    with pytest.raises(_lib.BogpError) as e:
        call()
    return e.value.code, str(e.value)


def test_error_returns():
    e = _lib.Engine(0)
    try:
        lib, h = e._lib, e._h
        one = np.ones(4)
        assert lib.bogp_lift_set(None, 2, None, None, None, None, None) == _lib.ERR_INVALID
        assert lib.bogp_lift_clear(None) == _lib.ERR_INVALID and lib.bogp_lift_last(None, None, None, None) == _lib.ERR_INVALID
        assert lib.bogp_lift_sweep_topk(None, 1, None, None, 0.0, 1, 1, None, None, None, None, None) == _lib.ERR_INVALID
        p = lambda a: a.ctypes.data_as(_lib._dp)  # noqa: E731
        assert lib.bogp_lift_set(h, 2, p(one), p(one), None, p(one), p(one)) == _lib.ERR_INVALID  # no training set: r is unknown
        assert b"bogp_set_train" in lib.bogp_last_error(h)
        plugin = _model(e, 50, 2)
        code, msg = _code(lambda: e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, 1))
        assert code == _lib.ERR_INVALID and "bogp_lift_set" in msg  # no lift
        I2, z2 = np.eye(2), np.zeros(2)
        assert lib.bogp_lift_set(h, 2, None, p(z2), None, p(z2), p(z2)) == _lib.ERR_INVALID
        assert lib.bogp_lift_set(h, 0, p(I2), p(z2), None, p(z2), p(z2)) == _lib.ERR_INVALID
        assert _code(lambda: e.set_lift(np.array([[np.nan, 0], [0, 1.0]]), z2, None, -one[:2], one[:2]))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.set_lift(I2, np.array([np.inf, 0]), None, -one[:2], one[:2]))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.set_lift(I2, z2, np.array([0, np.nan]), -one[:2], one[:2]))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.set_lift(I2, z2, None, one[:2], -one[:2]))[0] == _lib.ERR_INVALID  # lo > hi
        assert _code(lambda: e.set_lift(I2, z2, None, np.array([np.nan, 0]), one[:2]))[0] == _lib.ERR_INVALID
        code, msg = _code(lambda: e.set_lift(np.zeros((2, 321)), np.zeros(321), None, -np.ones(321), np.ones(321)))
        assert code == _lib.ERR_UNSUPPORTED and "BOGP_MAX_DIM" in msg
        e.set_lift(I2, z2, None, np.array([-np.inf, -1.0]), np.array([np.inf, 1.0]))  # infinite bounds are a box too
        code, msg = _code(lambda: e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, 1))
        assert code == _lib.ERR_INVALID and "no candidates" in msg
        e.upload_candidates(np.random.default_rng(0).uniform(-2, 2, size=(100, 2)))
        assert _code(lambda: e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, 0))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, _lib.MAX_TOPK + 1))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.lift_sweep_topk([(7, 0.0)], plugin, True, 1))[0] == _lib.ERR_INVALID
        assert _code(lambda: e.lift_sweep_topk([(_lib.ACQ_UCB, -1.0)], plugin, True, 1))[0] == _lib.ERR_INVALID
        best, idx, nf, pen = e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, 2, return_penalty=True)
        assert 0 < nf < 100 and np.array_equal(pen == 0, np.abs(e.read_candidates(np.arange(100))[:, 1]) <= 1)
        # a training set of another d: the lift must be set again
        _model(e, 50, 3)
        e.upload_candidates(np.zeros((10, 3)))
        code, msg = _code(lambda: e.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], plugin, True, 1))
        assert code == _lib.ERR_INVALID and "bogp_lift_set again" in msg
        e.clear_lift()
        # the staging limits: r > BOGP_LIFT_MAX_R, r D > BOGP_LIFT_MAX_RD
        rng = np.random.default_rng(1)
        e.set_train(rng.uniform(size=(80, 65)), rng.uniform(size=(80, 1)))
        code, msg = _code(lambda: e.set_lift(np.zeros((65, 65)), np.zeros(65), None, -np.ones(65), np.ones(65)))
        assert code == _lib.ERR_UNSUPPORTED and "BOGP_LIFT_MAX_R" in msg
        e.set_train(rng.uniform(size=(80, 40)), rng.uniform(size=(80, 1)))
        code, msg = _code(lambda: e.set_lift(np.zeros((40, 320)), np.zeros(320), None, -np.ones(320), np.ones(320)))
        assert code == _lib.ERR_UNSUPPORTED and "BOGP_LIFT_MAX_RD" in msg
        e.set_lift(np.zeros((40, 102)), np.zeros(102), None, -np.ones(102), np.ones(102))  # 4080 <= 4096
        e.clear_lift()
    finally:
        e.close()


def test_lift_with_ehvi_and_forest_is_refused():
    e = _lib.Engine(0)
    try:
        rng = np.random.default_rng(2)
        X = rng.uniform(-1, 1, size=(40, 2))
        e.set_train(X, np.c_[np.sin(X[:, 0]), np.cos(X[:, 1])])
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[0.15, 0.15, 0.9], 0.0, False, 0.0)  # (as tests/test_gpu_ehvi.py commits)
        e.upload_candidates(rng.uniform(-1, 1, size=(64, 2)))
        cells = (np.array([[-2.0, -2.0]]), np.array([[np.inf, np.inf]]))
        before = e.sweep_ehvi(*cells, k=2, return_values=True)
        e.set_lift(np.eye(2), np.zeros(2), None, -np.ones(2), np.ones(2))
        code, msg = _code(lambda: e.sweep_ehvi(*cells, k=2))
        assert code == _lib.ERR_UNSUPPORTED and "bogp_lift_clear" in msg
        e.clear_lift()
        for a, b in zip(before, e.sweep_ehvi(*cells, k=2, return_values=True)):
            assert np.array_equal(a, b)
    finally:
        e.close()
    f = _lib.Engine(0)
    try:  # two one-leaf trees over two columns: a forest handle
        f.forest_set(2, np.array([0, 1, 2]), np.array([-2, -2]), np.zeros(2), np.array([-1, -1]), np.array([-1, -1]), np.array([0.5, 0.7]))
        code, msg = _code(lambda: f.set_lift(np.eye(2), np.zeros(2), None, -np.ones(2), np.ones(2)))
        assert code == _lib.ERR_UNSUPPORTED and "forest" in msg
        f.upload_candidates(np.zeros((4, 2)))
        code, msg = _code(lambda: f.lift_sweep_topk([(_lib.ACQ_EI, 0.0)], 0.0, True, 1))
        assert code == _lib.ERR_UNSUPPORTED and "forest" in msg
    finally:
        f.close()


@pytest.mark.parametrize("N", [300, 1024])
def test_plain_sweep_is_untouched_by_a_lift(eng, N):
    r, D, M = 3, 20, 9001
    plugin = _model(eng, N, r, seed=3)
    Z = np.random.default_rng(14).uniform(-1, 1, size=(M, r))
    eng.upload_candidates(Z)
    before = eng.sweep_topk(Q4, plugin, True, k=16) + eng.sweep(Q4, plugin, True, return_values=True) + eng.predict()
    _set(eng, _lift(r, D))
    during = eng.sweep_topk(Q4, plugin, True, k=16) + eng.sweep(Q4, plugin, True, return_values=True) + eng.predict()
    eng.lift_sweep_topk(Q4, plugin, True, k=16)
    mid = eng.sweep_topk(Q4, plugin, True, k=16) + eng.sweep(Q4, plugin, True, return_values=True) + eng.predict()
    eng.clear_lift()
    after = eng.sweep_topk(Q4, plugin, True, k=16) + eng.sweep(Q4, plugin, True, return_values=True) + eng.predict()
    for other in (during, mid, after):  # a lift that is set changes nothing the plain calls return, before or after a lifted sweep
        for a, b in zip(before, other):
            assert np.array_equal(a, b)
