"""Modelled constraints on the device (`bogp_sweep_constrained`, kernels_constrained.hip): the feasibility-weighted criteria against
the NumPy restatement (tests/support/constrained_ref.py) on the reference's moments (golden G45) and on the device's own moments;
the moments byte for byte against `bogp_sweep_ehvi`'s; chunk, criterion-count and top-k invariance; the small / lazy / generated
candidate paths; the exact cases (every bound infinite, lo == hi, the model's own training rows); the ABI's error returns; and
single-target sweeps left bit-identical.  T19: |v - ref| <= 1e-6 |ref| + 1e-12 max|ref|, every row (T12's form and reason)."""
import numpy as np
import pytest

from bogp import _lib
from support import constrained_ref as R
from support.ranked_tail import pin_ranked_tail
from test_gpu_ehvi import _check_argmax, _close_mse, _close_mu, _model

pytestmark = pytest.mark.gpu
INF = float("inf")
ACQ4 = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_EPSILON_PI, 0.0), (_lib.ACQ_MGFI, 2.0), (_lib.ACQ_NONE, 0.0)]  # EI, PI, MGFI (t = 2), feasibility only


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _t19(v, ref):
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    err = np.abs(v - ref)
    print("T19: max |v - ref| = %.3g, max |ref| = %.3g" % (err.max(), np.abs(ref).max()))
    assert np.all(err <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()), err.max()


def _bounds(Y):
    """intervals cycling through (-inf, q50], [q25, q75], [q50, +inf) of the training columns 1 .. m - 1"""
    lo, hi = [], []
    for k in range(1, Y.shape[1]):
        q25, q50, q75 = np.quantile(Y[:, k], [0.25, 0.5, 0.75])
        a, b = ((-INF, q50), (q25, q75), (q50, INF))[(k - 1) % 3]
        lo.append(a), hi.append(b)
    return np.array(lo), np.array(hi)


def _check_all(eng, acq, plugin, minimize, lo, hi, mom=None):
    """one call with every output; values, PoF and winners against the restatement on `mom` (default: the device's own moments)"""
    best, idx, vals, pof, mu, mse = eng.sweep_constrained(acq, plugin, minimize, lo, hi, return_values=True, return_pof=True, return_moments=True)
    sig2 = eng.get_state(with_C=False)["sigma2"]
    rmu, rmse = (mu, mse) if mom is None else mom
    ref, rpof = R.constrained(rmu, rmse, sig2, lo, hi, acq, plugin, minimize)
    _t19(pof, rpof)
    for c in range(len(acq)):
        _t19(vals[c], ref[c])
        _check_argmax(best[c], idx[c], vals[c], ref[c])
    return best, idx, vals, pof, mu, mse


def test_g45_reference_golden(eng):
    """G45 (tests/support/make_constrained_golden.py): a reference GaussianProcess on y (200, 3) -- objective and two constraints scaled as
    the drop-in scales them --, its moments on 2048 candidates.  The device's moments at T1 / T2; EI, PI, MGFI (t = 2) and the
    probability of feasibility against the restatement on the REFERENCE's moments at T19; the argmax exact on the device's values."""
    from conftest import load_golden

    g = load_golden("G45_constrained")
    y = g["y"]
    eng.set_train(g["X"], y)
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], float(g["noise_var"]), False, 0.0)
    np.testing.assert_allclose(eng.get_state(with_C=False)["sigma2"], g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    lo, hi = np.array([-INF, np.quantile(y[:, 2], 0.25)]), np.array([0.0, np.quantile(y[:, 2], 0.75)])
    feas = np.all((y[:, 1:] >= lo) & (y[:, 1:] <= hi), axis=1)
    assert feas.any()
    for minimize in (True, False):
        plugin = float(y[feas, 0].min() if minimize else -y[feas, 0].max())
        best, idx, vals, pof, mu, mse = _check_all(eng, ACQ4, plugin, minimize, lo, hi, mom=(g["mu"], g["mse"]))
        for t in range(3):
            _close_mu(mu[:, t], g["mu"][:, t])
            _close_mse(mse[:, t], g["mse"][:, t], g["sigma2"][t])
        assert 0 < pof.min() and pof.max() < 1 and pof.max() > 0.5


CASES = [  # (m, N, d, kernel, noisy): below one 64-tile, two slices, three column groups, the largest m, the workload's N
    (2, 40, 1, _lib.KERNEL_SE, False),
    (2, 300, 5, _lib.KERNEL_MATERN52, True),
    (3, 300, 5, _lib.KERNEL_SE, True),
    (3, 700, 20, _lib.KERNEL_MATERN52, False),
    (8, 300, 5, _lib.KERNEL_MATERN52, True),
    (4, 2048, 20, _lib.KERNEL_MATERN52, True),
]


@pytest.mark.parametrize("m,N,d,kernel,noisy", CASES)
def test_values_pof_and_winner_match_the_restatement(eng, m, N, d, kernel, noisy):
    X, Y, _, _ = _model(eng, m, N, d, kernel, noisy, seed=N + m)
    Xs = np.random.default_rng(1).uniform(-2.5, 2.5, size=(599 if m == 8 else 2999, d))  # (no multiple of 64)
    eng.upload_candidates(Xs)
    lo, hi = _bounds(Y)
    sig2 = eng.get_state(with_C=False)["sigma2"]
    for minimize in (True, False):
        plugin = float(Y[:, 0].min() if minimize else -Y[:, 0].max())
        best, idx, vals, pof, mu, mse = _check_all(eng, ACQ4, plugin, minimize, lo, hi)
        ratio = np.sqrt(mse) / np.sqrt(sig2)
        assert not np.any((ratio > 1e-6 * (1 - 1e-3)) & (ratio < 1e-6 * (1 + 1e-3)))  # no row decides the guard by rounding
        assert 0 <= pof.min() < pof.max() <= 1  # both infinite sides and a finite interval: PoF is no constant


def test_moments_are_the_ehvi_sweeps_bytes(eng):
    X, Y, clo, chi = _model(eng, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=3)
    Xs = np.random.default_rng(2).uniform(-2.5, 2.5, size=(1001, 5))
    eng.upload_candidates(Xs)
    _, _, _, mu_e, mse_e = eng.sweep_ehvi(clo[:1], chi[:1], return_values=True, return_moments=True)
    lo, hi = _bounds(Y)
    _, _, mu_c, mse_c = eng.sweep_constrained(ACQ4[:1], float(Y[:, 0].min()), True, lo, hi, return_moments=True)
    assert mu_c.tobytes() == mu_e.tobytes() and mse_c.tobytes() == mse_e.tobytes()


def test_chunk_criteria_and_topk_invariance(eng, monkeypatch):
    X, Y, _, _ = _model(eng, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=3)
    Xs = np.random.default_rng(2).uniform(-2.5, 2.5, size=(1001, 5))
    eng.upload_candidates(Xs)
    lo, hi = _bounds(Y)
    plugin = float(Y[:, 0].min())
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_MGFI, 2.0), (_lib.ACQ_EPSILON_PI, 0.05)]
    full = eng.sweep_constrained(acq, plugin, True, lo, hi, return_values=True, return_pof=True, return_moments=True)
    assert eng.last_timing()["acquisition_ms"] > 0
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 candidates per chunk at Np = 704: 8 chunks
    chunked = eng.sweep_constrained(acq, plugin, True, lo, hi, return_values=True, return_pof=True, return_moments=True)
    assert eng.last_timing()["n_chunks"] >= 3
    monkeypatch.delenv("BOGP_CHUNK_MB")
    for a, b in zip(full, chunked):
        assert a.tobytes() == b.tobytes()
    best, idx, vals = full[:3]
    for c, one in enumerate(acq):  # q = 3 in one call == three q = 1 calls, bit for bit
        b1, i1, v1 = eng.sweep_constrained([one], plugin, True, lo, hi, return_values=True)
        assert v1[0].tobytes() == vals[c].tobytes() and b1[0, 0] == best[c, 0] and i1[0, 0] == idx[c, 0]
    bk, ik = eng.sweep_constrained(acq, plugin, True, lo, hi, k=7)
    for c in range(3):  # k = 7: the stable sort of the stored values
        order = sorted(range(len(vals[c])), key=lambda j: (-vals[c][j], j))[:7]
        assert list(ik[c]) == order and np.array_equal(bk[c], vals[c][order])
    # the edges of the ranked tail on a tiny model: more ranks than candidates, a tie across the partial second workgroup
    X, Y, _, _ = _model(eng, 2, 16, 2, _lib.KERNEL_SE, True, seed=9)
    lo, hi = _bounds(Y)
    Xt = np.random.default_rng(3).uniform(-2.5, 2.5, size=(257, 2))
    one = lambda k: [a[0] for a in eng.sweep_constrained(acq[:1], float(Y[:, 0].min()), True, lo, hi, k=k, return_values=True)]  # noqa: E731
    pin_ranked_tail(eng.upload_candidates, one, Xt)


def test_single_target_sweep_unchanged_around_constrained(eng):
    X, Y, _, _ = _model(eng, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=7)
    Xs = np.random.default_rng(6).uniform(-2.5, 2.5, size=(3999, 5))
    eng.upload_candidates(Xs)
    eng.select_target(1)
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 1.0)]
    before = eng.sweep(acq, float(Y[:, 1].min()), True, return_values=True)
    mu_b, mse_b = eng.predict()
    lo, hi = _bounds(Y)
    eng.sweep_constrained(ACQ4, float(Y[:, 0].min()), True, lo, hi, k=4, return_values=True, return_pof=True, return_moments=True)
    after = eng.sweep(acq, float(Y[:, 1].min()), True, return_values=True)
    mu_a, mse_a = eng.predict()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(mu_a, mu_b) and np.array_equal(mse_a, mse_b)
    eng.select_target(0)


def test_small_lazy_generated_and_exact_bounds(eng):
    X, Y, _, _ = _model(eng, 3, 300, 3, _lib.KERNEL_SE, True, seed=5)
    Xs = np.random.default_rng(4).uniform(-2.5, 2.5, size=(20001, 3))
    lo, hi = _bounds(Y)
    plugin = float(Y[:, 0].min())
    eng.upload_candidates(Xs)
    _, _, vfull, pfull = eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True, return_pof=True)
    for M in (1, 37, 257):  # M = 1: the criterion's one-row call; no single-target small-batch shortcut is taken
        eng.upload_candidates(Xs[:M])
        b, i, v, p = eng.sweep_constrained(ACQ4, plugin, True, lo, hi, k=3, return_values=True, return_pof=True)
        assert v.tobytes() == np.ascontiguousarray(vfull[:, :M]).tobytes() and p.tobytes() == pfull[:M].tobytes()
        assert np.array_equal(i[:, 0], np.argmax(v, axis=1))
        if M == 1:
            assert i.tolist() == [[0, -1, -1]] * 4 and np.all(b[:, 1:] == -INF)
    eng.upload_candidates(Xs, lazy=True)
    _, _, vlazy = eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True)
    assert vlazy.tobytes() == vfull.tobytes()
    eng.generate_candidates(np.full(3, -2.5), np.full(3, 2.5), 5001, 11)
    Xg = eng.read_candidates(np.arange(5001))
    _, _, vg = _check_all(eng, ACQ4, plugin, True, lo, hi)[:3]
    eng.upload_candidates(Xg)
    assert eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True)[2].tobytes() == vg.tobytes()
    # every bound infinite: PoF is exactly 1, the values are the single-target sweep's on target 0 (T19: another summation order of mu)
    eng.upload_candidates(Xs[:2999])
    wide = eng.sweep_constrained(ACQ4[:3], plugin, True, [-INF, -INF], [INF, INF], return_values=True, return_pof=True)
    assert np.all(wide[3] == 1.0)
    eng.select_target(0)
    _, _, single = eng.sweep(ACQ4[:3], plugin, True, return_values=True)
    for c in range(3):
        _t19(wide[2][c], single[c])
    # lo == hi: every value 0, the winner is row 0
    b0, i0, v0 = eng.sweep_constrained(ACQ4, plugin, True, [0.25, -INF], [0.25, INF], return_values=True)
    assert np.all(v0 == 0.0) and np.all(i0 == 0) and np.all(b0 == 0.0)


def test_training_rows_of_a_noiseless_model_give_the_indicator(eng):
    X, Y, _, _ = _model(eng, 3, 300, 5, _lib.KERNEL_MATERN52, False, seed=11)
    eng.upload_candidates(X[:299])
    lo, hi = _bounds(Y)
    for k in range(2):  # bounds at least 1e-3 away from every training value: the middle of the widest gap near the quantile
        col = np.sort(Y[:, k + 1])
        for b in (lo, hi):
            if np.isfinite(b[k]):
                j0 = int(np.searchsorted(col, b[k]))
                j = max(range(max(0, j0 - 8), min(len(col) - 1, j0 + 8)), key=lambda i: col[i + 1] - col[i])
                b[k] = 0.5 * (col[j] + col[j + 1])
                assert np.abs(Y[:, k + 1] - b[k]).min() >= 1e-3
    _, _, vals, pof, mu, mse = eng.sweep_constrained([(_lib.ACQ_NONE, 0.0), (_lib.ACQ_EI, 0.0)], float(Y[:, 0].min()), True, lo, hi,
                                                     return_values=True, return_pof=True, return_moments=True)  # fmt: skip
    sig2 = eng.get_state(with_C=False)["sigma2"]
    assert np.all(np.sqrt(mse) / np.sqrt(sig2) < 1e-6)  # interpolation: every target under the guard
    want = np.all((Y[:299, 1:] >= lo) & (Y[:299, 1:] <= hi), axis=1).astype(float)
    assert 0 < want.sum() < len(want)
    assert np.array_equal(vals[0], want) and np.array_equal(pof, want)
    assert np.all(vals[1] == 0.0)


def test_abi_errors(eng):
    fresh = _lib.Engine(0)
    try:
        fresh.set_train(np.random.default_rng(0).uniform(size=(30, 2)), np.random.default_rng(1).uniform(size=(30, 2)))
        fresh.upload_candidates(np.zeros((4, 2)))
        with pytest.raises(_lib.BogpError, match="no committed model") as e:
            fresh.sweep_constrained(ACQ4[:1], 0.0, True, [-INF], [0.0])
        assert e.value.code == _lib.ERR_INVALID
    finally:
        fresh.close()
    X, Y, _, _ = _model(eng, 3, 300, 2, _lib.KERNEL_SE, True, seed=9)
    eng.upload_candidates(np.random.default_rng(3).uniform(-2, 2, size=(37, 2)))
    lo, hi = _bounds(Y)
    ok = lambda: eng.sweep_constrained(ACQ4, 0.0, True, lo, hi, return_values=True)  # noqa: E731
    good = ok()

    def refused(match, code, *a, **kw):
        with pytest.raises(_lib.BogpError, match=match) as e:
            eng.sweep_constrained(*a, **kw)
        assert e.value.code == code
        again = ok()  # the handle is usable afterwards, and answers as before
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again))

    refused("n_con = 1", _lib.ERR_INVALID, ACQ4, 0.0, True, lo[:1], hi[:1])
    refused("q = 0", _lib.ERR_INVALID, [], 0.0, True, lo, hi)
    refused("q = 65", _lib.ERR_INVALID, ACQ4[:1] * 65, 0.0, True, lo, hi)
    refused("k = 0", _lib.ERR_INVALID, ACQ4, 0.0, True, lo, hi, k=0)
    refused("k = 33", _lib.ERR_INVALID, ACQ4, 0.0, True, lo, hi, k=33)
    refused("UCB", _lib.ERR_INVALID, [(_lib.ACQ_UCB, 0.5)], 0.0, True, lo, hi)
    refused("unknown acquisition id", _lib.ERR_INVALID, [(7, 0.5)], 0.0, True, lo, hi)
    refused("must be > 0", _lib.ERR_INVALID, [(_lib.ACQ_MGFI, 0.0)], 0.0, True, lo, hi)
    refused("NaN", _lib.ERR_INVALID, ACQ4, 0.0, True, [np.nan, -INF], hi)
    refused("below its lower", _lib.ERR_INVALID, ACQ4, 0.0, True, [1.0, -INF], [0.5, INF])
    rc = eng._lib.bogp_sweep_constrained(eng._h, 1, None, None, 0.0, 1, 2, None, None, 1, None, None, None, None, None, None)
    assert rc == _lib.ERR_INVALID  # null required arrays
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, ok()))
    eng.set_lift(np.eye(2), np.zeros(2), np.zeros(2), np.full(2, -3.0), np.full(2, 3.0))
    try:
        refused_lift = pytest.raises(_lib.BogpError, match="lift")
        with refused_lift as e:
            eng.sweep_constrained(ACQ4, 0.0, True, lo, hi)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        eng.clear_lift()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, ok()))
    # one target; a polynomial trend basis; no candidates
    eng.set_train(X, Y[:, :1])
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(2, 0.15), 0.9], 0.0, False, 0.0)
    eng.upload_candidates(np.zeros((8, 2)))
    with pytest.raises(_lib.BogpError, match="1 target") as e:
        eng.sweep_constrained(ACQ4, 0.0, True, [-INF], [0.0])
    assert e.value.code == _lib.ERR_INVALID
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(2, 0.15), 0.9], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    with pytest.raises(_lib.BogpError, match="constant trend") as e:
        eng.sweep_constrained(ACQ4, 0.0, True, [-INF], [0.0])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    eng.set_train(X[:, :1], Y)  # another width forgets the candidates
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[0.15, 0.9], 0.0, False, 0.0)
    with pytest.raises(_lib.BogpError, match="no candidates") as e:
        eng.sweep_constrained(ACQ4, 0.0, True, lo, hi)
    assert e.value.code == _lib.ERR_INVALID


def test_forest_handle_is_refused():
    fe = _lib.Engine(0)
    try:  # two trees of three nodes over two columns
        fe.forest_set(d=2, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                      left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=[0, 1.0, 2.0, 0, 3.0, 5.0])  # fmt: skip
        fe.upload_candidates(np.random.default_rng(0).uniform(size=(8, 2)))
        with pytest.raises(_lib.BogpError, match="forest") as e:
            fe.sweep_constrained(ACQ4[:1], 0.0, True, [-INF], [0.0])
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        fe.close()
