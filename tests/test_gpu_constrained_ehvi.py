"""Modelled constraints of a multi-objective run on the device (`bogp_sweep_ehvi_constrained`, kernels_ehvi_constrained.hip): the
feasibility-weighted EHVI against the NumPy restatement (tests/support/constrained_ehvi_ref.py) on the device's own moments and on the
reference's (golden G48); the moments and the probability of feasibility byte for byte against `bogp_sweep_constrained`'s; chunk and
top-k invariance; the skipped cell loop of wavefronts whose rows all have P == 0; the exact settings (every bound infinite, lo == hi,
no cells); the ABI's error returns; and the sibling sweeps left bit-identical.
T25: |v - ref| <= 1e-6 |ref| + 1e-12 max|ref|, every row, values and P alike (T12's / T19's form and reason: a dominated or
infeasible row is a product of differences of tail terms).

Measured on an MI355X (largest error over the bound's allowance, per row): values 8.2e-5, P 1.4e-9 over the seven cases; G48 on the
reference's moments 8.8e-8 and 3.6e-8, and 1.9e-7 of the batch maximum against its float32 EHVI (README ledger T25)."""
import numpy as np
import pytest

from bogp import _lib, pareto
from support import constrained_ehvi_ref as R
from support.ranked_tail import pin_ranked_tail
from test_gpu_ehvi import _check_argmax, _close_mse, _close_mu, _model

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _t25(v, ref, what="value"):
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    err = np.abs(v - ref)
    allow = 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()
    print("T25 %s: max |v - ref| = %.3g, max |ref| = %.3g, max err / allowance = %.3g" % (what, err.max(), np.abs(ref).max(), (err / allow).max()))
    assert np.all(err <= allow), err.max()


def _bounds(Y, m):
    """intervals cycling through (-inf, q50], [q25, q75], [q50, +inf) of the training columns m .. m + c - 1"""
    lo, hi = [], []
    for j in range(Y.shape[1] - m):
        q25, q50, q75 = np.quantile(Y[:, m + j], [0.25, 0.5, 0.75])
        a, b = ((-INF, q50), (q25, q75), (q50, INF))[j % 3]
        lo.append(a), hi.append(b)
    return np.array(lo), np.array(hi)


def _cells(Y, m):
    """the cells of the front of the first m columns, capped as test_gpu_ehvi._model caps it (6 points; 2 above three objectives)"""
    Yo = Y[:, :m]
    ref = Yo.min(axis=0) - 0.1 * np.abs(Yo.min(axis=0))
    P = pareto.pareto_front(Yo, ref)
    if m > 3 or len(P) > 40:
        return pareto.hypercell_bounds(P[np.argsort(-P[:, 0])[: (2 if m > 3 else 6)]], ref)
    return pareto.hypercell_bounds(Yo, ref)


def _candidates(X, M):
    """a third of the rows next to training rows (where a noiseless model with short length scales knows something: the moments,
    hence P, vary), the rest uniform over twice the training box (towards the prior: wide posteriors, EHVI well above rounding)"""
    rng = np.random.default_rng(1)
    near = X[rng.integers(len(X), size=M // 3)] + 0.05 * rng.normal(size=(M // 3, X.shape[1]))
    return np.vstack([near, rng.uniform(-4.0, 4.0, size=(M - M // 3, X.shape[1]))])


def _setup(eng, m, c, N, d, kernel, noisy, seed, M):
    X, Y, _, _ = _model(eng, m + c, N, d, kernel, noisy, seed=seed)
    lower, upper = _cells(Y, m)
    lo, hi = _bounds(Y, m)
    Xs = _candidates(X, M)
    eng.upload_candidates(Xs)
    return X, Y, Xs, lower, upper, lo, hi


def _all(eng, lower, upper, lo, hi, k=1):
    return eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=k, return_values=True, return_pof=True, return_moments=True)


def _check_all(eng, m, lower, upper, lo, hi, mom=None):
    """one call with every output; values, P and the winner against the restatement on `mom` (default: the device's own moments)"""
    best, idx, vals, pof, mu, mse = _all(eng, lower, upper, lo, hi)
    sig2 = eng.get_state(with_C=False)["sigma2"]
    rmu, rmse = (mu, mse) if mom is None else mom
    ref, rpof = R.values(rmu, rmse, sig2, m, lower, upper, lo, hi)
    _t25(pof, rpof, "P")
    _t25(vals, ref)
    _check_argmax(best, idx, vals, ref)  # T10
    return best, idx, vals, pof, mu, mse, ref, rpof


CASES = [  # (m, c, N, d, kernel, noisy)
    (2, 1, 43, 1, _lib.KERNEL_SE, False),  # below one tile; N no multiple of 8: the look-ahead tail
    (2, 2, 300, 5, _lib.KERNEL_MATERN52, True),
    (3, 1, 300, 5, _lib.KERNEL_SE, True),
    (3, 2, 700, 20, _lib.KERNEL_MATERN52, False),
    (2, 6, 300, 5, _lib.KERNEL_MATERN52, True),  # MT = 8
    (7, 1, 300, 5, _lib.KERNEL_MATERN52, True),  # the widest cell loop: a front of 2 points, 729 cells
    (3, 1, 2048, 20, _lib.KERNEL_MATERN52, True),  # the workload's N
]


@pytest.mark.parametrize("m,c,N,d,kernel,noisy", CASES)
def test_values_pof_and_winner_match_the_restatement(eng, m, c, N, d, kernel, noisy):
    M = 599 if m + c == 8 else 2999  # (neither is a multiple of 64)
    X, Y, Xs, lower, upper, lo, hi = _setup(eng, m, c, N, d, kernel, noisy, N + m + c, M)
    if m == 7:
        assert len(lower) == 729
    sig2 = eng.get_state(with_C=False)["sigma2"]
    # the restatement alone, on the device's moments, before the device's values are compared
    _, _, _, _, mu, mse = _all(eng, lower, upper, lo, hi)
    ref, rpof = R.values(mu, mse, sig2, m, lower, upper, lo, hi)
    assert 0 <= rpof.min() < rpof.max() <= 1
    assert (ref > 0).sum() >= len(ref) / 4
    ratio = np.sqrt(mse) / np.sqrt(sig2)
    assert not np.any((ratio > 1e-6 * (1 - 1e-3)) & (ratio < 1e-6 * (1 + 1e-3)))  # no row decides the variance guard by rounding
    _check_all(eng, m, lower, upper, lo, hi)


def test_moments_and_pof_are_the_constrained_sweeps_bytes(eng):
    m = 2
    X, Y, Xs, lower, upper, lo, hi = _setup(eng, m, 2, 700, 5, _lib.KERNEL_MATERN52, True, 3, 1001)
    _, _, _, pof, mu, mse = _all(eng, lower, upper, lo, hi)
    # bogp_sweep_constrained reads target 0 as the objective and targets 1 .. as constraints: infinite bounds on the objectives
    # 1 .. m - 1 contribute exactly 1.0 each, the rest are the same factors in the same order
    clo, chi = np.r_[np.full(m - 1, -INF), lo], np.r_[np.full(m - 1, INF), hi]
    _, _, pof_c, mu_c, mse_c = eng.sweep_constrained([(_lib.ACQ_NONE, 0.0)], 0.0, True, clo, chi, return_pof=True, return_moments=True)
    assert mu.tobytes() == mu_c.tobytes() and mse.tobytes() == mse_c.tobytes()
    assert pof.tobytes() == pof_c.tobytes()
    _, _, _, mu_e, mse_e = eng.sweep_ehvi(np.zeros((1, 4)), np.ones((1, 4)), return_values=True, return_moments=True)
    assert mu.tobytes() == mu_e.tobytes() and mse.tobytes() == mse_e.tobytes()


def test_chunk_and_topk_invariance(eng, monkeypatch):
    X, Y, Xs, lower, upper, lo, hi = _setup(eng, 3, 1, 700, 5, _lib.KERNEL_MATERN52, True, 3, 1001)
    full = _all(eng, lower, upper, lo, hi)
    assert eng.last_timing()["acquisition_ms"] > 0
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 candidates per chunk at Np = 704: 8 chunks
    chunked = _all(eng, lower, upper, lo, hi)
    assert eng.last_timing()["n_chunks"] >= 3
    monkeypatch.delenv("BOGP_CHUNK_MB")
    for a, b in zip(full, chunked):
        assert a.tobytes() == b.tobytes()
    vals = full[2]
    bk, ik = eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=7)
    order = sorted(range(len(vals)), key=lambda j: (-vals[j], j))[:7]  # k = 7: the stable sort of the stored values
    assert list(ik) == order and np.array_equal(bk, vals[order]) and ik[0] == full[1][0]
    # fewer candidates than k
    eng.upload_candidates(Xs[:1])
    b, i = eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=3)
    assert list(i) == [0, -1, -1] and b[0] == vals[0] and np.all(b[1:] == -INF)
    # the edges of the ranked tail on a tiny model: more ranks than candidates, a tie across the partial second workgroup
    X, Y, Xt, lower, upper, lo, hi = _setup(eng, 2, 1, 16, 2, _lib.KERNEL_SE, True, 9, 257)
    pin_ranked_tail(eng.upload_candidates, lambda k: eng.sweep_ehvi_constrained(lower[:4], upper[:4], lo, hi, k=k, return_values=True), Xt)


def test_wavefronts_whose_rows_are_all_infeasible_skip_the_cells(eng):
    m = 2
    X, Y, _, _ = _model(eng, m + 1, 300, 5, _lib.KERNEL_MATERN52, False, seed=11)
    lower, upper = _cells(Y, m)
    lo, hi = _bounds(Y, m)  # (-inf, q50]
    col = np.sort(Y[:, m])  # the bound at least 1e-3 away from every training value: the middle of the widest gap near the quantile
    j0 = int(np.searchsorted(col, hi[0]))
    j = max(range(max(0, j0 - 8), min(len(col) - 1, j0 + 8)), key=lambda i: col[i + 1] - col[i])
    hi[0] = 0.5 * (col[j] + col[j + 1])
    assert np.abs(Y[:, m] - hi[0]).min() >= 1e-3
    bad = Y[:, m] > hi[0]
    n_bad = int(bad.sum())
    assert 128 <= n_bad < 300  # two whole wavefronts of rows with P == 0 at least
    Xs = np.vstack([X[bad], X[~bad], np.random.default_rng(5).uniform(-2.5, 2.5, size=(500, 5))])
    eng.upload_candidates(Xs)
    best, idx, vals, pof, mu, mse = _all(eng, lower, upper, lo, hi)
    sig2 = eng.get_state(with_C=False)["sigma2"]
    assert np.all(np.sqrt(mse[:300]) / np.sqrt(sig2) < 1e-6)  # interpolation: every target of a training row under the guard
    assert np.all(pof[:n_bad] == 0.0) and np.all(pof[n_bad:300] == 1.0)
    assert np.all(vals[:n_bad] == 0.0) and not np.any(np.signbit(vals[:n_bad]))  # exactly +0.0
    ref, rpof = R.values(mu, mse, sig2, m, lower, upper, lo, hi)
    _t25(pof[n_bad:], rpof[n_bad:], "P")
    _t25(vals[n_bad:], ref[n_bad:])
    assert np.all(ref[:n_bad] == 0.0)
    _check_argmax(best, idx, vals, ref)
    assert idx[0] >= n_bad and best[0] > 0


def test_exact_constraint_settings_and_no_cells(eng):
    m, c, d = 3, 2, 5
    X, Y, Xs, lower, upper, lo, hi = _setup(eng, m, c, 300, d, _lib.KERNEL_MATERN52, True, 5, 2999)
    # every bound infinite: P is exactly 1 and the values are bogp_sweep_ehvi's on a model of the objective columns alone (T12:
    # the same expressions on the same moments, to rounding of another commit)
    bw, iw, vw, pw, muw, msew = _all(eng, lower, upper, np.full(c, -INF), np.full(c, INF))
    assert np.all(pw == 1.0)
    other = _lib.Engine(0)
    try:
        other.set_train(X, Y[:, :m])
        other.commit(_lib.KERNEL_MATERN52, _lib.MODE_NOISE_ESTIM, np.r_[np.full(d, 0.3 / d), 0.9], 0.0, False, 0.0)  # (_model's parameters)
        other.upload_candidates(Xs)
        be, ie, ve = other.sweep_ehvi(lower, upper, return_values=True)
    finally:
        other.close()
    assert np.all(np.abs(vw - ve) <= 1e-6 * np.abs(ve) + 1e-12 * np.abs(ve).max()), np.abs(vw - ve).max()  # T12
    _check_argmax(bw, iw, vw, ve)  # T10
    # lo == hi: every value +0.0, the winner is row 0
    b0, i0, v0, p0 = eng.sweep_ehvi_constrained(lower, upper, np.r_[0.25, lo[1:]], np.r_[0.25, hi[1:]], return_values=True, return_pof=True)
    assert np.all(p0 == 0.0) and np.all(v0 == 0.0) and not np.any(np.signbit(v0)) and i0[0] == 0 and b0[0] == 0.0
    # no cells: the probability of feasibility alone, byte for byte; NULL cell arrays are accepted
    bn, inn, vn, pn = eng.sweep_ehvi_constrained(np.zeros((0, m)), np.zeros((0, m)), lo, hi, return_values=True, return_pof=True)
    assert vn.tobytes() == pn.tobytes() and inn[0] == int(np.argmax(pn)) and bn[0] == pn.max()
    _, _, _, pof, _, _ = _all(eng, lower, upper, lo, hi)
    assert pn.tobytes() == pof.tobytes()


def test_g48_reference_golden(eng):
    """G48 (tests/support/make_constrained_ehvi_golden.py): a reference GaussianProcess on y (200, 4) -- two MOBO-style objectives and
    two constraints scaled as the drop-in scales them --, its moments on 2048 candidates, its NondominatedPartitioning cells of the
    feasible front and its own float32 EHVI of the objective columns.  The device's moments at T1 / T2; values and P against the
    restatement on the REFERENCE's moments at T25; with infinite bounds, against the reference's float32 EHVI to 1e-5 of the batch
    maximum (G39's rule); the argmax under T10."""
    from conftest import load_golden

    g = load_golden("G48_constrained_ehvi")
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], float(g["noise_var"]), False, 0.0)
    np.testing.assert_allclose(eng.get_state(with_C=False)["sigma2"], g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    best, idx, vals, pof, mu, mse, ref, rpof = _check_all(eng, 2, g["lower"], g["upper"], g["lo"], g["hi"], mom=(g["mu"], g["mse"]))
    for t in range(4):
        _close_mu(mu[:, t], g["mu"][:, t])
        _close_mse(mse[:, t], g["mse"][:, t], g["sigma2"][t])
    assert 0 < pof.min() and pof.max() > 0.5
    _, _, vw, pw = eng.sweep_ehvi_constrained(g["lower"], g["upper"], [-INF, -INF], [INF, INF], return_values=True, return_pof=True)
    assert np.all(pw == 1.0)
    print("G48: max |v - ehvi32| / max ehvi32 = %.3g" % (np.abs(vw - g["ehvi32"]).max() / np.abs(g["ehvi32"]).max()))
    assert np.abs(vw - g["ehvi32"]).max() <= 1e-5 * np.abs(g["ehvi32"]).max()


def test_sibling_sweeps_unchanged_around_constrained_ehvi(eng):
    X, Y, Xs, lower, upper, lo, hi = _setup(eng, 2, 1, 700, 5, _lib.KERNEL_MATERN52, True, 7, 3999)
    l3, u3 = _cells(Y, 3)
    clo, chi = np.r_[-INF, lo], np.r_[INF, hi]
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 1.0)]

    def siblings():
        eng.select_target(1)
        out = list(eng.sweep(acq, float(Y[:, 1].min()), True, return_values=True)) + list(eng.predict())
        eng.select_target(0)
        out += list(eng.sweep_ehvi(l3, u3, k=3, return_values=True, return_moments=True))
        out += list(eng.sweep_constrained([(_lib.ACQ_EI, 0.0), (_lib.ACQ_NONE, 0.0)], float(Y[:, 0].min()), True, clo, chi, k=2,
                                          return_values=True, return_pof=True, return_moments=True))  # fmt: skip
        return out

    before = siblings()
    _all(eng, lower, upper, lo, hi, k=4)
    after = siblings()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()


def test_abi_errors(eng):
    cells = (np.zeros((2, 2)), np.full((2, 2), INF))
    fresh = _lib.Engine(0)
    try:
        fresh.set_train(np.random.default_rng(0).uniform(size=(30, 2)), np.random.default_rng(1).uniform(size=(30, 3)))
        fresh.upload_candidates(np.zeros((4, 2)))
        with pytest.raises(_lib.BogpError, match="no committed model") as e:
            fresh.sweep_ehvi_constrained(*cells, [-INF], [0.0])
        assert e.value.code == _lib.ERR_INVALID
    finally:
        fresh.close()
    X, Y, _, _ = _model(eng, 3, 300, 2, _lib.KERNEL_SE, True, seed=9)
    eng.upload_candidates(np.random.default_rng(3).uniform(-2, 2, size=(37, 2)))
    lower, upper = _cells(Y, 2)
    lo, hi = _bounds(Y, 2)
    ok = lambda: _all(eng, lower, upper, lo, hi)  # noqa: E731
    good = ok()

    def refused(match, code, *a, **kw):
        with pytest.raises(_lib.BogpError, match=match) as e:
            eng.sweep_ehvi_constrained(*a, **kw)
        assert e.value.code == code
        again = ok()  # the handle is usable afterwards, and answers as before
        assert all(x.tobytes() == y.tobytes() for x, y in zip(good, again))

    refused("m_obj = 1", _lib.ERR_INVALID, lower[:, :1], upper[:, :1], np.r_[lo, lo], np.r_[hi, hi])
    refused("m_obj \\+ n_con = 2 \\+ 2", _lib.ERR_INVALID, lower, upper, np.r_[lo, lo], np.r_[hi, hi])
    refused("m_obj \\+ n_con = 3 \\+ 1", _lib.ERR_INVALID, np.zeros((1, 3)), np.ones((1, 3)), lo, hi)
    refused("cells", _lib.ERR_INVALID, np.zeros((_lib.MAX_EHVI_CELLS + 1, 2)), np.ones((_lib.MAX_EHVI_CELLS + 1, 2)), lo, hi)
    refused("k = 0", _lib.ERR_INVALID, lower, upper, lo, hi, k=0)
    refused("k = 33", _lib.ERR_INVALID, lower, upper, lo, hi, k=33)
    bad = lower.copy()
    bad[0, 0] = -INF
    refused("not finite", _lib.ERR_INVALID, bad, upper, lo, hi)
    bad = upper.copy()
    bad[0, 0] = np.nan
    refused("NaN", _lib.ERR_INVALID, lower, bad, lo, hi)
    bad = upper.copy()
    bad[0, 1] = -INF  # an inverted cell: upper below lower
    refused("below its lower", _lib.ERR_INVALID, lower, bad, lo, hi)
    refused("NaN", _lib.ERR_INVALID, lower, upper, [np.nan], hi)
    refused("below its lower", _lib.ERR_INVALID, lower, upper, [1.0], [0.5])
    h = eng._h
    f = eng._lib.bogp_sweep_ehvi_constrained
    one, idx1 = np.zeros(1), np.zeros(1, dtype=np.int64)
    P, L = _lib._ptr, idx1.ctypes.data_as(_lib._lp)
    assert f(h, 2, 0, None, None, 0, P(lo), P(hi), 1, P(one), L, None, None, None, None) == _lib.ERR_INVALID  # n_con < 1
    assert f(h, 2, 2, None, None, 1, P(lo), P(hi), 1, P(one), L, None, None, None, None) == _lib.ERR_INVALID  # null cells with C > 0
    assert f(h, 2, 2, P(lower), P(upper), 1, None, None, 1, P(one), L, None, None, None, None) == _lib.ERR_INVALID  # null bounds
    assert f(h, 2, 2, P(lower), P(upper), 1, P(lo), P(hi), 1, None, None, None, None, None, None) == _lib.ERR_INVALID  # null results
    assert f(h, 2, -1, None, None, 1, P(lo), P(hi), 1, P(one), L, None, None, None, None) == _lib.ERR_INVALID  # C < 0
    assert f(h, 2, 0, None, None, 1, P(lo), P(hi), 1, P(one), L, None, None, None, None) == _lib.OK  # C == 0 takes NULL cells
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, ok()))
    eng.set_lift(np.eye(2), np.zeros(2), np.zeros(2), np.full(2, -3.0), np.full(2, 3.0))
    try:
        with pytest.raises(_lib.BogpError, match="lift") as e:
            eng.sweep_ehvi_constrained(lower, upper, lo, hi)
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        eng.clear_lift()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(good, ok()))
    # two targets (no constraint column left); one target under a polynomial trend basis; no candidates
    eng.set_train(X, Y[:, :2])
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(2, 0.15), 0.9], 0.0, False, 0.0)
    eng.upload_candidates(np.zeros((8, 2)))
    with pytest.raises(_lib.BogpError, match="2 targets") as e:
        eng.sweep_ehvi_constrained(lower, upper, lo, hi)
    assert e.value.code == _lib.ERR_INVALID
    eng.set_train(X, Y[:, :1])
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(2, 0.15), 0.9], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    eng.upload_candidates(np.zeros((8, 2)))
    with pytest.raises(_lib.BogpError, match="constant trend") as e:
        eng.sweep_ehvi_constrained(lower, upper, lo, hi)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    eng.set_train(X[:, :1], Y)  # another width forgets the candidates
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[0.15, 0.9], 0.0, False, 0.0)
    with pytest.raises(_lib.BogpError, match="no candidates") as e:
        eng.sweep_ehvi_constrained(lower, upper, lo, hi)
    assert e.value.code == _lib.ERR_INVALID


def test_forest_handle_is_refused():
    fe = _lib.Engine(0)
    try:  # two trees of three nodes over two columns
        fe.forest_set(d=2, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                      left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=[0, 1.0, 2.0, 0, 3.0, 5.0])  # fmt: skip
        fe.upload_candidates(np.random.default_rng(0).uniform(size=(8, 2)))
        with pytest.raises(_lib.BogpError, match="forest") as e:
            fe.sweep_ehvi_constrained(np.zeros((1, 2)), np.ones((1, 2)), [-INF], [0.0])
        assert e.value.code == _lib.ERR_UNSUPPORTED
    finally:
        fe.close()
