"""EHVI on the device (`bogp_sweep_ehvi`, kernels_ehvi.hip): the m-target posterior of the chunked sweep and the
expected hypervolume improvement against the float64 restatement of the reference's algebra (tests/support/ehvi_ref64.py)
evaluated on the device's own moments; the moments against `bogp_predict` per target; chunk invariance, top-k, the
small / lazy / generated candidate paths, the ABI's error returns, and single-target sweeps left bit-identical."""
import os

import numpy as np
import pytest

from bogp import _lib
from bogp import pareto
from support.ehvi_ref64 import ehvi as ehvi_ref
from support.ranked_tail import pin_ranked_tail

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _model(eng, m, N, d, kernel, noisy, seed=0):
    """An m-target model committed at fixed hyper-parameters (fixed constant trend, as several targets require) with
    distinct per-target scales, so that the sigma2_k differ.  Returns (Y, cells lower, cells upper)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    base = np.sin(X @ rng.normal(size=(d, m)))
    Y = base * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    eng.set_train(X, Y)
    theta = np.full(d, (0.3 if noisy else 200.0) / d)  # (noiseless: short length scales keep R well conditioned)
    if kernel == _lib.KERNEL_MATERN_NU:
        par, mode, nv = np.r_[theta, 1.7], _lib.MODE_NOISELESS, 0.0
    elif noisy:
        par, mode, nv = np.r_[theta, 0.9], _lib.MODE_NOISE_ESTIM, 0.0  # (sigma2_k = 0.9 x the target's total variance)
    else:
        par, mode, nv = theta, _lib.MODE_NOISELESS, 0.0
    eng.commit(kernel, mode, par, nv, False, 0.0)
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    P = pareto.pareto_front(Y, ref)
    if m > 3 or len(P) > 40:  # keep the grid small: a front of at most 6 points (2 above three objectives: 3^(m-1) cells)
        Ysub = P[np.argsort(-P[:, 0])[: (2 if m > 3 else 6)]]
        lo, hi = pareto.hypercell_bounds(Ysub, ref)
    else:
        lo, hi = pareto.hypercell_bounds(Y, ref)
    return X, Y, lo, hi


def _check_ehvi(vals, mu, mse, lo, hi):
    ref = ehvi_ref(mu, mse, lo, hi)
    scale = np.abs(ref).max()
    assert np.all(np.abs(vals - ref) <= 1e-6 * np.abs(ref) + 1e-12 * scale), np.abs(vals - ref).max()
    return ref


def _check_argmax(best, idx, vals, ref):
    assert best[0] == vals[idx[0]]
    j = int(np.argmax(vals))
    assert idx[0] == j
    r = int(np.argmax(ref))
    assert idx[0] == r or abs(ref[idx[0]] - ref[r]) <= 1e-9 * abs(ref[r])  # T10: exact unless the restatement ties


def _close_mu(a, ref):  # T1 (tests/test_gpu_parity.py close_mu)
    np.testing.assert_allclose(np.ravel(a), np.ravel(ref), rtol=1e-6, atol=1e-9)


def _close_mse(a, ref, sigma2):  # T2 (close_mse)
    np.testing.assert_allclose(np.ravel(a), np.ravel(ref), rtol=1e-6, atol=1e-12 * float(sigma2))


@pytest.mark.parametrize("state", ["m2", "m3"])
def test_g39_reference_golden(eng, state):
    """G39 (tests/support/make_ehvi_golden.py): a reference GaussianProcess on MOBO-style y (MinMax-scaled, negated), its moments on
    2048 candidates, its float64 cells and its own per-row float32 EHVI as MOBO computes it.  The device's moments at T1 / T2; the
    device's EHVI on the reference's cells against the float64 restatement on the reference's moments (T12) and against the
    reference's own float32 values to 1e-5 of the batch maximum; the argmax under T10.  The cells go in twice: with +inf upper
    bounds and with the reference's 1e10 clamp (analytic.py:236-238) -- same values."""
    from conftest import load_golden

    g = {k[len(state) + 1 :]: v for k, v in load_golden("G39_ehvi").items() if k.startswith(state + "_")}
    m = g["y"].shape[1]
    eng.set_train(g["X"], g["y"])
    eng.commit(int(g["kernel"]), int(g["mode"]), g["par"], float(g["noise_var"]), False, 0.0)
    np.testing.assert_allclose(eng.get_state(with_C=False)["sigma2"], g["sigma2"], rtol=1e-9)
    eng.upload_candidates(g["Xs"])
    best, idx, vals, mu, mse = eng.sweep_ehvi(g["lower"], g["upper"], k=1, return_values=True, return_moments=True)
    for t in range(m):
        _close_mu(mu[:, t], g["mu"][:, t])
        _close_mse(mse[:, t], g["mse"][:, t], g["sigma2"][t])
    ref = ehvi_ref(g["mu"], g["mse"], g["lower"], g["upper"])
    assert np.all(np.abs(vals - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()), np.abs(vals - ref).max()
    assert np.abs(vals - g["ehvi32"]).max() <= 1e-5 * np.abs(g["ehvi32"]).max()
    _check_argmax(best, idx, vals, ref)
    _, idx_c, vals_c = eng.sweep_ehvi(g["lower"], np.minimum(g["upper"], 1e10), return_values=True)
    assert np.all(np.abs(vals_c - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max())
    assert idx_c[0] == idx[0]


CASES = [  # (m, N, d, kernel, noisy)
    (2, 40, 1, _lib.KERNEL_SE, False),
    (2, 300, 5, _lib.KERNEL_MATERN52, True),
    (3, 300, 5, _lib.KERNEL_SE, True),
    (3, 700, 20, _lib.KERNEL_MATERN52, False),
    (2, 2048, 20, _lib.KERNEL_MATERN52, True),
    (3, 2048, 5, _lib.KERNEL_MATERN_NU, False),
    (8, 300, 5, _lib.KERNEL_MATERN52, True),
    (8, 700, 1, _lib.KERNEL_SE, True),
    (2, 3200, 5, _lib.KERNEL_SE, True),
]


@pytest.mark.parametrize("m,N,d,kernel,noisy", CASES)
def test_ehvi_matches_restatement_and_predict(eng, m, N, d, kernel, noisy):
    X, Y, lo, hi = _model(eng, m, N, d, kernel, noisy, seed=N + m)
    rng = np.random.default_rng(1)
    Xs = rng.uniform(-2.5, 2.5, size=(3000 if m <= 3 else 600, d))  # (the restatement's 2^m terms cost host time)
    eng.upload_candidates(Xs)
    best, idx, vals, mu, mse = eng.sweep_ehvi(lo, hi, k=1, return_values=True, return_moments=True)
    sig2 = eng.get_state(with_C=False)["sigma2"]
    for t in range(m):
        eng.select_target(t)
        pm, pmse = eng.predict()
        np.testing.assert_allclose(mu[:, t], pm, rtol=1e-9, atol=1e-12 * np.abs(pm).max())
        np.testing.assert_allclose(mse[:, t], pmse, rtol=1e-6, atol=1e-12 * float(sig2[t]))
    eng.select_target(0)
    assert len(set(np.round(sig2, 12))) == m  # distinct sigma2_k
    ref = _check_ehvi(vals, mu, mse, lo, hi)
    _check_argmax(best, idx, vals, ref)


def test_chunk_invariance_and_topk(eng, monkeypatch):
    X, Y, lo, hi = _model(eng, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=3)
    Xs = np.random.default_rng(2).uniform(-2.5, 2.5, size=(1000, 5))
    eng.upload_candidates(Xs)
    b1, i1, v1, mu1, mse1 = eng.sweep_ehvi(lo, hi, k=1, return_values=True, return_moments=True)
    assert eng.last_timing()["acquisition_ms"] > 0
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 candidates per chunk at Np = 704: 8 chunks
    b2, i2, v2, mu2, mse2 = eng.sweep_ehvi(lo, hi, k=1, return_values=True, return_moments=True)
    assert eng.last_timing()["n_chunks"] >= 3
    assert np.array_equal(v1, v2) and np.array_equal(mu1, mu2) and np.array_equal(mse1, mse2)
    assert np.array_equal(b1, b2) and np.array_equal(i1, i2)
    monkeypatch.delenv("BOGP_CHUNK_MB")
    bk, ik = eng.sweep_ehvi(lo, hi, k=7)
    order = sorted(range(len(v1)), key=lambda j: (-v1[j], j))[:7]
    assert list(ik) == order and np.array_equal(bk, v1[order])
    assert ik[0] == i1[0]
    # the edges of the ranked tail on a tiny model: more ranks than candidates, a tie across the partial second workgroup
    _, _, lo, hi = _model(eng, 2, 16, 2, _lib.KERNEL_SE, True, seed=9)
    Xt = np.random.default_rng(3).uniform(-2.5, 2.5, size=(257, 2))
    pin_ranked_tail(eng.upload_candidates, lambda k: eng.sweep_ehvi(lo[:4], hi[:4], k=k, return_values=True), Xt)


def test_small_lazy_generated_and_cells(eng):
    X, Y, lo, hi = _model(eng, 2, 300, 3, _lib.KERNEL_SE, True, seed=5)
    Xs = np.random.default_rng(4).uniform(-2.5, 2.5, size=(20000, 3))
    eng.upload_candidates(Xs)
    _, _, vfull = eng.sweep_ehvi(lo, hi, return_values=True)
    for M in (1, 5, 33):  # M = 1: the criterion's one-row call; no single-target small-batch shortcut is taken
        eng.upload_candidates(Xs[:M])
        b, i, v, mu, mse = eng.sweep_ehvi(lo, hi, k=3, return_values=True, return_moments=True)
        np.testing.assert_allclose(v, vfull[:M], rtol=1e-12, atol=1e-15)
        _check_ehvi(v, mu, mse, lo, hi)
        if M == 1:
            assert list(i) == [0, -1, -1] and b[1] == -np.inf
    eng.upload_candidates(Xs, lazy=True)
    _, _, vlazy = eng.sweep_ehvi(lo, hi, return_values=True)
    assert np.array_equal(vlazy, vfull)
    eng.generate_candidates(np.full(3, -2.5), np.full(3, 2.5), 5000, 11)
    Xg = eng.read_candidates(np.arange(5000))
    bg, ig, vg, mug, mseg = eng.sweep_ehvi(lo, hi, return_values=True, return_moments=True)
    _check_ehvi(vg, mug, mseg, lo, hi)
    eng.upload_candidates(Xg)
    assert np.array_equal(eng.sweep_ehvi(lo, hi, return_values=True)[2], vg)
    # a single cell with +inf upper bounds (an empty front): EHVI = prod_k E[(Y_k - l_k)^+]
    eng.upload_candidates(Xs[:2000])
    one_lo, one_hi = np.array([[-1.0, -2.0]]), np.full((1, 2), np.inf)
    _, _, v1, mu1, mse1 = eng.sweep_ehvi(one_lo, one_hi, return_values=True, return_moments=True)
    _check_ehvi(v1, mu1, mse1, one_lo, one_hi)
    # a one-point front: two cells
    l2, h2 = pareto.hypercell_bounds(np.array([[0.5, 0.5]]), [-1.0, -1.0])
    assert len(l2) == 2
    _, _, v2, mu2, mse2 = eng.sweep_ehvi(l2, h2, return_values=True, return_moments=True)
    _check_ehvi(v2, mu2, mse2, l2, h2)


def test_single_target_sweep_unchanged_around_ehvi(eng):
    X, Y, lo, hi = _model(eng, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=7)
    Xs = np.random.default_rng(6).uniform(-2.5, 2.5, size=(4000, 5))
    eng.upload_candidates(Xs)
    eng.select_target(1)
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 1.0)]
    before = eng.sweep(acq, float(Y[:, 1].min()), True, return_values=True)
    mu_b, mse_b = eng.predict()
    eng.sweep_ehvi(lo, hi, k=4, return_values=True, return_moments=True)
    after = eng.sweep(acq, float(Y[:, 1].min()), True, return_values=True)
    mu_a, mse_a = eng.predict()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(mu_a, mu_b) and np.array_equal(mse_a, mse_b)
    eng.select_target(0)


def test_abi_errors(eng):
    lo, hi = np.zeros((2, 2)), np.full((2, 2), np.inf)
    fresh = _lib.Engine(0)
    try:
        fresh.set_train(np.random.default_rng(0).uniform(size=(30, 2)), np.random.default_rng(1).uniform(size=(30, 2)))
        fresh.upload_candidates(np.zeros((4, 2)))
        with pytest.raises(_lib.BogpError, match="no committed model"):
            fresh.sweep_ehvi(lo, hi)
    finally:
        fresh.close()
    X, Y, lo3, hi3 = _model(eng, 3, 300, 2, _lib.KERNEL_SE, True, seed=9)
    eng.upload_candidates(np.zeros((8, 2)))
    with pytest.raises(_lib.BogpError, match="m = 2"):
        eng.sweep_ehvi(lo, hi)  # a 3-target model with 2-objective cells
    with pytest.raises(_lib.BogpError, match="cells"):
        eng.sweep_ehvi(np.zeros((_lib.MAX_EHVI_CELLS + 1, 3)), np.ones((_lib.MAX_EHVI_CELLS + 1, 3)))
    with pytest.raises(_lib.BogpError, match="cells"):
        eng.sweep_ehvi(np.zeros((0, 3)), np.zeros((0, 3)))
    bad = hi3.copy()
    bad[0, 0] = np.nan
    with pytest.raises(_lib.BogpError, match="NaN"):
        eng.sweep_ehvi(lo3, bad)
    bad = hi3.copy()
    bad[0, 1] = -np.inf  # an inverted cell: upper below lower
    with pytest.raises(_lib.BogpError, match="below its lower"):
        eng.sweep_ehvi(lo3, bad)
    bad, bad_hi = lo3.copy(), hi3.copy()
    bad[1, 0], bad_hi[1, 0] = 5.0, 4.5  # finite and inverted
    with pytest.raises(_lib.BogpError, match="below its lower"):
        eng.sweep_ehvi(bad, bad_hi)
    with pytest.raises(_lib.BogpError, match="k = 33"):
        eng.sweep_ehvi(lo3, hi3, k=33)
    eng.set_train(X, Y[:, :1])
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(2, 0.15), 0.9], 0.0, False, 0.0)
    eng.upload_candidates(np.zeros((8, 2)))
    with pytest.raises(_lib.BogpError, match="1 target"):
        eng.sweep_ehvi(lo, hi)
    eng.set_train(X[:, :1], Y)  # another width forgets the candidates
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[0.15, 0.9], 0.0, False, 0.0)
    with pytest.raises(_lib.BogpError, match="no candidates"):
        eng.sweep_ehvi(lo3, hi3)
