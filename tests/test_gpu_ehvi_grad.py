"""EHVI and its input gradient at B points on the device (`bogp_point_eval_ehvi`, `bogp_polish_ehvi`; kernels_point_ehvi.hip)
against the NumPy restatement of tests/support/ehvi_grad_ref.py, against `bogp_sweep_ehvi`, and the properties the ABI states:
independence of B, determinism, the clamp edges, the cell cache, the polish's guarantees, the error returns, and
`EHVI(input_gradient=True)` under `optim.argmax_restart` on the real engine.

Shapes: N in {37, 100, 157} (below a row block, not a multiple of 64, just past the small-N fit path), d in {2, 12, 23} (12 columns
in one pass, 22 in one pass, two passes), m in {2, 3, 8}, cells {one cell with every upper bound +inf, a 2-target front of 5 points,
a 3-target front of 16 points = 289 cells (more than the 256 threads), for m = 8 a front of 1 point = 128 cells}, B in {1, 33}, four
correlation kernels, noisy and noiseless models."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bogp import _lib, optim, pareto
from oracle import gp_oracle as O
from support import ehvi_grad_ref as R

import bogp

pytestmark = pytest.mark.gpu

KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP]
BOX = (-2.0, 2.0)


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _cells(Y, m, kind):
    """The cells of a synthetic front between the reference point and the best observations (maximised targets)."""
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    top = Y.max(axis=0)
    if kind == "one":
        return ref[None, :].copy(), np.full((1, m), np.inf)
    P = {"front5": 5, "front16": 16, "front1": 1}[kind]
    t = np.linspace(0.15, 0.85, P)[:, None]
    w = np.hstack([np.repeat(t, m - 1, axis=1), 1.0 - t])  # every coordinate distinct: (P + 1)^(m - 1) cells
    return pareto.hypercell_bounds(ref + w * (top - ref), ref)


def _problem(kernel, noisy, N, d, m, kind, seed=0):
    """(par, mode, X, Y, lower, upper): an m-target model at fixed hyper-parameters, fixed constant trend (as several targets
    require), per-target scales so that the sigma2_k differ."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    if noisy:
        par, mode = np.r_[np.full(d, 0.6 / d), 0.9], _lib.MODE_NOISE_ESTIM
    else:  # (short length scales keep the noiseless R well conditioned)
        par, mode = np.full(d, 200.0 / d), _lib.MODE_NOISELESS
    lo, hi = _cells(Y, m, kind)
    return par, mode, X, Y, lo, hi


def _commit(eng, kernel, par, mode, X, Y):
    eng.set_train(X, Y)
    eng.commit(kernel, mode, par, 0.0, False, 0.0)
    return O.make_state(par, X, Y, kernel, mode, 0.0, beta=0.0)


def _rows(rng, X, B, d):
    """B rows: uniform draws and, among several, one next to a training point."""
    rows = rng.uniform(*BOX, size=(B, d))
    if B > 1:
        rows[-1] = X[1] + 1e-3
    return rows


def _configs():
    """About 40 of the 3 x 3 x 3 x 4 x 2 x 2 product: the 27 (N, d, m) triples with the other axes dealt round, then every kernel
    with both B on the 289-cell front, and the 5-point front at every d."""
    out = []
    kind_of = {2: ("front5", "one"), 3: ("front16", "one"), 8: ("front1", "one")}
    for i, (N, d, m) in enumerate(itertools.product((37, 100, 157), (2, 12, 23), (2, 3, 8))):
        out.append((KERNELS[(i + i // 4) % 4], i % 3 != 2, N, d, m, kind_of[m][(i // 2) % 2], (1, 33)[(i + i // 3) % 2]))
    for kernel, B in itertools.product(KERNELS, (1, 33)):
        out.append((kernel, True, 100, 12, 3, "front16", B))
    for d in (2, 12, 23):
        out.append((_lib.KERNEL_MATERN52, False, 157, d, 2, "front5", 33))
    return out


def _id(c):
    return "k%d-%s-N%d-d%d-m%d-%s-B%d" % (c[0], "noisy" if c[1] else "exact", c[2], c[3], c[4], c[5], c[6])


def _close_values(ehvi, mu, mse, ref, sigma2):
    """T1 / T2 / T12 (README, tolerance ledger)."""
    np.testing.assert_allclose(mu, ref[2], rtol=1e-6, atol=1e-9)
    for k in range(mu.shape[1]):
        np.testing.assert_allclose(mse[:, k], ref[3][:, k], rtol=1e-6, atol=1e-12 * sigma2[k])
    np.testing.assert_allclose(ehvi, ref[0], rtol=1e-6, atol=1e-12 * np.abs(ref[0]).max())


def _excess(a, ref):
    """Largest |a - ref| in units of the allowed rtol 1e-6 |ref| + 1e-12 max|ref| (T14): <= 1 passes."""
    ref = np.asarray(ref)
    return float((np.abs(a - ref) / (1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max() + 1e-300)).max())


@pytest.mark.parametrize("cfg", _configs(), ids=_id)
def test_agrees_with_the_restatement(eng, cfg):
    """Check 1.  Values at T1 / T2 / T12; gradients at rtol 1e-6 beside atol = 1e-12 max|component| of the batch (T14)."""
    kernel, noisy, N, d, m, kind, B = cfg
    par, mode, X, Y, lo, hi = _problem(*cfg[:6], seed=N + d + m)
    st = _commit(eng, kernel, par, mode, X, Y)
    rows = _rows(np.random.default_rng(1), X, B, d)
    ehvi, dehvi, mu, mse, dmu, dmse = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    ref = R.batch(st, rows, lo, hi)
    _close_values(ehvi, mu, mse, ref, st.sigma2)
    assert np.abs(ref[1]).max() > 0  # (a gradient to compare)
    ex = [_excess(dehvi, ref[1]), _excess(dmu, ref[4]), _excess(dmse, ref[5])]
    print("%s cells=%d: gradient errors in units of the tolerance: dehvi %.3g dmu %.3g dmse %.3g" % (_id(cfg), len(lo), *ex))
    assert max(ex) <= 1.0
    # without the moment block the record is the same
    e2, g2 = eng.point_eval_ehvi(rows, lo, hi)
    assert np.array_equal(e2, ehvi) and np.array_equal(g2, dehvi)


@pytest.mark.parametrize("m,kind,d", [(2, "front5", 2), (3, "front16", 12), (8, "front1", 23)])
def test_agrees_with_the_sweep(eng, m, kind, d):
    """Check 2: the value of the B rows against bogp_sweep_ehvi on the same rows, at check 1's tolerance (the summation orders
    differ, no bit identity is claimed)."""
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_MATERN52, True, 157, d, m, kind, seed=3)
    _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rows = _rows(np.random.default_rng(2), X, 33, d)
    ehvi, _, mu, mse, _, _ = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    eng.upload_candidates(rows)
    _, _, vals, smu, smse = eng.sweep_ehvi(lo, hi, return_values=True, return_moments=True)
    np.testing.assert_allclose(ehvi, vals, rtol=1e-6, atol=1e-12 * np.abs(vals).max())
    np.testing.assert_allclose(mu, smu, rtol=1e-6, atol=1e-9)
    sigma2 = eng.get_state(with_C=False)["sigma2"]
    for k in range(m):
        np.testing.assert_allclose(mse[:, k], smse[:, k], rtol=1e-6, atol=1e-12 * sigma2[k])


def _tri_split(N, d, B):
    """`point_tri_geometry` (csrc/kernels_point.hip) restated: workgroups per 64-row block of V."""
    nc = 12 if d + 1 <= 12 else 22
    npass = (d + nc - 2) // (nc - 1)
    wgs = ((N + 63) // 64 + 1) * npass * B
    s = 16 if wgs < 128 else (8 if wgs < 512 else 4)
    return max(1, min(s, (N + 15) // 16))


@pytest.mark.parametrize("N,d", [(37, 2), (100, 12), (157, 23)])
def test_independent_of_B_and_deterministic(eng, N, d):
    """Checks 3 and 4.  N = 37, d = 2 and N = 100, d = 12 run the same row-block split for B = 1 and B = 33 (3 and 7 workgroups per
    block): row b of the batch equals the one-point call bit for bit.  N = 157, d = 23 splits 10-fold for one point and 8-fold for 33:
    there the rows agree to check 1's tolerance."""
    same = _tri_split(N, d, 1) == _tri_split(N, d, 33)
    assert same == ((N, d) != (157, 23))
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_SE, True, N, d, 3, "front16", seed=N)
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    rows = _rows(np.random.default_rng(3), X, 33, d)
    batch = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    again = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))  # identical calls, identical bits
    for b in (0, 7, 32):
        one = eng.point_eval_ehvi(rows[b : b + 1], lo, hi, moments=True)
        one2 = eng.point_eval_ehvi(rows[b : b + 1], lo, hi, moments=True)
        assert all(np.array_equal(a, c) for a, c in zip(one, one2))
        if same:
            assert all(np.array_equal(o[0], a[b]) for o, a in zip(one, batch))
        else:
            assert max(_excess(np.asarray(o[0]), np.asarray(a[b])) for o, a in zip(one, batch)) <= 1.0


def test_large_batches_are_served_in_chunks(eng):
    """More rows than one launch takes (4096 points a chunk): at N = 37, d = 2 the row blocks split 3-fold for every B, so a row's bytes
    do not depend on the chunk it fell into.  Rows at both ends of both chunks equal their one-row calls byte for byte, every array."""
    N, d, m, B = 37, 2, 2, 4100
    assert _tri_split(N, d, 1) == _tri_split(N, d, 4096) == _tri_split(N, d, B - 4096) == 3
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_SE, True, N, d, m, "front5", seed=N)
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    rows = _rows(np.random.default_rng(8), X, B, d)
    batch = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    assert [a.shape for a in batch] == [(B,), (B, d), (B, m), (B, m), (B, m, d), (B, m, d)]
    for b in (0, 4095, 4096, 4099):
        one = eng.point_eval_ehvi(rows[b : b + 1], lo, hi, moments=True)
        assert all(np.ascontiguousarray(o[0]).tobytes() == np.ascontiguousarray(a[b]).tobytes() for o, a in zip(one, batch)), b


def test_clamp_edges(eng):
    """Check 5.  A row ON a training point of a noiseless model: MSE is rounding noise below the 1e-9 clamp, the gradient is finite
    and is the mean path alone.  So it is 1e-6 away from the training point, where MSE is still below the clamp but its gradient is
    not small: without the guard the sd path would dominate.  A row whose every cell factor underflows: value 0 and gradient 0, not NaN."""
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_MATERN52, False, 100, 2, 2, "front5", seed=5)
    _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rows = np.vstack([X[3], X[3] + [1e-6, 0.0], X[3] + 0.05])
    mu = eng.point_eval_ehvi(rows, lo, hi, moments=True)[2]
    # one cell whose lower edge sits a third of the clamped sd (3.2e-5) below the mean there: phi(a) is not small, so dEHVI/dsd is not
    lo, hi = mu[1][None, :] - 1e-5, np.full((1, 2), np.inf)
    ehvi, dehvi, mu, mse, dmu, dmse = eng.point_eval_ehvi(rows, lo, hi, moments=True)
    assert np.all(mse[:2] <= 1e-9) and np.all(mse[2] > 1e-9) and np.all(np.isfinite(dehvi)) and np.all(np.isfinite(ehvi))
    for b in (0, 1):
        _, c_mu, c_sd, sd = R.ehvi_and_coefficients(mu[b], mse[b], lo, hi)
        mean_path = c_mu @ dmu[b]
        sd_path = c_sd @ (dmse[b] / (2.0 * sd[:, None]))  # what the gradient would hold without the clamp's guard
        print("row %d: mean path %s, unguarded sd path %s, device %s" % (b, mean_path, sd_path, dehvi[b]))
        assert np.abs(mean_path).max() > 0
        if b == 1:
            assert np.abs(sd_path).max() > 1e-3 * np.abs(mean_path).max()  # (the check below can tell the two apart)
        assert _excess(dehvi[b], mean_path) <= 1.0
    rows = rows[[0, 2]]
    # cells far above everything the model can reach: a = (l - mu) / sd beyond 38 standard deviations
    far_lo = np.full((3, 2), 1e6) + np.arange(3)[:, None]
    v, g = eng.point_eval_ehvi(rows, far_lo, np.full((3, 2), np.inf))
    assert np.array_equal(v, np.zeros(2)) and np.array_equal(g, np.zeros((2, 2)))
    v, g = eng.point_eval_ehvi(rows, far_lo, far_lo + 1.0)
    assert np.array_equal(v, np.zeros(2)) and np.array_equal(g, np.zeros((2, 2)))


def test_cell_cache(eng):
    """Check 6: two cell sets alternated, a bogp_sweep_ehvi (which writes the same device buffer) in between: every result equals
    that of a fresh handle, bit for bit."""
    par, mode, X, Y, lo_a, hi_a = _problem(_lib.KERNEL_SE, True, 100, 2, 2, "front5", seed=6)
    lo_b, hi_b = _cells(Y, 2, "one")
    lo_c, hi_c = lo_a + 0.01, hi_a + 0.01  # same (m, C), other bytes
    rows = _rows(np.random.default_rng(4), X, 4, 2)
    fresh = {}
    for name, (lo, hi) in dict(a=(lo_a, hi_a), b=(lo_b, hi_b), c=(lo_c, hi_c)).items():
        e = _lib.Engine(0)
        _commit(e, _lib.KERNEL_SE, par, mode, X, Y)
        fresh[name] = e.point_eval_ehvi(rows, lo, hi)
        e.close()
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    eng.upload_candidates(rows)

    def same(name, lo, hi):
        out = eng.point_eval_ehvi(rows, lo, hi)
        return np.array_equal(out[0], fresh[name][0]) and np.array_equal(out[1], fresh[name][1])

    assert same("a", lo_a, hi_a) and same("a", lo_a, hi_a) and same("b", lo_b, hi_b) and same("a", lo_a, hi_a)
    assert same("c", lo_c, hi_c) and same("a", lo_a, hi_a)
    eng.sweep_ehvi(lo_b, hi_b)  # overwrites the resident cells
    assert same("a", lo_a, hi_a)
    eng.sweep_ehvi(lo_c, hi_c)  # same (m, C) as set a
    assert same("a", lo_a, hi_a) and same("b", lo_b, hi_b)
    xs, fs, _ = eng.polish_ehvi(rows, [BOX[0]] * 2, [BOX[1]] * 2, lo_c, hi_c, max_evals=1)
    assert np.array_equal(fs, fresh["c"][0]) and same("a", lo_a, hi_a)


def test_polish(eng):
    """Check 7."""
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_MATERN52, True, 100, 2, 2, "front5", seed=7)
    _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rng = np.random.default_rng(5)
    blo, bhi = np.array([-2.0, -1.5]), np.array([2.0, 1.5])
    starts = rng.uniform(-2.5, 2.5, size=(33, 2))  # some outside the box: clipped first
    clipped = np.clip(starts, blo, bhi)
    f0 = eng.point_eval_ehvi(clipped, lo, hi)[0]
    xs, fs, ne = eng.polish_ehvi(starts, blo, bhi, lo, hi, max_evals=50)
    assert np.all(fs >= f0)  # exact: a start never moves to a worse point
    assert np.all(xs >= blo) and np.all(xs <= bhi) and np.all(ne >= 1) and np.all(ne <= 50)
    again = eng.point_eval_ehvi(xs, lo, hi)[0]
    np.testing.assert_allclose(fs, again, rtol=1e-6, atol=1e-12 * np.abs(again).max())
    assert fs.max() > f0.max()  # (it does climb)
    # the best polished value against the best of a 4096-row sweep
    eng.generate_candidates(blo, bhi, 4096, seed=11)
    best, idx = eng.sweep_ehvi(lo, hi, k=32)
    tx = eng.read_candidates(idx)
    px, pf, _ = eng.polish_ehvi(tx, blo, bhi, lo, hi, max_evals=50)
    print("sweep of 4096 rows: %.9g, polished: %.9g" % (best[0], pf.max()))
    assert pf.max() >= best[0]
    # a degenerate dimension stays put; max_evals = 1 returns the clipped start
    dlo, dhi = np.array([-2.0, 0.25]), np.array([2.0, 0.25])
    xd, fd, _ = eng.polish_ehvi(starts[:5], dlo, dhi, lo, hi, max_evals=30)
    assert np.all(xd[:, 1] == 0.25) and np.all(fd >= eng.point_eval_ehvi(np.clip(starts[:5], dlo, dhi), lo, hi)[0])
    x1, f1, n1 = eng.polish_ehvi(starts, blo, bhi, lo, hi, max_evals=1)
    assert np.array_equal(x1, clipped) and np.array_equal(f1, f0) and np.all(n1 == 1)


def _tiny_forest(m=2):
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])
    return dict(d=2, m=m, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=np.stack([v + k for k in range(m)], axis=1))


def test_error_returns(eng):
    """Check 8: one call per line of the ABI's INVALID / UNSUPPORTED lists (d > BOGP_MAX_DIM cannot be reached: no training set of
    that width can be set); afterwards the handle still sweeps and evaluates as before."""
    lib, dp, ip = eng._lib, C.POINTER(C.c_double), C.POINTER(C.c_int)
    par, mode, X, Y, lo, hi = _problem(_lib.KERNEL_SE, True, 37, 2, 2, "front5", seed=8)
    rows = _rows(np.random.default_rng(6), X, 3, 2)
    blo, bhi = np.full(2, BOX[0]), np.full(2, BOX[1])

    def p(a):
        return None if a is None else np.ascontiguousarray(a, dtype=float).ctypes.data_as(dp)

    def ev(e, Xb=rows, B=3, m=2, Cn=None, lower=lo, upper=hi, out=True):
        v, g = np.empty(max(B, 1)), np.empty((max(B, 1), 2))
        return lib.bogp_point_eval_ehvi(e._h, p(Xb), B, m, len(lower) if Cn is None else Cn, p(lower), p(upper), p(v) if out else None,
                                        p(g), None, None, None, None)

    def po(e, X0=rows, B=3, blo_=blo, bhi_=bhi, m=2, lower=lo, upper=hi, max_evals=5, out=True):
        xo, fo = np.empty((max(B, 1), 2)), np.empty(max(B, 1))
        return lib.bogp_polish_ehvi(e._h, p(X0), B, p(blo_), p(bhi_), m, len(lower), p(lower), p(upper), max_evals, 1e-8, 1e6,
                                    p(xo) if out else None, p(fo), None)

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    fresh = _lib.Engine(0)
    fresh.set_train(X, Y)
    assert ev(fresh) == INV and po(fresh) == INV  # no committed model
    fresh.close()
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    eng.upload_candidates(rows)
    before = eng.point_eval_ehvi(rows, lo, hi)
    sweep_before = eng.sweep_ehvi(lo, hi, return_values=True)[2]
    lo3, hi3 = np.zeros((1, 3)), np.ones((1, 3))
    assert ev(eng, m=3, lower=lo3, upper=hi3) == INV and po(eng, m=3, lower=lo3, upper=hi3) == INV  # m != n_targets
    bad = [(np.array([[np.nan, 0.0]]), np.ones((1, 2))), (np.zeros((1, 2)), np.array([[np.nan, 1.0]])), (np.ones((1, 2)), np.zeros((1, 2)))]
    for l_, u_ in bad:  # non-finite lower, NaN upper, upper below lower
        assert ev(eng, lower=l_, upper=u_) == INV and po(eng, lower=l_, upper=u_) == INV
    assert ev(eng, Cn=0) == INV and ev(eng, Cn=_lib.MAX_EHVI_CELLS + 1) == INV
    assert ev(eng, lower=None, Cn=1) == INV and ev(eng, Xb=None) == INV and ev(eng, out=False) == INV  # null required pointers
    assert po(eng, X0=None) == INV and po(eng, out=False) == INV and po(eng, blo_=None) == INV
    assert ev(eng, B=0) == INV and po(eng, B=0) == INV
    assert po(eng, blo_=bhi, bhi_=blo) == INV  # lo > hi
    assert po(eng, max_evals=0) == INV
    # a model of ONE target: m < 2
    one = _lib.Engine(0)
    one.set_train(X, Y[:, :1])
    one.commit(_lib.KERNEL_SE, mode, par, 0.0, False, 0.0)
    assert ev(one, m=1, lower=lo[:, :1], upper=hi[:, :1]) == INV and ev(one, m=2) == INV
    # ... and with a linear trend basis: unsupported
    one.commit(_lib.KERNEL_SE, mode, par, 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    assert ev(one, m=1, lower=lo[:, :1], upper=hi[:, :1]) == UNS and po(one, m=1, lower=lo[:, :1], upper=hi[:, :1]) == UNS
    one.close()
    # kernels without corr_dx
    k2 = _lib.Engine(0)
    k2.set_train(X, Y)
    k2.commit(_lib.KERNEL_MATERN_NU, _lib.MODE_NOISELESS, np.r_[np.full(2, 100.0), 1.7], 0.0, False, 0.0)
    assert ev(k2) == UNS and po(k2) == UNS
    k2.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISELESS, np.full(2, 100.0), 0.0, False, 0.0)
    assert ev(k2) == UNS and po(k2) == UNS
    k2.close()
    # a forest on the handle
    fo = _lib.Engine(0)
    fo.forest_set_multi(**_tiny_forest())
    assert ev(fo) == UNS and po(fo) == UNS
    fo.close()
    # the handle is as it was: active target, candidates, sweeps, the evaluation itself
    after = eng.point_eval_ehvi(rows, lo, hi)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert np.array_equal(eng.sweep_ehvi(lo, hi, return_values=True)[2], sweep_before)
    mu1, _ = eng.predict()
    eng.select_target(1)
    eng.point_eval_ehvi(rows, lo, hi)
    assert not np.array_equal(eng.predict()[0], mu1)  # still target 1
    eng.select_target(0)
    assert np.array_equal(eng.predict()[0], mu1)


@pytest.mark.parametrize("optimizer", ["sweep-device-BFGS", "BFGS"])
def test_criterion_on_the_real_engine(optimizer):
    """Check 9: `EHVI(input_gradient=True)` under the polish hybrid and under the reference-style loop on a 2-d problem, against
    "sweep-device" with the same seed and budget."""
    rng = np.random.default_rng(9)
    X = rng.uniform(*BOX, size=(30, 2))
    Y = np.sin(X @ rng.normal(size=(2, 2))) * (1.0 + np.arange(2)) + 0.3 * rng.normal(size=(30, 2))
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(2, beta=0.0), corr="matern", thetaL=[1e-3] * 2, thetaU=[1e2] * 2, nugget=1e-6)
    model.set_state(np.r_[0.3, 0.3, 0.9], X, Y)
    ref = Y.min(axis=0) - 0.1 * np.abs(Y.min(axis=0))
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, input_gradient=True)
    v, g = crit(X[:1] + 0.1, return_dx=True)
    assert v.shape == (1,) and g.shape == (1, 2)
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, optimizer="sweep-device")
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, n_restart=10, optimizer=optimizer)
    print("%s: sweep-device %.9g, result %.9g" % (optimizer, fs, fp))
    assert fp >= fs and all(BOX[0] <= t <= BOX[1] for t in xp)
    model.engine.close()
