"""The feasibility-weighted criteria and their input gradients at B points on the device (`bogp_point_eval_constrained`,
`bogp_polish_constrained`; kernels_point_constrained.hip) against the NumPy restatement of tests/support/constrained_grad_ref.py,
against `bogp_sweep_constrained`, and the properties the ABI states: independence of B, of the launch and of the other criteria, the
exact cases (every bound infinite, lo == hi, the guards), the polish's guarantees, `Constrained(input_gradient=True)` under
`optim.argmax_restart` on the real engine, `feasibility_grad` on the device against the exact table G47, and the error returns.

Shapes are tests/test_gpu_ehvi_grad.py's: N in {37, 100, 157} (below a row block, not a multiple of 64, just past the one-launch fit),
d in {2, 12, 23} (12 columns in one pass, 22 in one pass, two passes), m in {2, 3, 8}, B in {1, 33}, four correlation kernels, noisy and
noiseless models; every call has q = 4: EI, EpsilonPI 0.05, MGFI t = 2 and the probability of feasibility alone.  The bounds rotate
through (-inf, median], [q40, q60], [q90, +inf) and [-tol, tol] of the training columns.  d = 2 takes short length scales in the noisy
mode: with long ones the variance bracket clips to 0 on most rows (P in {0, 1}, a zero gradient), which is check (e)'s state."""
import ctypes as C
import itertools

import numpy as np
import pytest

import feasibility_grad_cases as FG
from bogp import _lib, optim
from conftest import load_golden
from oracle import gp_oracle as O
from support import constrained_grad_ref as R

import bogp

pytestmark = pytest.mark.gpu

KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP]
ACQ4 = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_EPSILON_PI, 0.05), (_lib.ACQ_MGFI, 2.0), (_lib.ACQ_NONE, 0.0)]
BOX = (-2.0, 2.0)
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _bounds(Y, first=0):
    """The four kinds in rotation over the constraint columns, as quantiles of the training column."""
    lo, hi = [], []
    for k in range(1, Y.shape[1]):
        col = Y[:, k]
        kind = (first + k - 1) % 4
        if kind == 0:
            lo.append(-INF), hi.append(float(np.median(col)))
        elif kind == 1:
            lo.append(float(np.quantile(col, 0.4))), hi.append(float(np.quantile(col, 0.6)))
        elif kind == 2:
            lo.append(float(np.quantile(col, 0.9))), hi.append(INF)
        else:
            tol = 0.3 * float(col.std())
            lo.append(-tol), hi.append(tol)
    return np.array(lo), np.array(hi)


def _problem(kernel, noisy, N, d, m, first=0, seed=0, theta=None):
    """(par, mode, X, Y, lo, hi, plugin): an m-target model at fixed hyper-parameters, fixed constant trend (as several targets require),
    per-target scales so that the sigma2_k differ; plugin the median of the objective column (EI is alive on about half the box)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.sin(X @ rng.normal(size=(d, m))) * (1.0 + np.arange(m)) + 0.3 * rng.normal(size=(N, m))
    if noisy:
        par, mode = np.r_[np.full(d, theta or (10.0 if d == 2 else 0.6 / d)), 0.9], _lib.MODE_NOISE_ESTIM
    else:  # (short length scales keep the noiseless R well conditioned)
        par, mode = np.full(d, theta or 200.0 / d), _lib.MODE_NOISELESS
    lo, hi = _bounds(Y, first)
    return par, mode, X, Y, lo, hi, float(np.median(Y[:, 0]))


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
    """About 40 of the product, dealt round as tests/test_gpu_ehvi_grad.py deals them: the 27 (N, d, m) triples with kernel, mode, first
    bound kind, direction and B in rotation, then every kernel with both B at N = 100, d = 12, m = 3, and a noiseless model at every d."""
    out = []
    for i, (N, d, m) in enumerate(itertools.product((37, 100, 157), (2, 12, 23), (2, 3, 8))):
        out.append((KERNELS[(i + i // 4) % 4], i % 3 != 2, N, d, m, i % 4, i % 5 != 3, (1, 33)[(i + i // 3) % 2]))
    for kernel, B in itertools.product(KERNELS, (1, 33)):
        out.append((kernel, True, 100, 12, 3, 1, True, B))
    for d in (2, 12, 23):
        out.append((_lib.KERNEL_MATERN52, False, 157, d, 2, 2, False, 33))
    return out


def _id(c):
    return "k%d-%s-N%d-d%d-m%d-b%d-%s-B%d" % (c[0], "noisy" if c[1] else "exact", c[2], c[3], c[4], c[5], "min" if c[6] else "max", c[7])


def _case(cfg):
    kernel, noisy, N, d, m, first, minimize, B = cfg
    par, mode, X, Y, lo, hi, plugin = _problem(kernel, noisy, N, d, m, first, seed=N + d + m)
    return par, mode, X, Y, lo, hi, (plugin if minimize else -plugin), _rows(np.random.default_rng(1), X, B, d)


def _t19(v, ref):
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    assert np.all(np.abs(v - ref) <= 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()), np.abs(v - ref).max()


def _close_values(acq, pof, mu, mse, ref, sigma2):
    """T1 / T2 / T19 (README, tolerance ledger)."""
    np.testing.assert_allclose(mu, ref[4], rtol=1e-6, atol=1e-9)
    for k in range(mu.shape[1]):
        np.testing.assert_allclose(mse[:, k], ref[5][:, k], rtol=1e-6, atol=1e-12 * sigma2[k])
    _t19(pof, ref[2])
    for c in range(acq.shape[1]):
        _t19(acq[:, c], ref[0][:, c])


def _excess(a, ref):
    """Largest |a - ref| in units of the allowed rtol 1e-6 |ref| + 1e-12 max|ref| (T14), over the entries where `ref` is finite: <= 1 passes."""
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    ok = np.isfinite(ref)
    assert np.all(np.isfinite(a[ok]))  # no NaN anywhere the restatement is finite
    scale = np.abs(ref[ok]).max() if ok.any() else 0.0
    return float((np.abs(a[ok] - ref[ok]) / (1e-6 * np.abs(ref[ok]) + 1e-12 * scale + 1e-300)).max()) if ok.any() else 0.0


def condition_on_the_inputs(ref):
    """From the restatement alone: the fraction of rows on which every MSE_k > 0, 0 < P and each of the four criteria has a non-zero
    gradient.  A configuration needs at least half."""
    alive = np.all(ref[5] > 0, axis=1) & (ref[2] > 0) & np.all(np.abs(ref[1]).max(axis=2) > 0, axis=1)
    return float(alive.mean())


@pytest.mark.parametrize("cfg", _configs(), ids=_id)
def test_agrees_with_the_restatement(eng, cfg):
    """Check (a).  Values, P, mu, MSE at T1 / T2 / T19; dacq, dpof, dmu, dmse at rtol 1e-6 beside atol = 1e-12 max|component| of the batch
    (T14).  Measured on an MI355X over the 38 configurations: see the ledger row T22 of the README."""
    kernel, noisy, N, d, m, first, minimize, B = cfg
    par, mode, X, Y, lo, hi, plugin, rows = _case(cfg)
    st = _commit(eng, kernel, par, mode, X, Y)
    ref = R.batch(st, rows, lo, hi, ACQ4, plugin, minimize)
    assert condition_on_the_inputs(ref) >= 0.5
    acq, dacq, pof, dpof, mu, mse, dmu, dmse = eng.point_eval_constrained(rows, ACQ4, plugin, minimize, lo, hi, moments=True)
    _close_values(acq, pof, mu, mse, ref, st.sigma2)
    ex = [_excess(dacq, ref[1]), _excess(dpof, ref[3]), _excess(dmu, ref[6]), _excess(dmse, ref[7])]
    print("%s: gradient errors in units of the tolerance: dacq %.3g dpof %.3g dmu %.3g dmse %.3g" % (_id(cfg), *ex))
    assert max(ex) <= 1.0
    assert np.array_equal(dacq[:, 3], dpof) and np.array_equal(acq[:, 3], pof)  # feasibility only: P and dP/dx themselves
    # without the second block the record is the same
    a2, g2 = eng.point_eval_constrained(rows, ACQ4, plugin, minimize, lo, hi)
    assert np.array_equal(a2, acq) and np.array_equal(g2, dacq)


@pytest.mark.parametrize("m,d,first", [(2, 2, 0), (3, 12, 1), (8, 23, 2)])
def test_agrees_with_the_sweep(eng, m, d, first):
    """Check (b): the B rows against bogp_sweep_constrained on the same rows uploaded as candidates, at T1 / T2 / T19 (the two paths sum
    in different orders: no bit identity is claimed)."""
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_MATERN52, True, 157, d, m, first, seed=3)
    _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rows = _rows(np.random.default_rng(2), X, 33, d)
    acq, _, pof, _, mu, mse, _, _ = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    eng.upload_candidates(rows)
    _, _, vals, spof, smu, smse = eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True, return_pof=True, return_moments=True)
    for c in range(4):
        _t19(acq[:, c], vals[c])
    _t19(pof, spof)
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
def test_bits(eng, N, d):
    """Check (c).  N = 37, d = 2 and N = 100, d = 12 run the same row-block split for B = 1 and B = 33: row b of the batch equals the
    one-point call bit for bit; N = 157, d = 23 splits 10-fold for one point and 8-fold for 33, so there the rows agree to check (a)'s
    tolerance.  Identical calls give identical bytes, and a criterion's bytes do not depend on the criteria it shares the call with."""
    same = _tri_split(N, d, 1) == _tri_split(N, d, 33)
    assert same == ((N, d) != (157, 23))
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_SE, True, N, d, 3, 1, seed=N)
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    rows = _rows(np.random.default_rng(3), X, 33, d)
    batch = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    again = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))  # identical calls, identical bytes
    for b in (0, 7, 32):
        one = eng.point_eval_constrained(rows[b : b + 1], ACQ4, plugin, True, lo, hi, moments=True)
        one2 = eng.point_eval_constrained(rows[b : b + 1], ACQ4, plugin, True, lo, hi, moments=True)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(one, one2))
        if same:
            assert all(np.array_equal(o[0], a[b]) for o, a in zip(one, batch))
        else:
            assert max(_excess(np.asarray(o[0]), np.asarray(a[b])) for o, a in zip(one, batch)) <= 1.0
    for c, crit in enumerate(ACQ4):  # criterion c alone: its value and gradient bytes are those of the q = 4 call
        for r_, B in ((rows, 33), (rows[:1], 1)):
            a1, g1 = eng.point_eval_constrained(r_, [crit], plugin, True, lo, hi)
            full = eng.point_eval_constrained(r_, ACQ4, plugin, True, lo, hi)
            assert a1[:, 0].tobytes() == np.ascontiguousarray(full[0][:, c]).tobytes()
            assert g1[:, 0].tobytes() == np.ascontiguousarray(full[1][:, c]).tobytes()


def test_large_batches_are_served_in_chunks(eng):
    """More rows than one launch takes (4096 points a chunk): at N = 37, d = 2 the row blocks split 3-fold for every B, so a row's bytes
    do not depend on the chunk it fell into.  Rows at both ends of both chunks equal their one-row calls byte for byte, every array."""
    N, d, m, B = 37, 2, 3, 4100
    assert _tri_split(N, d, 1) == _tri_split(N, d, 4096)
    assert _tri_split(N, d, 4096) == _tri_split(N, d, B - 4096)
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_SE, True, N, d, m, 1, seed=N)
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    rows = _rows(np.random.default_rng(8), X, B, d)
    batch = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    assert [a.shape for a in batch] == [(B, 4), (B, 4, d), (B,), (B, d), (B, m), (B, m), (B, m, d), (B, m, d)]
    for b in (0, 4095, 4096, 4099):
        one = eng.point_eval_constrained(rows[b : b + 1], ACQ4, plugin, True, lo, hi, moments=True)
        assert all(np.ascontiguousarray(o[0]).tobytes() == np.ascontiguousarray(a[b]).tobytes() for o, a in zip(one, batch)), b


@pytest.mark.parametrize("kernel,N,d,m,B", [(_lib.KERNEL_MATERN52, 100, 12, 3, 33), (_lib.KERNEL_SE, 37, 2, 2, 1), (_lib.KERNEL_ABSEXP, 157, 23, 8, 33)])
def test_all_bounds_infinite(eng, kernel, N, d, m, B):
    """Check (d): P = 1.0 and dpof = 0 exactly; acq / dacq equal bogp_point_eval_batch on a model committed on column 0 alone at rtol 1e-6."""
    par, mode, X, Y, _, _, plugin = _problem(kernel, True, N, d, m, seed=11 + N)
    rows = _rows(np.random.default_rng(4), X, B, d)
    _commit(eng, kernel, par, mode, X, Y)
    lo, hi = np.full(m - 1, -INF), np.full(m - 1, INF)
    acq, dacq, pof, dpof = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)[:4]
    assert np.array_equal(pof, np.ones(B)) and np.array_equal(dpof, np.zeros((B, d)))
    assert np.array_equal(acq[:, 3], np.ones(B)) and np.array_equal(dacq[:, 3], np.zeros((B, d)))
    eng.set_train(X, Y[:, :1])
    eng.commit(kernel, mode, par, 0.0, False, 0.0)
    _, _, _, _, vals, dvals = eng.point_eval_batch(rows, ACQ4[:3], plugin, True, return_dx=True)
    ok = np.isfinite(dvals)  # (next to a training point MSE_0 clips to 0, where the single-target call returns the reference's 0 / 0 for EpsilonPI)
    assert ok.mean() > 0.9 and np.abs(dvals[ok]).max() > 0 and np.all(np.isfinite(dacq))
    np.testing.assert_allclose(acq[:, :3], vals, rtol=1e-6, atol=0)
    np.testing.assert_allclose(dacq[:, :3][ok], dvals[ok], rtol=1e-6, atol=0)


def test_guards(eng):
    """Check (e).  A row ON a training point of a noiseless model: the variance is rounding noise inside the small-variance guard
    (MSE < 1e-12 sigma2), so P is the indicator of the bounds at the observed values, dpof is exactly 0 and EI is exactly 0 with a zero
    gradient.  The noisy d = 2 state with long length scales: MSE clips to exactly 0 on most rows -- P in {0, 1}, every gradient exactly
    0.  lo == hi: value and gradient exactly 0.  No NaN anywhere the restatement is finite (and none at all in the values)."""
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_MATERN52, False, 100, 2, 3, 0, seed=5)
    st = _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    feasible = np.all((Y[:, 1:] >= lo + 0.05) & (Y[:, 1:] <= hi - 0.05), axis=1)  # (clear of the bounds: the indicator is not a rounding matter)
    outside = ~np.all((Y[:, 1:] >= lo - 0.05) & (Y[:, 1:] <= hi + 0.05), axis=1)
    pick = [int(np.flatnonzero(feasible)[0]), int(np.flatnonzero(outside)[0])]
    rows = np.vstack([X[pick[0]], X[pick[1]], X[pick[0]] + 0.05])
    acq, dacq, pof, dpof, mu, mse, dmu, dmse = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    sigma2 = np.asarray(st.sigma2).ravel()
    print("guards: MSE / sigma2 on two training points %s, next to one %s" % (mse[:2] / sigma2, mse[2] / sigma2))
    assert np.all(mse[:2] < 1e-12 * sigma2) and np.all(mse[2] > 1e-12 * sigma2)
    for b in (0, 1):
        assert np.abs(Y[pick[b], 1:] - mu[b, 1:]).max() < 1e-6 and pof[b] == (1.0, 0.0)[b]
        assert np.array_equal(dpof[b], np.zeros(2))
        assert acq[b, 0] == 0.0 and np.array_equal(dacq[b, 0], np.zeros(2))  # EI's guard
        assert acq[b, 2] == 0.0 and np.array_equal(dacq[b, 2], np.zeros(2))  # MGFI's (np.isclose(sd, 0))
        assert acq[b, 3] == pof[b] and np.array_equal(dacq[b, 3], np.zeros(2))
    assert 0 < pof[2] < 1 and np.abs(dpof[2]).max() > 0 and np.all(np.isfinite(dacq)) and np.all(np.isfinite(acq))
    assert np.array_equal(dacq[0, 1], np.zeros(2))  # EpsilonPI on a training point: a step in mu, coefficients taken as 0
    ref = R.batch(st, rows, lo, hi, ACQ4, plugin, True)
    assert _excess(dacq, ref[1]) <= 1.0 and _excess(dpof, ref[3]) <= 1.0
    # lo == hi on one constraint: F = 0 exactly
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1] = hi2[1] = float(np.median(Y[:, 2]))
    acq, dacq, pof, dpof = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo2, hi2, moments=True)[:4]
    assert np.array_equal(acq, np.zeros((3, 4))) and np.array_equal(dacq, np.zeros((3, 4, 2)))
    assert np.array_equal(pof, np.zeros(3)) and np.array_equal(dpof, np.zeros((3, 2)))
    # the clipped state
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_MATERN52, True, 37, 2, 3, 0, seed=6, theta=0.3)
    st = _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rows = _rows(np.random.default_rng(7), X, 33, 2)
    acq, dacq, pof, dpof, mu, mse, dmu, dmse = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi, moments=True)
    clipped = np.all(mse == 0.0, axis=1)
    print("clipped state: %d of 33 rows have MSE = 0 exactly" % clipped.sum())
    assert clipped.sum() >= 8
    assert np.all(np.isin(pof[clipped], (0.0, 1.0))) and np.array_equal(dpof[clipped], np.zeros((clipped.sum(), 2)))
    assert np.array_equal(dacq[clipped], np.zeros((clipped.sum(), 4, 2))) and np.all(np.isfinite(acq)) and np.all(np.isfinite(dacq))
    assert np.array_equal(acq[clipped, 0], np.zeros(clipped.sum()))
    ref = R.batch(st, rows, lo, hi, ACQ4, plugin, True)
    assert _excess(dacq, ref[1]) <= 1.0 and _excess(dpof, ref[3]) <= 1.0


def test_polish(eng):
    """Check (f)."""
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_MATERN52, False, 100, 2, 3, 0, seed=7, theta=20.0)
    _commit(eng, _lib.KERNEL_MATERN52, par, mode, X, Y)
    rng = np.random.default_rng(5)
    blo, bhi = np.array([-2.0, -1.5]), np.array([2.0, 1.5])
    starts = rng.uniform(-2.5, 2.5, size=(32, 2))  # some outside the box: clipped first
    # a start ON a training point that violates a constraint: inside the guard, so P = 0 exactly with a zero gradient
    inside_box = np.all((X >= blo) & (X <= bhi), axis=1)
    bad = np.flatnonzero(inside_box & ~np.all((Y[:, 1:] >= lo - 0.2) & (Y[:, 1:] <= hi + 0.2), axis=1))[0]
    starts[5] = X[bad]
    clipped = np.clip(starts, blo, bhi)
    crit = ACQ4[0]
    f0, g0, p0 = eng.point_eval_constrained(clipped, [crit], plugin, True, lo, hi, moments=True)[:3]
    assert p0[5] == 0.0 and np.array_equal(g0[5, 0], np.zeros(2)) and f0[5, 0] == 0.0  # (the condition on that start)
    xs, fs, ne = eng.polish_constrained(starts, blo, bhi, crit, plugin, True, lo, hi, max_evals=50)
    assert np.all(fs >= f0[:, 0])  # exact: a start never moves to a worse point
    assert np.all(xs >= blo) and np.all(xs <= bhi) and np.all(ne >= 1) and np.all(ne <= 50)
    again = eng.point_eval_constrained(xs, [crit], plugin, True, lo, hi)[0][:, 0]
    assert fs.tobytes() == again.tobytes()  # fout is the value AT Xout, bit for bit
    print("polish: %d of 32 starts improved; best start %.6g -> best result %.6g" % ((fs > f0[:, 0]).sum(), f0.max(), fs.max()))
    assert np.any(fs > f0[:, 0])  # at least one start improves strictly
    assert np.array_equal(xs[5], clipped[5]) and fs[5] == 0.0  # P = 0 exactly, zero gradient: it does not move
    # max_evals = 1 returns the clipped starts
    x1, f1, n1 = eng.polish_constrained(starts, blo, bhi, crit, plugin, True, lo, hi, max_evals=1)
    assert np.array_equal(x1, clipped) and np.array_equal(f1, f0[:, 0]) and np.all(n1 == 1)


def test_criterion_on_the_real_engine():
    """Check (g): `Constrained(input_gradient=True)` under the polish hybrid against "sweep-device" with the same seed and budget: the
    polish starts from the sweep's top k, so f >= (1 - 1e-6) x the sweep's best (the margin is for the two summation orders only)."""
    rng = np.random.default_rng(9)
    X = rng.uniform(*BOX, size=(30, 2))
    Y = np.sin(X @ rng.normal(size=(2, 2))) * (1.0 + np.arange(2)) + 0.3 * rng.normal(size=(30, 2))
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(2, beta=0.0), corr="matern", thetaL=[1e-3] * 2, thetaU=[1e2] * 2, nugget=1e-6)
    model.set_state(np.r_[10.0, 10.0, 0.9], X, Y)
    crit = bogp.Constrained(model=model, fun="EI", input_gradient=True, lo=[-INF], hi=[float(np.median(Y[:, 1]))])
    v, g = crit(X[:1] + 0.1, return_dx=True)
    assert v.shape == (1,) and g.shape == (1, 2) and np.all(np.isfinite(g))
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, optimizer="sweep-device")
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, n_restart=10, optimizer="sweep-device-BFGS")
    print("sweep-device %.9g, sweep-device-BFGS %.9g" % (fs, fp))
    assert fs > 0 and fp >= (1 - 1e-6) * fs and all(BOX[0] <= t <= BOX[1] for t in xp)
    model.engine.close()


def test_feasibility_grad_on_the_device_against_the_table(eng):
    """Check (h): `bogp_selftest_feasibility_grad` against G47 with the allowance and F of the host check (ledger T21)."""
    g = load_golden("G47_feasibility_grad_truth")
    c = FG.draw()
    out = eng.selftest_feasibility_grad(c["mu"], c["mse"], c["sigma2"], c["lo"], c["hi"])
    F0 = eng.selftest_criteria(_lib.CRITERIA_FEASIBILITY, c["mu"], c["mse"], c["sigma2"], c["lo"], c["hi"])
    assert out[:, 0].tobytes() == F0.tobytes()
    for j, name in enumerate(FG.NAMES):
        r, cmp = FG.ratios(out[:, 1 + j], g[name + "_true"], g[name + "_rlo"], FG.allowance(name, c))
        print("T21 %s device: worst |value - exact| / allowance = %.4g over %d rows (F = %d)" % (name, r.max(), cmp.sum(), FG.F[name]))
        assert r.max() <= FG.F[name] and FG.tiny_rows_ok(out[:, 1 + j], cmp)
    edge = eng.selftest_feasibility_grad([0.5, 1.5, 0.3, 0.3, 0.3], [1e-14, 1e-14, 0.25, 0.25, 0.0], 1.0, [0.0, 0.0, -INF, 0.1, -INF],
                                         [1.0, 1.0, INF, 0.1, 0.0])  # fmt: skip
    assert np.array_equal(edge, [[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]])


def _tiny_forest(m=2):
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])
    return dict(d=2, m=m, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=np.stack([v + k for k in range(m)], axis=1))


def test_error_returns(eng):
    """Check (i): one call per line of the ABI's INVALID / UNSUPPORTED lists; afterwards the handle still sweeps and evaluates as before."""
    lib, dp, ip = eng._lib, C.POINTER(C.c_double), C.POINTER(C.c_int)
    par, mode, X, Y, lo, hi, plugin = _problem(_lib.KERNEL_SE, True, 37, 2, 2, 0, seed=8)
    rows = _rows(np.random.default_rng(6), X, 3, 2)
    blo, bhi = np.full(2, BOX[0]), np.full(2, BOX[1])

    def p(a):
        return None if a is None else np.ascontiguousarray(a, dtype=float).ctypes.data_as(dp)

    def ev(e, Xb=rows, B=3, ids=(_lib.ACQ_EI,), pars=(0.0,), n_con=1, lo_=lo, hi_=hi, out=True):
        q = len(ids)
        v, g = np.empty((max(B, 1), q)), np.empty((max(B, 1), q, 2))
        idv = np.ascontiguousarray(ids, dtype=np.int32)
        return lib.bogp_point_eval_constrained(e._h, p(Xb), B, q, idv.ctypes.data_as(ip), p(pars), plugin, 1, n_con, p(lo_), p(hi_),
                                               p(v) if out else None, p(g), None, None, None, None, None, None)

    def po(e, X0=rows, B=3, blo_=blo, bhi_=bhi, acq_id=_lib.ACQ_EI, n_con=1, lo_=lo, hi_=hi, max_evals=5, out=True):
        xo, fo = np.empty((max(B, 1), 2)), np.empty(max(B, 1))
        return lib.bogp_polish_constrained(e._h, p(X0), B, p(blo_), p(bhi_), acq_id, 0.5, plugin, 1, n_con, p(lo_), p(hi_), max_evals, 1e-8,
                                           1e6, p(xo) if out else None, p(fo), None)

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    fresh = _lib.Engine(0)
    fresh.set_train(X, Y)
    assert ev(fresh) == INV and po(fresh) == INV  # no committed model
    fresh.close()
    _commit(eng, _lib.KERNEL_SE, par, mode, X, Y)
    eng.upload_candidates(rows)
    before = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi)
    sweep_before = eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True)[2]
    two = np.array([-INF, -INF]), np.array([0.0, 0.0])
    assert ev(eng, n_con=2, lo_=two[0], hi_=two[1]) == INV and po(eng, n_con=2, lo_=two[0], hi_=two[1]) == INV  # wrong n_con
    assert ev(eng, n_con=0) == INV and po(eng, n_con=0) == INV
    assert ev(eng, ids=(_lib.ACQ_UCB,), pars=(0.5,)) == INV and po(eng, acq_id=_lib.ACQ_UCB) == INV  # UCB
    assert ev(eng, ids=(7,)) == INV and ev(eng, ids=(-2,)) == INV and po(eng, acq_id=7) == INV  # unknown id
    assert ev(eng, ids=(_lib.ACQ_MGFI,), pars=(0.0,)) == INV and ev(eng, ids=(_lib.ACQ_EPSILON_PI,), pars=(-1.0,)) == INV  # refused parameters
    assert ev(eng, ids=()) == INV  # q < 1
    for l_, h_ in (([np.nan], [0.0]), ([0.0], [np.nan]), ([1.0], [0.0])):  # NaN bounds, hi < lo
        assert ev(eng, lo_=l_, hi_=h_) == INV and po(eng, lo_=l_, hi_=h_) == INV
    assert ev(eng, lo_=[0.5], hi_=[0.5]) == 0  # (hi == lo is allowed)
    assert ev(eng, Xb=None) == INV and ev(eng, out=False) == INV and ev(eng, lo_=None) == INV and ev(eng, hi_=None) == INV  # null pointers
    assert po(eng, X0=None) == INV and po(eng, out=False) == INV and po(eng, blo_=None) == INV and po(eng, lo_=None) == INV
    assert ev(eng, B=0) == INV and po(eng, B=0) == INV and ev(eng, B=-1) == INV
    assert po(eng, blo_=bhi, bhi_=blo) == INV and po(eng, max_evals=0) == INV
    # a model of ONE target
    one = _lib.Engine(0)
    one.set_train(X, Y[:, :1])
    one.commit(_lib.KERNEL_SE, mode, par, 0.0, False, 0.0)
    assert ev(one) == INV and po(one) == INV and ev(one, n_con=0) == INV
    # ... and with a linear trend basis: unsupported
    one.commit(_lib.KERNEL_SE, mode, par, 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    assert ev(one, n_con=0) == UNS and po(one, n_con=0) == UNS
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
    # the selftest entry
    assert lib.bogp_selftest_feasibility_grad(eng._h, None, 1, p(np.empty(3))) == INV
    assert lib.bogp_selftest_feasibility_grad(eng._h, p(np.zeros(5)), 0, p(np.empty(3))) == INV
    # the handle is as it was: active target, candidates, sweeps, the evaluation itself
    after = eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert eng.sweep_constrained(ACQ4, plugin, True, lo, hi, return_values=True)[2].tobytes() == sweep_before.tobytes()
    mu1, _ = eng.predict()
    eng.select_target(1)
    eng.point_eval_constrained(rows, ACQ4, plugin, True, lo, hi)
    eng.polish_constrained(rows, blo, bhi, ACQ4[0], plugin, True, lo, hi, max_evals=3)
    assert not np.array_equal(eng.predict()[0], mu1)  # still target 1
    eng.select_target(0)
    assert np.array_equal(eng.predict()[0], mu1)
    best, idx = eng.sweep([(_lib.ACQ_EI, 0.0)], plugin, True)  # a single-target sweep on the active target still runs
    assert np.isfinite(best[0]) and 0 <= idx[0] < 3
