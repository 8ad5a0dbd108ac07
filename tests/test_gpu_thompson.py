"""Thompson-sampling batches on the device (`bogp_sweep_thompson`, kernels_thompson.hip) against the dense NumPy restatement
`bogp.thompson.paths_numpy` on the SAME draw: values and coefficients over a covering selection of 40 shapes (M, d, N, L, q around
every tile edge of the kernel and both sides of the N <= 512 sweep routing), the six served kernels and both kriging flavours;
the winners for k = 1 and k = 16, minimising and maximising, a NaN candidate row included; bit-identity across chunkings, across q,
of the prior paths, and of a plain sweep before and after; candidate sources; every error return but one.

Tolerance (values): |dev - ref| <= ptol (|ref| + A) with ptol = max(1e-6, 100 cond(R) eps) (ledger T5) and A the sum of the
ABSOLUTE terms of the restated sum, sqrt(2 sigma2 / L) sum_l |W_lj| + sum_n |r_n gt_nj| + |mu| + |bt_j| -- the rounding scale of a
signed sum that crosses zero (T1 / T12's reason).  Two conditions keep the restatement itself inside it and are asserted per case:
cond(R) <= 1e8 and max(sum_i |omega_i x_i| + |b|) <= 1e6 (the phase's own rounding, (d + 2) eps 1e6 ~ 4e-9, stays far below
1e-6).  The coefficients are held the same way against the absolute terms of THEIR sums: gt = R^-1 (s - bt 1) against
sum_m |R^-1_nm| (S_j + |bt_j|), bt against sum_m |w_m| S_j / |sum w|, S_j the first term of A.  A wrong lane map, k order or
padding moves a value by A / L or more, 1e3 above the tolerance.  The largest excess ratio measured over the 40 shapes is in
profiles/thompson_parity.txt (README ledger T16)."""
import ctypes as C

import numpy as np
import pytest

from bogp import _lib, thompson
from support.chunk_mb import with_chunk_mb as _with_chunk_mb
from support.thompson_engine import ranking

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP, _lib.KERNEL_MATERN_NU]
HEAVY = (_lib.KERNEL_MATERN12, _lib.KERNEL_ABSEXP, _lib.KERNEL_MATERN_NU)  # spectral draws with Cauchy-like tails
NU = 0.8
MS, DS, NS, LS, QS = [1, 15, 16, 17, 63, 64, 65, 1000], [1, 3, 4, 5, 20, 33], [5, 64, 67, 300, 600], [16, 48, 1024], [1, 2, 15, 16]
# 40 shapes: every value of every parameter several times, in changing company (strides chosen so that no two lists move together)
CONFIGS = [(MS[i % 8], DS[(i + i // 8) % 6], NS[i % 5], LS[(i // 2) % 3], QS[(i // 3) % 4], KERNELS[(i + i // 6) % 6], bool((i // 4) % 2))
           for i in range(40)]  # fmt: skip


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def problem(M, d, N, kernel, seed=0):
    """(X, y, theta, candidates).  The smooth kernels get the length scale at which a nearest neighbour correlates at about
    exp(-1) (exp(-3) for the squared exponential) -- r(x) matters and R stays well conditioned; the three with heavy-tailed spectra theta = 1 / d, which keeps their
    phases small (their R is well conditioned at any scale).  The first candidates sit 0.01 off training rows."""
    rng = np.random.default_rng(1000 * N + 10 * d + seed)
    X = rng.uniform(-2, 2, size=(N, d))
    y = 2 * np.sin(X @ rng.normal(size=d) / np.sqrt(d)) + 0.1 * rng.normal(size=N)
    nn = 4.0 / N ** (1.0 / d)  # spacing of N points in the box, per dimension
    theta = np.full(d, 1.0 / d) if kernel in HEAVY else np.full(d, (3.0 if kernel == _lib.KERNEL_SE else 1.0) / (d * nn * nn))
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    n_near = min(M, N, 8)
    Xs[:n_near] = X[:n_near] + 0.01
    return X, y, theta, Xs


def commit(eng, X, y, theta, kernel, est):
    eng.set_train(X, y)
    eng.commit(kernel, _lib.MODE_NOISELESS, np.r_[theta, NU] if kernel == _lib.KERNEL_MATERN_NU else theta, 0.0, est, 0.3)
    s = eng.get_state(with_C=False)
    return thompson.dense_state(X, y, theta, kernel, est, beta=float(np.ravel(s["beta"])[0]), nu=NU if kernel == _lib.KERNEL_MATERN_NU else None,
                                sigma2=float(np.ravel(s["sigma2"])[0]))  # fmt: skip


def restate(st, dr, Xs, conditioned=True):
    """The restatement with its tolerances: paths, coefficients, the allowance per value / coefficient, and the host-side conditions."""
    finite = np.all(np.isfinite(Xs), axis=1)
    Xf = np.where(finite[:, None], Xs, 0.0)
    R = thompson.correlation(st, st.X, st.X)
    cond = np.linalg.cond(R)
    phase = np.max(np.abs(Xf) @ np.abs(dr.omega).T + np.abs(dr.phase))
    assert cond <= 1e8, cond
    assert phase <= 1e6, phase
    ptol = max(1e-6, 100 * cond * EPS)
    paths, (gt, bt) = thompson.paths_numpy(st, dr, Xs, conditioned)
    L = len(dr.phase)
    S = np.sqrt(2 * st.sigma2 / L) * np.abs(dr.weights).sum(axis=0)  # (q,)
    if not conditioned:
        return dict(paths=paths, tol=ptol * (np.abs(paths) + S[:, None] + abs(st.beta)), ptol=ptol)
    r = thompson.correlation(st, Xf, st.X)
    mu = st.beta + r @ np.linalg.solve(R, st.y - st.beta)
    A = S[:, None] + (np.abs(r) @ np.abs(gt)).T + np.abs(mu)[None, :] + np.abs(bt)[:, None]
    Rinv = np.linalg.inv(R)
    w = Rinv.sum(axis=1)
    A_g = np.abs(Rinv).sum(axis=1)[:, None] * (S + np.abs(bt))[None, :]
    A_b = np.abs(w).sum() * S / abs(w.sum())
    # the conditioning term is no bystander: a wrong one would move some value by 1e-2 A or more, 1e4 above the tolerance
    assert np.max((np.abs(r) @ np.abs(gt)).T / A) >= 1e-2
    tol = ptol * (np.abs(paths) + A)
    tol[:, ~finite] = np.inf
    return dict(paths=paths, gt=gt, bt=bt, tol=tol, tol_g=ptol * (np.abs(gt) + A_g), tol_b=ptol * (np.abs(bt) + A_b), ptol=ptol)


_excess = {}


@pytest.mark.parametrize("cfg", range(40))
def test_values_and_coefficients_against_the_restatement(eng, cfg):
    M, d, N, L, q, kernel, est = CONFIGS[cfg]
    X, y, theta, Xs = problem(M, d, N, kernel)
    st = commit(eng, X, y, theta, kernel, est)
    dr = thompson.draw(st, q, L, seed=cfg)
    ref = restate(st, dr, Xs)
    eng.upload_candidates(Xs)
    out = eng.sweep_thompson(dr, minimize=bool(cfg % 2), k=1, return_values=True)
    e_p = float(np.max(np.abs(out["paths"] - ref["paths"]) / ref["tol"]))
    e_g = float(np.max(np.abs(out["coef"][0] - ref["gt"]) / ref["tol_g"]))
    e_b = float(np.max(np.abs(out["coef"][1] - ref["bt"]) / ref["tol_b"]))
    _excess[cfg] = (e_p, e_g, e_b)
    print("cfg %2d M %4d d %2d N %3d L %4d q %2d kernel %d est %d ptol %.1e: excess paths %.3g gt %.3g bt %.3g (largest so far %.3g)"
          % (cfg, M, d, N, L, q, kernel, est, ref["ptol"], e_p, e_g, e_b, max(max(v) for v in _excess.values())))  # fmt: skip
    assert e_p <= 1.0 and e_g <= 1.0 and e_b <= 1.0, (e_p, e_g, e_b)
    # the winner is the stored values' own np.argmax, and best_x its row
    crit = -out["paths"] if cfg % 2 else out["paths"]
    np.testing.assert_array_equal(out["best_idx"][:, 0], np.argmax(crit, axis=1))
    np.testing.assert_array_equal(out["best_val"][:, 0], crit.max(axis=1))
    np.testing.assert_array_equal(out["best_x"][:, 0], Xs[out["best_idx"][:, 0]])


@pytest.mark.parametrize("N,kernel,est,minimize,seed", [(67, _lib.KERNEL_MATERN52, True, True, 3), (300, _lib.KERNEL_SE, False, False, 5),
                                                        (600, _lib.KERNEL_MATERN32, True, False, 3)])  # fmt: skip
def test_winners_equal_the_restatements_ranking(eng, N, kernel, est, minimize, seed):
    """best_idx / best_val for k = 1 and k = 16 are the restatement's ranking exactly; M = 10 < 16 leaves (-inf, -1) slots.  Two
    NaN candidate rows win at their first position, whichever the direction.  No tie carve-out: the restatement's gap between
    consecutive ranks used (the one behind the last rank included) exceeds the sum of the two values' tolerances, asserted here."""
    d, M, q = 3, 1000, 4
    X, y, theta, Xs = problem(M, d, N, kernel, seed=1)
    Xs[[7, 3]] = np.nan
    st = commit(eng, X, y, theta, kernel, est)
    dr = thompson.draw(st, q, 48, seed=seed)  # (a draw whose ranks are no near-ties: the assertion below)
    for Mc in (M, 10):
        ref = restate(st, dr, Xs[:Mc])
        crit = -ref["paths"] if minimize else ref["paths"]
        val, idx = ranking(crit, 17)
        assert np.all(idx[:, :2] == [3, 7])
        for j in range(q):
            for r in range(2, min(16, Mc - 1)):
                a, b = idx[j, r], idx[j, r + 1]
                assert crit[j, a] - crit[j, b] > ref["tol"][j, a] + ref["tol"][j, b], (j, r)
        eng.upload_candidates(Xs[:Mc])
        for k in (1, 16):
            out = eng.sweep_thompson(dr, minimize=minimize, k=k, return_values=True)
            np.testing.assert_array_equal(out["best_idx"], idx[:, :k])
            dev = -out["paths"] if minimize else out["paths"]
            for j in range(q):
                n = min(k, Mc)
                np.testing.assert_array_equal(out["best_val"][j, :n], dev[j, idx[j, :n]])
                assert np.all(out["best_val"][j, n:] == -np.inf) and np.all(np.isnan(out["best_x"][j, n:]))
                np.testing.assert_array_equal(out["best_x"][j, :n], Xs[idx[j, :n]])
            for j in range(q):
                for r in range(2, min(k, Mc)):
                    assert abs(out["best_val"][j, r] - val[j, r]) <= ref["tol"][j, idx[j, r]], (j, r)
            assert np.all(np.isnan(out["best_val"][:, : min(k, 2)]))


def test_bit_identity(eng):
    """N = 300 (320 padded rows): BOGP_CHUNK_MB=1 splits M = 1000 into chunks of 384, 384 and 232 rows."""
    M, d, N, kernel = 1000, 5, 300, _lib.KERNEL_MATERN52
    X, y, theta, Xs = problem(M, d, N, kernel)
    st = commit(eng, X, y, theta, kernel, True)
    eng.upload_candidates(Xs)
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 2.0)]
    before = eng.sweep(acq, float(y.min()), True, return_values=True)
    dr = thompson.draw(st, 16, 48, seed=5)
    whole = eng.sweep_thompson(dr, k=16, return_values=True)
    assert eng.thompson_last()["n_chunks"] == 1
    parts = _with_chunk_mb(1, lambda: eng.sweep_thompson(dr, k=16, return_values=True))
    assert eng.thompson_last()["n_chunks"] >= 3
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(whole[key], parts[key], err_msg=key)
    for a, b in zip(whole["coef"], parts["coef"]):
        np.testing.assert_array_equal(a, b)
    # rank 0 from the kernel's own records (k = 1) is rank 0 of the k passes over the stored values, chunked or not
    for one in (eng.sweep_thompson(dr, k=1), _with_chunk_mb(1, lambda: eng.sweep_thompson(dr, k=1))):
        np.testing.assert_array_equal(one["best_idx"][:, 0], whole["best_idx"][:, 0])
        np.testing.assert_array_equal(one["best_val"][:, 0], whole["best_val"][:, 0])
    # a path does not depend on how many paths share the call
    three = eng.sweep_thompson(dr._replace(weights=np.ascontiguousarray(dr.weights[:, :3]), eps=np.ascontiguousarray(dr.eps[:, :3])), return_values=True)
    np.testing.assert_array_equal(three["paths"], whole["paths"][:3])
    np.testing.assert_array_equal(three["coef"][0], whole["coef"][0][:, :3])
    # the prior paths: beta + z, bit-identical across chunkings too, and zero coefficients
    prior = eng.sweep_thompson(dr, conditioned=False, k=16, return_values=True)
    prior_parts = _with_chunk_mb(1, lambda: eng.sweep_thompson(dr, conditioned=False, k=16, return_values=True))
    np.testing.assert_array_equal(prior["paths"], prior_parts["paths"])
    ref = restate(st, dr, Xs, conditioned=False)
    assert np.all(np.abs(prior["paths"] - ref["paths"]) <= ref["tol"])
    assert not prior["coef"][0].any() and not prior["coef"][1].any()
    np.testing.assert_array_equal(prior["best_idx"], ranking(-prior["paths"], 16)[1])
    # the handle is unaffected: a plain sweep gives the bits it gave before
    after = eng.sweep(acq, float(y.min()), True, return_values=True)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_candidate_sources(eng):
    M, d, N, kernel = 1000, 4, 67, _lib.KERNEL_SE
    X, y, theta, _ = problem(M, d, N, kernel)
    st = commit(eng, X, y, theta, kernel, True)
    dr = thompson.draw(st, 5, 48, seed=2)
    eng.generate_candidates(np.full(d, -2.2), np.full(d, 2.2), M, seed=17)
    gen = eng.sweep_thompson(dr, k=4, return_values=True)
    Xs = eng.read_candidates(np.arange(M))
    eng.upload_candidates(Xs)
    up = eng.sweep_thompson(dr, k=4, return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy = eng.sweep_thompson(dr, k=4, return_values=True)
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(gen[key], up[key], err_msg=key)
        np.testing.assert_array_equal(lazy[key], up[key], err_msg=key)
    np.testing.assert_array_equal(up["best_x"], Xs[up["best_idx"]])


def _call(eng, q=2, L=16, k=1, omega=True, phase=True, weights=True, eps=None, best=True, idx=True, bad=None):
    lib = _lib.load()
    d, N = max(eng.d, 1), max(eng.N, 1)
    om, ph, w = np.ones((max(L, 1), d)), np.zeros(max(L, 1)), np.ones((max(L, 1), max(q, 1)))
    ep = None if eps is None else np.zeros((N, max(q, 1)))
    if bad is not None:
        dict(omega=om, phase=ph, weights=w, eps=ep)[bad].flat[-1] = np.inf
    n = max(q, 1) * max(k, 1)
    bv, bi = np.empty(n), np.empty(n, dtype=np.int64)
    rc = lib.bogp_sweep_thompson(eng._h, q, L, _lib._ptr(om) if omega else None, _lib._ptr(ph) if phase else None, _lib._ptr(w) if weights else None,
                                 _lib._ptr(ep), 1, 1, k, _lib._ptr(bv) if best else None, bi.ctypes.data_as(C.POINTER(C.c_int64)) if idx else None,
                                 None, None, None)  # fmt: skip
    return rc, lib.bogp_last_error(eng._h).decode()


def test_error_returns():
    """Every error return of bogp_sweep_thompson but one: a communicator of more than one rank cannot be built on one device (its
    refusal is a comparison of the handle's world size; the Python layer's own refusal is exercised on the host)."""
    lib = _lib.load()
    assert lib.bogp_sweep_thompson(None, 1, 16, None, None, None, None, 1, 1, 1, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.bogp_thompson_last(None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, y, theta, Xs = problem(100, 3, 67, _lib.KERNEL_SE)
        e.set_train(X, y)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no committed model" in msg
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no candidates" in msg
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK and _call(e, eps=True)[0] == _lib.OK
        for kw in (dict(q=0), dict(q=17), dict(L=0), dict(L=24), dict(L=_lib.MAX_FEATURES + 16), dict(k=0), dict(k=_lib.MAX_TOPK + 1),
                   dict(omega=False), dict(phase=False), dict(weights=False), dict(best=False), dict(idx=False)):  # fmt: skip
            assert _call(e, **kw)[0] == _lib.ERR_INVALID, kw
        for bad in ("omega", "phase", "weights", "eps"):
            rc, msg = _call(e, eps=True, bad=bad)
            assert rc == _lib.ERR_INVALID and bad in msg and "non-finite" in msg
        st = thompson.dense_state(X, y, theta, _lib.KERNEL_SE)
        with pytest.raises(_lib.BogpError) as ei:
            e.sweep_thompson(thompson.draw(st, 2, 16, seed=0), k=33)
        assert ei.value.code == _lib.ERR_INVALID
        # a lift on the handle
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "lift" in msg
        with pytest.raises(NotImplementedError, match="lift"):
            e.sweep_thompson(thompson.draw(st, 2, 16, seed=0))
        e.clear_lift()
        assert _call(e)[0] == _lib.OK
        # the two modes with a rescaled R
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noisy mode" in msg
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[theta, 0.9], 0.0, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noise-estimating mode" in msg
        # the two kernels without a spectral draw
        e.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISELESS, np.full(3, 2.0), 0.0, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "cubic" in msg
        e.commit(_lib.KERNEL_GENEXP, _lib.MODE_NOISELESS, np.r_[theta, 1.5], 0.0, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "generalized-exponential" in msg
        # a polynomial trend basis
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "constant trend" in msg
        # several targets
        e.set_train(X, np.column_stack([y, 2 * y + 1]))
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
        e.upload_candidates(Xs)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "one target" in msg
    finally:
        e.close()
    f = _lib.Engine(0)  # a forest takes a handle of its own
    try:
        f.forest_set(3, [0, 1, 2], [-2, -2], [-2.0, -2.0], [-1, -1], [-1, -1], [0.0, 1.0])
        f.upload_candidates(Xs)
        rc, msg = _call(f)
        assert rc == _lib.ERR_UNSUPPORTED and "forest" in msg
    finally:
        f.close()


def test_refusals_keep_their_precedence():
    """Two faults in one call: the one that comes first in the entry's order of checks -- forest, not committed, no candidates, q, L,
    k, null pointers, non-finite omega / phase / weights / eps, mode, trend columns, targets, kernel, lift, ranks -- is reported."""
    e = _lib.Engine(0)
    try:
        X, y, theta, Xs = problem(100, 3, 67, _lib.KERNEL_SE)
        e.set_train(X, y)
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK
        for kw, first in ((dict(q=0, L=24), "q = 0 outside"), (dict(L=24, k=0), "L = 24"), (dict(k=0, omega=False), "k = 0 outside")):
            rc, msg = _call(e, **kw)
            assert rc == _lib.ERR_INVALID and first in msg, (kw, msg)
        # q = 17 and a lift on the handle: q
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _call(e, q=17)
        assert rc == _lib.ERR_INVALID and "q = 17 outside" in msg, msg
        e.clear_lift()
        # a non-finite omega and a noisy-mode commit: the non-finite entry
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, True, 0.0)
        rc, msg = _call(e, bad="omega")
        assert rc == _lib.ERR_INVALID and "omega has a non-finite entry" in msg, msg
        # the noisy mode and a linear trend: the mode
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, True, 0.0, trend=_lib.TREND_LINEAR)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noisy mode" in msg, msg
        # the cubic kernel and a lift: the kernel
        e.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISELESS, np.full(3, 2.0), 0.0, True, 0.0)
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "cubic" in msg, msg
    finally:
        e.close()
