"""Thompson batches for constrained multi-objective runs on the device (`bogp_sweep_thompson_ehvi_constrained`,
kernels_thompson_ehvi_constrained.hip) against the dense NumPy restatement `bogp.thompson.paths_multi_numpy` /
`hvi_constrained_select_numpy` on the SAME draw.  Cases: tests/thompson_ehvi_constrained_cases.py; what they are built for is asserted
on the restatement alone by tests/test_thompson_ehvi_constrained_host.py.

  paths and g against the restatement over 16 shapes: |dev - ref| <= ptol (|ref| + A), ptol = max(1e-6, 100 cond(R) eps) (ledger
    T29's form and allowance; the largest ratio measured is ledger T33);
  selection, EXACT: scores, rankings and best_x equal `hvi_constrained_select_numpy` applied to the device's own paths, byte for byte,
    at feasible shares of 0, 0.1, 0.5 and 1 (F = 320 pairs a workgroup), on the "far" front and on the one-cell front;
  bit identity: the constrained kernel's path values for the same columns, any chunking, with and without paths_out, a member alone;
  `bogp_sweep_thompson_ehvi` and `bogp_sweep_ehvi_constrained` before and after a call;  every error return through the real ABI;
  `bogp.constrained_ehvi_thompson_batch` on a real model."""
import ctypes as C

import numpy as np
import pytest

import thompson_constrained_cases as TC
import thompson_ehvi_constrained_cases as CC
from bogp import _lib, thompson
from support.chunk_mb import with_chunk_mb as _with_chunk_mb
from test_gpu_thompson_constrained import _assert_selection, commit

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _against_the_restatement(out, ref, tag):
    e_p = float(np.max(np.abs(out["paths"] - ref.paths) / ref.tol))
    e_g = float(np.max(np.abs(out["coef"] - ref.gt) / ref.tol_g))
    print("%s ptol %.1e: ratio to the allowance paths %.3g g %.3g" % (tag, ref.ptol, e_p, e_g))
    assert e_p <= 1.0 and e_g <= 1.0, (e_p, e_g)


@pytest.mark.parametrize("cfg", range(len(CC.SHAPES)))
def test_paths_coefficients_and_winners_over_the_shapes(eng, cfg):
    M, d, N, L, C_, m_obj, n_con, q, kernel = CC.SHAPES[cfg]
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, m_obj + n_con)
    st = commit(eng, X, Y, theta, kernel)
    dr = thompson.draw_multi(st, q, L, seed=cfg)
    ref = TC.restate(st, dr, Xs)
    assert ref.cond <= 1e8 and ref.share >= 1e-2, (ref.cond, ref.share)
    lower, upper = CC.cells_of(C_, Y[:, :m_obj])
    lo, hi = np.full(n_con, -INF), np.median(Y[:, m_obj:], axis=0)
    eng.upload_candidates(Xs)
    for k in (1, 3):
        out = eng.sweep_thompson_ehvi_constrained(dr, q, lower, upper, lo, hi, k=k, return_values=True)
        _against_the_restatement(out, ref, "cfg %2d %s k %d" % (cfg, CC.SHAPES[cfg], k))
        _assert_selection(out, thompson.hvi_constrained_select_numpy(out["paths"], m_obj, lower, upper, lo, hi, st.sigma2, k), Xs, k)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_selection_is_exact_on_the_devices_own_paths(eng, name):
    c = CC.case(name)
    st = commit(eng, c.X, c.Y, c.theta, c.kernel)
    lo, hi = CC.bounds_for_share(TC.restate(st, c.dr, c.Xs).paths, c.m_obj, c.share)
    for Mc in (CC.CASE_M, 10):  # M = 10 < 16 leaves (-inf, -1) slots
        Xs = c.Xs[:Mc]
        eng.upload_candidates(Xs)
        for k in (1, 16):
            out = eng.sweep_thompson_ehvi_constrained(c.dr, c.q, c.lower, c.upper, lo, hi, k=k, return_values=True)
            sel = thompson.hvi_constrained_select_numpy(out["paths"], c.m_obj, c.lower, c.upper, lo, hi, st.sigma2, k)
            _assert_selection(out, sel, Xs, k)
            if c.share == 0.0:
                assert not sel["feas"].any() and np.all(out["best_val"][:, :2] == -INF) and np.all(out["best_val"][:, 2, : min(k, Mc)] < 0)
            if c.share == 1.0:
                assert sel["feas"].all() and np.all(sel["V"] == 0)
            if c.front == "far":
                assert np.all(sel["A"] == -INF) and np.all(out["best_val"][:, 0] == -INF) and np.any(sel["B"] > -INF)
                assert np.all(out["best_val"][:, 1, 0] < 0) and np.all(out["best_val"][:, 1, 0] > -INF)
        if Mc == CC.CASE_M:
            share = float(np.mean(sel["feas"]))
            print("%s: feasible share %.3f, improving share %.3f" % (name, share, float(np.mean(sel["A"] > -INF))))
            assert CC.BAND[c.share][0] <= share <= CC.BAND[c.share][1]


def test_bit_identity(eng):
    """N = 300 (320 padded rows): BOGP_CHUNK_MB=1 splits M = 1000 into chunks of 384, 384 and 232 rows."""
    M, d, N, kernel, m_obj, n_con, q = 1000, 5, 300, _lib.KERNEL_MATERN52, 2, 1, 5
    m = m_obj + n_con
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, m)
    st = commit(eng, X, Y, theta, kernel)
    lower, upper = CC.cells_of(33, Y[:, :m_obj])
    lo, hi = np.full(n_con, -INF), np.median(Y[:, m_obj:], axis=0)
    eng.upload_candidates(Xs)
    dr = thompson.draw_multi(st, q, 48, seed=5)
    run = lambda k, rv=True: eng.sweep_thompson_ehvi_constrained(dr, q, lower, upper, lo, hi, k=k, return_values=rv)  # noqa: E731
    whole = run(16)
    assert eng.thompson_ehvi_constrained_last()["n_chunks"] == 1
    parts = _with_chunk_mb(1, lambda: run(16))
    assert eng.thompson_ehvi_constrained_last()["n_chunks"] >= 3
    for key in ("best_val", "best_idx", "best_x", "paths", "coef"):
        np.testing.assert_array_equal(whole[key], parts[key], err_msg=key)
    bare = run(16, False)  # with and without paths_out
    for key in ("best_val", "best_idx", "best_x", "coef"):
        np.testing.assert_array_equal(whole[key], bare[key], err_msg=key)
    for one in (run(1), run(1, False), _with_chunk_mb(1, lambda: run(1))):  # the kernel's own records against the ranked scores
        np.testing.assert_array_equal(one["best_idx"][:, :, 0], whole["best_idx"][:, :, 0])
        np.testing.assert_array_equal(one["best_val"][:, :, 0], whole["best_val"][:, :, 0])
    # the constrained kernel's bits for the same columns and total m: targets 1 .. m - 1 as its constraints, infinite bounds
    con = eng.sweep_thompson_constrained(dr, q, np.full(m - 1, -INF), np.full(m - 1, INF), k=1, return_values=True)
    np.testing.assert_array_equal(con["paths"], whole["paths"])
    np.testing.assert_array_equal(con["coef"], whole["coef"])
    # a member alone (q = 1: one round, 16 lanes, other columns, another place in the list) against the call of 5 (two rounds)
    cols = slice(2 * m, 3 * m)
    alone = eng.sweep_thompson_ehvi_constrained(dr._replace(weights=np.ascontiguousarray(dr.weights[:, cols]), eps=np.ascontiguousarray(dr.eps[:, cols])),
                                                1, lower, upper, lo, hi, k=16, return_values=True)  # fmt: skip
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(alone[key][0], whole[key][2], err_msg=key)
    np.testing.assert_array_equal(alone["coef"], whole["coef"][:, cols])


def test_the_neighbouring_sweeps_are_unchanged_by_a_call(eng):
    """`bogp_sweep_thompson_ehvi` and `bogp_sweep_ehvi_constrained` immediately before and after a call on the same handle: the same bytes."""
    M, d, N, kernel = 1000, 3, 67, _lib.KERNEL_MATERN52
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, 3)
    st = commit(eng, X, Y, theta, kernel)
    low3, up3 = CC.cells_of(33, Y)
    low2, up2 = CC.cells_of(33, Y[:, :2])
    lo, hi = np.array([-INF]), np.median(Y[:, 2:], axis=0)
    dr = thompson.draw_multi(st, 5, 48, seed=4)

    def neighbours():
        eng.upload_candidates(Xs)
        out = eng.sweep_thompson_ehvi(dr, 5, low3, up3, k=16, return_values=True)
        return [out[key] for key in ("best_val", "best_idx", "best_x", "paths", "coef")] + list(eng.sweep_ehvi_constrained(low2, up2, lo, hi, k=16, return_values=True))

    before = neighbours()
    eng.sweep_thompson_ehvi_constrained(dr, 5, low2[:7], up2[:7], lo, hi, k=16, return_values=True)
    for a, b in zip(before, neighbours()):
        np.testing.assert_array_equal(a, b)


def _call(eng, q=2, L=16, k=1, m_obj=2, n_con=1, C_=2, lower=None, upper=None, lo=None, hi=None, eps=None, bad=None, null=None):
    lib = _lib.load()
    qa, La, m = max(q, 1), max(L, 1), max(m_obj + n_con, 1)
    arr = dict(omega=np.ones((La, max(eng.d, 1))), phase=np.zeros(La), weights=np.ones((La, qa * m)), eps=np.zeros((max(eng.N, 1), qa * m)) if eps else None,
               lower=np.zeros((max(C_, 1), max(m_obj, 1))) if lower is None else np.array(lower, dtype=float),
               upper=np.full((max(C_, 1), max(m_obj, 1)), INF) if upper is None else np.array(upper, dtype=float),
               lo=np.full(max(n_con, 1), -INF) if lo is None else np.array(lo, dtype=float),
               hi=np.zeros(max(n_con, 1)) if hi is None else np.array(hi, dtype=float), best_val=np.empty(3 * qa * max(k, 1)))  # fmt: skip
    bi = np.empty(3 * qa * max(k, 1), dtype=np.int64)
    if bad is not None:
        arr[bad].flat[-1] = np.inf
    p = {n: (None if n == null or a is None else _lib._ptr(a)) for n, a in arr.items()}
    rc = lib.bogp_sweep_thompson_ehvi_constrained(eng._h, m_obj, q, L, p["omega"], p["phase"], p["weights"], p["eps"], C_, p["lower"], p["upper"], n_con,
                                                  p["lo"], p["hi"], k, p["best_val"], None if null == "best_idx" else bi.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  None, None, None)  # fmt: skip
    return rc, lib.bogp_last_error(eng._h).decode()


def test_error_returns():
    """Every error return of bogp_sweep_thompson_ehvi_constrained but one (a communicator of more than one rank cannot be built on one
    device), each by its message; where a call carries two faults, the one the entry's order of checks has first."""
    lib, INV, UNS = _lib.load(), _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert lib.bogp_sweep_thompson_ehvi_constrained(None, 2, 1, 16, None, None, None, None, 1, None, None, 1, None, None, 1, None, None, None, None, None) == INV
    assert lib.bogp_thompson_ehvi_constrained_last(None, None, None, None, None) == INV
    X, Y, theta, Xs = TC.problem(100, 3, 67, _lib.KERNEL_SE, 3)
    NOISELESS, upside = _lib.MODE_NOISELESS, dict(lower=[[0, 1.0], [0, 0]], upper=[[1, 0.0], [1, 1]])
    e = _lib.Engine(0)
    try:
        e.set_train(X, Y)
        assert _call(e)[0] == INV and "no committed model" in _call(e)[1]
        e.commit(_lib.KERNEL_SE, NOISELESS, theta, 0.0, False, 0.3)
        assert _call(e)[0] == INV and "no candidates" in _call(e)[1]
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK and _call(e, eps=True)[0] == _lib.OK and _call(e, q=5)[0] == _lib.OK
        for kw, word in ((dict(m_obj=1, n_con=2), "m_obj = 1"), (dict(m_obj=3, n_con=0), "n_con = 0"), (dict(m_obj=3, q=0), "m_obj = 3 and n_con = 1"),
                         (dict(q=0), "q = 0"), (dict(q=6, L=24), "q = 6 members"), (dict(L=0), "L = 0"), (dict(L=24), "L = 24"),
                         (dict(L=_lib.MAX_FEATURES + 16), "L ="), (dict(k=0, C_=0), "k = 0 outside"), (dict(k=_lib.MAX_TOPK + 1), "k ="),
                         (dict(C_=0, null="lower"), "C = 0 cells"), (dict(C_=_lib.MAX_EHVI_CELLS + 1), "cells outside"), (dict(lower=[[0, INF], [0, 0]]), "not finite"),
                         (dict(upper=[[1, np.nan], [1, 1]], lo=[np.nan]), "is NaN"), (upside, "below its lower bound"), (dict(lo=[np.nan], bad="omega"), "a bound of constraint 0 is NaN"),
                         (dict(lo=[1.0], hi=[0.0], bad="omega"), "upper bound of constraint 0"), (dict(eps=True, bad="eps"), "eps has a non-finite"),
                         (dict(bad="omega"), "omega has a non-finite"), (dict(bad="phase"), "phase has a non-finite"), (dict(bad="weights"), "weights has a non-finite"),
                         ) + tuple((dict(null=n), "must be non-null") for n in ("omega", "phase", "weights", "lower", "upper", "lo", "hi", "best_val", "best_idx")):  # fmt: skip
            rc, msg = _call(e, **kw)
            assert rc == INV and word in msg, (kw, msg)
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        assert _call(e, q=0)[0] == UNS and "lift" in _call(e, q=0)[1]  # a lift and q = 0: the lift
        e.clear_lift()
        for kernel, mode, par, word in ((_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], "noisy mode"),
                                        (_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[theta, 0.9], "noise-estimating mode"),
                                        (_lib.KERNEL_CUBIC, NOISELESS, np.full(3, 2.0), "cubic"),
                                        (_lib.KERNEL_GENEXP, NOISELESS, np.r_[theta, 1.5], "generalized-exponential")):  # fmt: skip
            e.commit(kernel, mode, par, 1e-6 if mode == _lib.MODE_NOISY else 0.0, False, 0.3)
            assert _call(e)[0] == UNS and word in _call(e)[1], word
        e.set_train(X, Y[:, 0])  # one target: a polynomial trend is refused by name, the constant one is sent to bogp_sweep_thompson
        for trend, rc, word in ((_lib.TREND_LINEAR, UNS, "constant trend"), (_lib.TREND_CONSTANT, INV, "bogp_sweep_thompson serves it")):
            e.commit(_lib.KERNEL_SE, NOISELESS, theta, 0.0, True, 0.0, trend=trend)
            e.upload_candidates(Xs)
            assert _call(e)[0] == rc and word in _call(e)[1], word
    finally:
        e.close()
    f = _lib.Engine(0)  # a forest takes a handle of its own
    try:
        f.forest_set(3, [0, 1, 2], [-2, -2], [-2.0, -2.0], [-1, -1], [-1, -1], [0.0, 1.0])
        f.upload_candidates(Xs)
        assert _call(f)[0] == UNS and "forest" in _call(f)[1]
    finally:
        f.close()


def test_the_python_batch_on_the_device():
    """`bogp.constrained_ehvi_thompson_batch` on a real model: q = 7 (calls of 5 and 2 members) distinct rows, none a `history` row;
    the first member's proposal is the best row of the first non-empty tier of the device's own scores outside `history`, fopt its value."""
    import bogp
    from bogp import optim

    X, Y, _, Xs = TC.problem(300, 3, 40, _lib.KERNEL_MATERN52, 3, seed=9)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    model.set_state(np.r_[0.6, 0.6, 0.6], X, Y)
    lo, hi = np.array([-INF]), np.median(Y[:, 2:], axis=0)
    crit = bogp.ConstrainedEHVI(model=model, ref_point=np.quantile(Y[:, :2], 0.3, axis=0), lo=lo, hi=hi)
    lower, upper = crit.cell_lower_bounds, crit.cell_upper_bounds
    assert len(lower) >= 1
    kw = dict(q=7, n_features=64, seed=4, Xs=Xs)
    first, _ = bogp.constrained_ehvi_thompson_batch(crit, optim.Box([(-2.2, 2.2)] * 3, random_seed=3), 300, **kw)
    xs, fs = bogp.constrained_ehvi_thompson_batch(crit, optim.Box([(-2.2, 2.2)] * 3, random_seed=3), 300, history=np.array(first[:2]), **kw)
    row_of = lambda x: int(np.flatnonzero(np.all(Xs == np.asarray(x), axis=1))[0])  # noqa: E731
    rows, gone = [row_of(x) for x in xs], [row_of(x) for x in first[:2]]
    assert len(set(rows)) == 7 and not set(rows) & set(gone)
    dr = thompson.draw_multi(model, 5, 64, np.random.SeedSequence(4).spawn(2)[0])
    out = model.engine.sweep_thompson_ehvi_constrained(dr, 5, lower, upper, lo, hi, return_values=True)
    sel = thompson.hvi_constrained_select_numpy(out["paths"], 2, lower, upper, lo, hi, thompson.state_of_multi(model).sigma2, 1)
    score = next(s[0] for s in (sel["A"], sel["B"], sel["V"]) if np.any(s[0] > -INF))
    score[gone] = -INF
    assert rows[0] == int(np.argmax(score)) and fs[0] == score[rows[0]]
    model.engine.close()
