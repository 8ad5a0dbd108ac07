"""Thompson batches under modelled constraints on the device (`bogp_sweep_thompson_constrained`, kernels_thompson_constrained.hip)
against the dense NumPy restatement `bogp.thompson.paths_multi_numpy` / `select_numpy` on the SAME draw.  The cases and their
allowances live in tests/thompson_constrained_cases.py; the conditions that keep this file from hiding a failure (conditioning, no
near-ties, no row at a bound that could enter a ranking) are asserted on the restatement alone by
tests/test_thompson_constrained_host.py and again here on the state the engine committed.

  paths and g against the restatement over 28 shapes (every tile edge of the kernel, 16 / 15 / fewer columns, the six kernels, both
    directions): |dev - ref| <= ptol (|ref| + A), ptol = max(1e-6, 100 cond(R) eps) (the project's north star, ledger T16's form).
    The largest excess measured: 1.8e-8 of the allowance for the paths, 2.4e-8 for g (ledger T29);
  selection, EXACT and without a carve-out: scores, rankings and best_x equal `select_numpy` applied to the device's own paths;
  end to end: the winners are the restatement's ranking where the host twin's conditions decide it;
  bit identity across chunkings, across the members of a call, with and without paths_out, across candidate sources;
  `bogp_sweep_thompson` before and after a constrained call;  every error return through the real ABI;
  `bogp.constrained_thompson_batch` on a real model against the device's own scores."""
import ctypes as C

import numpy as np
import pytest

import thompson_constrained_cases as TC
from bogp import _lib, thompson
from support.chunk_mb import with_chunk_mb as _with_chunk_mb

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def commit(eng, X, Y, theta, kernel):
    """Commit the multi-target model (noiseless, fixed constant trend) and return the dense state with the engine's own sigma2."""
    eng.set_train(X, Y)
    eng.commit(kernel, _lib.MODE_NOISELESS, np.r_[theta, TC.NU] if kernel == _lib.KERNEL_MATERN_NU else theta, 0.0, False, TC.BETA)
    s = eng.get_state(with_C=False)
    assert float(np.ravel(s["beta"])[0]) == TC.BETA
    return TC.state(X, Y, theta, kernel, sigma2=np.ravel(s["sigma2"]))


_excess = {}


@pytest.mark.parametrize("cfg", range(len(TC.SHAPES)))
def test_paths_and_coefficients_against_the_restatement(eng, cfg):
    M, d, N, L, m, q, kernel, minimize = TC.SHAPES[cfg]
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, m)
    st = commit(eng, X, Y, theta, kernel)
    dr = thompson.draw_multi(st, q, L, seed=cfg)
    ref = TC.restate(st, dr, Xs)
    assert ref.cond <= 1e8 and ref.phase <= 1e6, (ref.cond, ref.phase)
    assert ref.share >= 1e-2  # the conditioning term is no bystander: a wrong one would move some value 1e4 allowances
    lo, hi = TC.bounds("median", Y)
    eng.upload_candidates(Xs)
    out = eng.sweep_thompson_constrained(dr, q, lo, hi, minimize=minimize, k=1, return_values=True)
    e_p = float(np.max(np.abs(out["paths"] - ref.paths) / ref.tol))
    e_g = float(np.max(np.abs(out["coef"] - ref.gt) / ref.tol_g))
    _excess[cfg] = (e_p, e_g)
    print("cfg %2d M %4d d %2d N %3d L %4d m %d q %d kernel %d min %d ptol %.1e: excess paths %.3g g %.3g (largest so far %.3g %.3g)"
          % (cfg, M, d, N, L, m, q, kernel, minimize, ref.ptol, e_p, e_g, max(v[0] for v in _excess.values()), max(v[1] for v in _excess.values())))  # fmt: skip
    assert e_p <= 1.0 and e_g <= 1.0, (e_p, e_g)
    # the winners are the selection of the device's own paths, and best_x their rows
    sel = thompson.select_numpy(out["paths"], lo, hi, st.sigma2, minimize, 1)
    np.testing.assert_array_equal(out["best_val"], sel["best_val"])
    np.testing.assert_array_equal(out["best_idx"], sel["best_idx"])
    np.testing.assert_array_equal(out["best_x"], Xs[out["best_idx"]])


def _assert_selection(out, sel, Xs, k):
    np.testing.assert_array_equal(out["best_val"].view(np.int64), sel["best_val"].view(np.int64))  # byte for byte: +0.0 is not -0.0
    np.testing.assert_array_equal(out["best_idx"], sel["best_idx"])
    filled = out["best_idx"] >= 0
    np.testing.assert_array_equal(out["best_x"][filled], Xs[out["best_idx"][filled]])
    assert np.all(np.isnan(out["best_x"][~filled])) and np.all(out["best_val"][~filled] == -INF)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_selection_is_exact_on_the_devices_own_paths_and_the_winners_are_the_restatements(eng, name):
    c = TC.case(name)
    st = commit(eng, c.X, c.Y, c.theta, c.kernel)
    c.st = st
    ref = TC.restate(st, c.dr, c.Xs)
    assert ref.cond <= 1e8 and ref.phase <= 1e6
    assert TC.conditions(c, ref) == []
    want = thompson.select_numpy(ref.paths, c.lo, c.hi, st.sigma2, c.minimize, 16)
    kind = TC.CASES[name][5]
    for Mc in (TC.CASE_M, 10):  # M = 10 < 16 leaves (-inf, -1) slots
        Xs = c.Xs[:Mc]
        eng.upload_candidates(Xs)
        for k in (1, 16):
            out = eng.sweep_thompson_constrained(c.dr, c.q, c.lo, c.hi, minimize=c.minimize, k=k, return_values=True)
            sel = thompson.select_numpy(out["paths"], c.lo, c.hi, st.sigma2, c.minimize, k)
            _assert_selection(out, sel, Xs, k)
            if kind == "none":
                assert not sel["feas"].any() and np.all(sel["A"] == -INF) and np.all(sel["B"] < 0)
                assert np.all(out["best_val"][:, 0] == -INF)
            if kind == "open":
                np.testing.assert_array_equal(sel["A"], -out["paths"][:, 0] if c.minimize else out["paths"][:, 0])
                assert np.all(sel["B"].view(np.int64) == 0) and np.all(out["best_val"][:, 1, : min(k, Mc)].view(np.int64) == 0)
                np.testing.assert_array_equal(out["best_idx"][:, 1, : min(k, Mc)], np.tile(np.arange(min(k, Mc)), (c.q, 1)))
            if Mc == TC.CASE_M:  # end to end: the conditions above decide these rankings
                n_dec = np.minimum(np.sum(want["best_val"][:, 0] > -INF, axis=1), k)
                for j in range(c.q):
                    np.testing.assert_array_equal(out["best_idx"][j, 0, : n_dec[j]], want["best_idx"][j, 0, : n_dec[j]])
                    for r in range(n_dec[j]):
                        assert abs(out["best_val"][j, 0, r] - want["best_val"][j, 0, r]) <= ref.tol[j, 0, want["best_idx"][j, 0, r]]
                    assert np.all(out["best_val"][j, 0, n_dec[j] : k] == -INF)  # as many feasible rows as the restatement has
                if kind == "none":
                    np.testing.assert_array_equal(out["best_idx"][:, 1], want["best_idx"][:, 1, :k])


def test_a_nan_candidate_row_is_never_listed(eng):
    c = TC.case("m2-mixed")
    st = commit(eng, c.X, c.Y, c.theta, c.kernel)
    Xs = c.Xs.copy()
    Xs[[3, 7]] = np.nan
    eng.upload_candidates(Xs)
    out = eng.sweep_thompson_constrained(c.dr, c.q, c.lo, c.hi, minimize=c.minimize, k=16, return_values=True)
    sel = thompson.select_numpy(out["paths"], c.lo, c.hi, st.sigma2, c.minimize, 16)
    _assert_selection(out, sel, Xs, 16)
    assert np.all(np.isnan(out["paths"][:, :, [3, 7]])) and np.all(sel["A"][:, [3, 7]] == -INF) and np.all(sel["B"][:, [3, 7]] == -INF)
    for j in range(c.q):
        rows = [gi for gi, _, _ in thompson.merge_ranks(out["best_val"][j], out["best_idx"][j], 32)]
        assert rows and 3 not in rows and 7 not in rows


def test_bit_identity(eng):
    """N = 300 (320 padded rows): BOGP_CHUNK_MB=1 splits M = 1000 into chunks of 384, 384 and 232 rows."""
    M, d, N, kernel, m, q = 1000, 5, 300, _lib.KERNEL_MATERN52, 4, 4
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, m)
    st = commit(eng, X, Y, theta, kernel)
    lo, hi = TC.bounds("median", Y)
    eng.upload_candidates(Xs)
    dr = thompson.draw_multi(st, q, 48, seed=5)
    run = lambda k, rv=True: eng.sweep_thompson_constrained(dr, q, lo, hi, k=k, return_values=rv)  # noqa: E731
    whole = run(16)
    assert eng.thompson_constrained_last()["n_chunks"] == 1
    parts = _with_chunk_mb(1, lambda: run(16))
    assert eng.thompson_constrained_last()["n_chunks"] >= 3
    for key in ("best_val", "best_idx", "best_x", "paths", "coef"):
        np.testing.assert_array_equal(whole[key], parts[key], err_msg=key)
    # with and without paths_out
    bare = run(16, False)
    for key in ("best_val", "best_idx", "best_x", "coef"):
        np.testing.assert_array_equal(whole[key], bare[key], err_msg=key)
    # rank 0 from the kernel's own records (k = 1) is rank 0 of the k passes over the stored scores, chunked or not
    for one in (run(1), run(1, False), _with_chunk_mb(1, lambda: run(1))):
        np.testing.assert_array_equal(one["best_idx"][:, :, 0], whole["best_idx"][:, :, 0])
        np.testing.assert_array_equal(one["best_val"][:, :, 0], whole["best_val"][:, :, 0])
    # a member's bytes do not depend on the members beside it: member 2 alone (q = 1, other device columns) against the call of 4
    cols = slice(2 * m, 3 * m)
    alone = eng.sweep_thompson_constrained(dr._replace(weights=np.ascontiguousarray(dr.weights[:, cols]), eps=np.ascontiguousarray(dr.eps[:, cols])),
                                           1, lo, hi, k=16, return_values=True)  # fmt: skip
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(alone[key][0], whole[key][2], err_msg=key)
    np.testing.assert_array_equal(alone["coef"], whole["coef"][:, cols])


def test_candidate_sources(eng):
    M, d, N, kernel, m, q = 1000, 4, 67, _lib.KERNEL_SE, 3, 5
    X, Y, theta, _ = TC.problem(M, d, N, kernel, m)
    st = commit(eng, X, Y, theta, kernel)
    lo, hi = TC.bounds("median", Y)
    dr = thompson.draw_multi(st, q, 48, seed=2)
    eng.generate_candidates(np.full(d, -2.2), np.full(d, 2.2), M, seed=17)
    gen = eng.sweep_thompson_constrained(dr, q, lo, hi, k=4, return_values=True)
    Xs = eng.read_candidates(np.arange(M))
    eng.upload_candidates(Xs)
    up = eng.sweep_thompson_constrained(dr, q, lo, hi, k=4, return_values=True)
    eng.upload_candidates(Xs, lazy=True)
    lazy = eng.sweep_thompson_constrained(dr, q, lo, hi, k=4, return_values=True)
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(gen[key], up[key], err_msg=key)
        np.testing.assert_array_equal(lazy[key], up[key], err_msg=key)
    np.testing.assert_array_equal(up["best_x"], Xs[up["best_idx"]])


def test_the_single_target_paths_are_unchanged_by_a_constrained_call(eng):
    """`bogp_sweep_thompson` immediately before and after a constrained call on the same handle: the same bytes."""
    M, d, N, kernel = 1000, 3, 67, _lib.KERNEL_MATERN52
    X, Y, theta, Xs = TC.problem(M, d, N, kernel, 3)
    lo, hi = TC.bounds("median", Y)

    def single():
        eng.set_train(X, Y[:, 0])
        eng.commit(kernel, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        st1 = thompson.dense_state(X, Y[:, 0], theta, kernel)
        eng.upload_candidates(Xs)
        return eng.sweep_thompson(thompson.draw(st1, 16, 48, seed=3), k=16, return_values=True)

    before = single()
    st = commit(eng, X, Y, theta, kernel)
    eng.upload_candidates(Xs)
    eng.sweep_thompson_constrained(thompson.draw_multi(st, 5, 48, seed=4), 5, lo, hi, k=16, return_values=True)
    after = single()
    for key in ("best_val", "best_idx", "best_x", "paths"):
        np.testing.assert_array_equal(before[key], after[key], err_msg=key)
    for a, b in zip(before["coef"], after["coef"]):
        np.testing.assert_array_equal(a, b)


def _call(eng, q=2, L=16, k=1, m=2, n_con=None, lo=None, hi=None, eps=None, bad=None, null=None):
    lib = _lib.load()
    d, N = max(eng.d, 1), max(eng.N, 1)
    qa, La, ka = max(q, 1), max(L, 1), max(k, 1)
    arr = dict(omega=np.ones((La, d)), phase=np.zeros(La), weights=np.ones((La, qa * m)), eps=None if eps is None else np.zeros((N, qa * m)),
               lo=np.full(m - 1, -INF) if lo is None else np.asarray(lo, dtype=float), hi=np.zeros(m - 1) if hi is None else np.asarray(hi, dtype=float),
               best_val=np.empty(2 * qa * ka))  # fmt: skip
    bi = np.empty(2 * qa * ka, dtype=np.int64)
    if bad is not None:
        arr[bad].flat[-1] = np.inf
    p = {n: (None if n == null or a is None else _lib._ptr(a)) for n, a in arr.items()}
    rc = lib.bogp_sweep_thompson_constrained(eng._h, q, L, p["omega"], p["phase"], p["weights"], p["eps"], 1, m - 1 if n_con is None else n_con,
                                             p["lo"], p["hi"], k, p["best_val"], None if null == "best_idx" else bi.ctypes.data_as(C.POINTER(C.c_int64)),
                                             None, None, None)  # fmt: skip
    return rc, lib.bogp_last_error(eng._h).decode()


def test_error_returns():
    """Every error return of bogp_sweep_thompson_constrained but one: a communicator of more than one rank cannot be built on one
    device (its refusal is a comparison of the handle's world size; the Python layer's own refusal is exercised on the host)."""
    lib = _lib.load()
    assert lib.bogp_sweep_thompson_constrained(None, 1, 16, None, None, None, None, 1, 1, None, None, 1, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.bogp_thompson_constrained_last(None, None, None, None, None) == _lib.ERR_INVALID
    e = _lib.Engine(0)
    try:
        X, Y, theta, Xs = TC.problem(100, 3, 67, _lib.KERNEL_SE, 2)
        e.set_train(X, Y)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no committed model" in msg
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "no candidates" in msg
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK and _call(e, eps=True)[0] == _lib.OK and _call(e, q=8)[0] == _lib.OK
        for kw in (dict(q=0), dict(q=9), dict(n_con=2), dict(n_con=0), dict(L=0), dict(L=24), dict(L=_lib.MAX_FEATURES + 16), dict(k=0),
                   dict(k=_lib.MAX_TOPK + 1), dict(null="omega"), dict(null="phase"), dict(null="weights"), dict(null="lo"), dict(null="hi"),
                   dict(null="best_val"), dict(null="best_idx"), dict(lo=[np.nan]), dict(hi=[np.nan]), dict(lo=[1.0], hi=[0.0])):  # fmt: skip
            assert _call(e, **kw)[0] == _lib.ERR_INVALID, kw
        assert "NaN" in _call(e, lo=[np.nan])[1] and "below its lower bound" in _call(e, lo=[1.0], hi=[0.0])[1]
        assert _call(e, lo=[0.5], hi=[0.5])[0] == _lib.OK  # lo == hi is a bound like any other
        for bad in ("omega", "phase", "weights", "eps"):
            rc, msg = _call(e, eps=True, bad=bad)
            assert rc == _lib.ERR_INVALID and bad in msg and "non-finite" in msg
        st = TC.state(X, Y, theta, _lib.KERNEL_SE)
        with pytest.raises(_lib.BogpError) as ei:
            e.sweep_thompson_constrained(thompson.draw_multi(st, 2, 16, seed=0), 2, [-INF], [0.0], k=33)
        assert ei.value.code == _lib.ERR_INVALID
        # a lift on the handle
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "lift" in msg
        with pytest.raises(NotImplementedError, match="lift"):
            e.sweep_thompson_constrained(thompson.draw_multi(st, 2, 16, seed=0), 2, [-INF], [0.0])
        e.clear_lift()
        assert _call(e)[0] == _lib.OK
        # the two modes with a rescaled R
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noisy mode" in msg
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[theta, 0.9], 0.0, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noise-estimating mode" in msg
        # the two kernels without a spectral draw
        e.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISELESS, np.full(3, 2.0), 0.0, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "cubic" in msg
        e.commit(_lib.KERNEL_GENEXP, _lib.MODE_NOISELESS, np.r_[theta, 1.5], 0.0, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "generalized-exponential" in msg
        # one target: a polynomial trend basis is refused by name, the constant one is sent to bogp_sweep_thompson
        e.set_train(X, Y[:, 0])
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
        e.upload_candidates(Xs)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "constant trend" in msg
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, True, 0.0)
        rc, msg = _call(e)
        assert rc == _lib.ERR_INVALID and "bogp_sweep_thompson serves it" in msg
        # and the single-target entry keeps refusing several targets as it did
        e.set_train(X, Y)
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, False, 0.0)
        e.upload_candidates(Xs)
        om, ph, w = np.ones((16, 3)), np.zeros(16), np.ones((16, 2))
        bv, bi = np.empty(2), np.empty(2, dtype=np.int64)
        rc = lib.bogp_sweep_thompson(e._h, 2, 16, _lib._ptr(om), _lib._ptr(ph), _lib._ptr(w), None, 1, 1, 1, _lib._ptr(bv),
                                     bi.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None)  # fmt: skip
        assert rc == _lib.ERR_UNSUPPORTED and "one target" in lib.bogp_last_error(e._h).decode()
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
    """Two faults in one call: the one that comes first in the entry's order of checks -- forest, not committed, no candidates, lift,
    trend columns, one target, n_con, variance count, q m, L, k, null pointers, bounds, non-finite omega / phase / weights / eps, mode,
    kernel, ranks -- is reported."""
    e = _lib.Engine(0)
    try:
        X, Y, theta, Xs = TC.problem(100, 3, 67, _lib.KERNEL_SE, 2)
        e.set_train(X, Y)
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISELESS, theta, 0.0, False, 0.3)
        e.upload_candidates(Xs)
        assert _call(e)[0] == _lib.OK
        for kw, first in ((dict(n_con=2, q=0), "n_con = 2"), (dict(q=9, L=24), "q = 9 members"), (dict(k=0, null="lo"), "k = 0 outside"),
                          (dict(lo=[1.0], hi=[0.0], bad="omega"), "below its lower bound")):  # fmt: skip
            rc, msg = _call(e, **kw)
            assert rc == _lib.ERR_INVALID and first in msg, (kw, msg)
        # a lift on the handle and q = 0: the lift
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _call(e, q=0)
        assert rc == _lib.ERR_UNSUPPORTED and "lift" in msg, msg
        e.clear_lift()
        # non-finite weights and a noisy-mode commit: the non-finite entry
        e.commit(_lib.KERNEL_SE, _lib.MODE_NOISY, np.r_[theta, 0.7], 1e-6, False, 0.3)
        rc, msg = _call(e, bad="weights")
        assert rc == _lib.ERR_INVALID and "weights has a non-finite entry" in msg, msg
        # the noisy mode and the cubic kernel: the mode
        e.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISY, np.r_[np.full(3, 2.0), 0.7], 1e-6, False, 0.3)
        rc, msg = _call(e)
        assert rc == _lib.ERR_UNSUPPORTED and "noisy mode" in msg, msg
    finally:
        e.close()


def test_the_python_batch_on_the_device():
    """`bogp.constrained_thompson_batch` on a real model: q distinct rows, each the member's best row of the device's own scores
    among the rows not yet taken, `fopt` the device's objective path there -- exactly for a feasible proposal, within the path's
    allowance for a least violating one (that value is one row of the restatement on the device's g and the model's gamma)."""
    import bogp
    from bogp import optim

    X, Y, _, Xs = TC.problem(300, 3, 40, _lib.KERNEL_MATERN52, 3, seed=9)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    model.set_state(np.r_[0.6, 0.6, 0.6], X, Y)
    box = optim.Box([(-2.2, 2.2)] * 3, random_seed=3)
    st = thompson.state_of_multi(model)
    dr = thompson.draw_multi(model, 3, 64, seed=4)
    ref = TC.restate(st, dr, Xs)
    for lo, hi in (([-INF, -INF], np.quantile(Y[:, 1:], 0.6, axis=0)), ([40.0, 40.0], [INF, INF])):
        crit = bogp.Constrained(model=model, fun="EI", lo=lo, hi=hi)
        xs, fs = bogp.constrained_thompson_batch(crit, box, 300, q=3, n_features=64, seed=4, Xs=Xs)
        out = model.engine.sweep_thompson_constrained(dr, 3, crit.lo, crit.hi, minimize=True, k=1, return_values=True)
        sel = thompson.select_numpy(out["paths"], crit.lo, crit.hi, st.sigma2, True, 1)
        taken = []
        for j in range(3):
            score = sel["A"][j] if sel["feas"][j].any() else sel["B"][j]
            row = int(np.argmax(np.where(np.isin(np.arange(len(Xs)), taken), -INF, score)))
            taken.append(row)
            assert xs[j] == Xs[row].tolist()
            if sel["feas"][j].any():
                assert fs[j] == float(out["paths"][j, 0, row])
            else:
                assert abs(fs[j] - out["paths"][j, 0, row]) <= ref.tol[j, 0, row]
        assert len(set(taken)) == 3
    model.engine.close()
