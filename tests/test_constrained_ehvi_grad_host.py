"""Input gradient of the feasibility-weighted EHVI, the parts that need no GPU: the NumPy restatement
(tests/support/constrained_ehvi_grad_ref.py) against central differences of the value restatement over the oracle's posterior, the
conditions on the shared cases (tests/constrained_ehvi_grad_cases.py) asserted on the restatement alone, the exact cases,
`ConstrainedEHVI(input_gradient=True)` and the routing of `optim.argmax_restart` / `polish_topk` on the oracle-backed stand-in
(tests/support/constrained_ehvi_grad_engine.py), every refusal by name, and the reference's unmodified `MOBO` under
`install(expensive_constraints=True, constrained_mobo=True, constrained_mobo_gradient=True)`."""
import functools
import os

import numpy as np
import pytest

import constrained_ehvi_grad_cases as K
import test_constrained_ehvi_host as H
from oracle import gp_oracle as O
from support import constrained_ehvi_grad_ref as R
from support import constrained_ehvi_ref as CE
from support.constrained_ehvi_engine import ConstrainedEhviOracleEngine
from support.constrained_ehvi_grad_engine import ConstrainedEhviGradOracleEngine

import bogp
from bogp import optim, pareto

BOX = K.BOX
INF = float("inf")
NAME = "ConstrainedEHVI"


# ----------------------------------------------------------------------------------------------------------------------
# 1. the restatement against central differences
# ----------------------------------------------------------------------------------------------------------------------
def _state(m, c, d, kernel, N=30, seed=0, first=0, no_cells=False):
    """An (m + c)-target oracle state at fixed hyper-parameters (fixed constant trend, as several targets require), the cases' bounds and
    cells.  `no_cells`: a feasibility-only criterion whatever the training rows say."""
    par, mode, X, Y, lo, hi = K.problem(kernel, True, N, d, m, c, first, seed)
    st = O.make_state(par, X, Y, kernel, mode, 0.0, beta=0.0)
    # (the cells of the first training rows' front whether feasible or not: with six constraints no row of 30 is feasible, and any cells
    # serve a derivative check)
    ref = Y[:, :m].min(0) - 0.1 * np.abs(Y[:, :m].min(0))
    lower, upper = pareto.hypercell_bounds(Y[: 8 if m < 5 else 4, :m], ref)
    if no_cells:
        lower = upper = np.zeros((0, m))
    return st, X, Y, lo, hi, lower, upper, np.random.default_rng(seed + 1)


FD_CASES = [  # (kernel, d, m, c, first bound kind, feasibility only): the four kernels, d in {2, 12, 23}, few and many constraints
    (O.KERNEL_SE, 2, 2, 1, 0, False), (O.KERNEL_MATERN32, 2, 2, 6, 1, False), (O.KERNEL_MATERN52, 2, 5, 1, 2, False),
    (O.KERNEL_ABSEXP, 2, 3, 2, 3, False), (O.KERNEL_MATERN52, 12, 2, 2, 0, True), (O.KERNEL_SE, 12, 3, 1, 1, False),
    (O.KERNEL_MATERN32, 12, 7, 1, 0, False), (O.KERNEL_ABSEXP, 12, 2, 3, 2, False), (O.KERNEL_MATERN52, 23, 4, 1, 0, False),
    (O.KERNEL_SE, 23, 2, 1, 3, True), (O.KERNEL_MATERN32, 23, 3, 2, 1, False),
]


@pytest.mark.parametrize("case", FD_CASES, ids=lambda c: "k%d-d%d-m%d-c%d-b%d-%s" % (c[0], c[1], c[2], c[3], c[4], "pof" if c[5] else "cells"))
def test_restatement_against_central_differences(case):
    """Tolerance (ledger T15): the difference quotient's own error, estimated per case as max |FD(h) - FD(h / 2)| with h = 1e-5 of the
    box width, times 10, on rows with value > 1e-8.  The same rows: the restatement's value equals `constrained_ehvi_ref.values` on the
    oracle's moments.  Measured (ledger T27): |grad - FD| is 0.51 .. 1.42 of FD's own estimate over the eleven cases, 0.051 .. 0.142 of the allowance."""
    kernel, d, m, c, first, no_cells = case
    st, X, Y, lo, hi, lower, upper, rng = _state(m, c, d, kernel, seed=100 * m + 10 * kernel + d + c, first=first, no_cells=no_cells)
    assert (len(lower) == 0) == no_cells
    h = 1e-5 * (BOX[1] - BOX[0])

    def value(z):
        mu, mse = O.predict(st, z[None, :])
        return CE.values(mu, mse, st.sigma2, m, lower, upper, lo, hi)[0][0]

    def fd(x, step):
        return np.array([(value(x + step * e) - value(x - step * e)) / (2 * step) for e in np.eye(d)])

    err = own = scale = 0.0
    n = tries = 0
    while n < 4:
        tries += 1
        assert tries < 400, "no row with a value to differentiate"
        x = rng.uniform(BOX[0] + 0.1, BOX[1] - 0.1, size=d)  # away from the training set (a continuous draw)
        v, g, P, dP, E, dE = R.at(st, x, m, lower, upper, lo, hi)[:6]
        if not (v > 1e-8 and np.abs(g).max() > 0):
            continue
        n += 1
        np.testing.assert_allclose(v, value(x), rtol=1e-9, atol=0)
        a, b = fd(x, h), fd(x, h / 2)
        err, own, scale = max(err, np.abs(g - a).max()), max(own, np.abs(a - b).max()), max(scale, np.abs(g).max())
    print("T27 %s: |grad - FD| / max|grad| = %.3g, FD's own error estimate %.3g (ratio %.3g of the allowance)"
          % (case, err / scale, own / scale, err / (10.0 * own)))  # fmt: skip
    assert scale > 0 and err <= 10.0 * own


# ----------------------------------------------------------------------------------------------------------------------
# 2. conditions on the shared cases, from the restatement alone
# ----------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference_of(cfg):
    """(problem, oracle state, restatement of the 33 rows): computed once per configuration."""
    if cfg.i not in _REF:
        p = cfg.build()
        st = O.make_state(p["par"], p["X"], p["Y"], cfg.kernel, p["mode"], 0.0, beta=0.0)
        _REF[cfg.i] = (p, st, R.batch(st, p["rows"], cfg.m, p["lower"], p["upper"], p["lo"], p["hi"]))
    return _REF[cfg.i]


@pytest.mark.parametrize("cfg", K.CONFIGS, ids=K.IDS)
def test_every_configuration_is_well_posed(cfg):
    p, st, ref = reference_of(cfg)
    val, dval, P, dP, E, dE, mu, mse = ref[:8]
    assert p["rows"].shape == (K.ROWS, cfg.d) and len(p["lo"]) == cfg.c and p["lower"].shape[1] == cfg.m
    alive = np.all(mse > 0, axis=1) & (P > 0) & (val > 0) & (np.abs(dval).max(axis=1) > 0) & np.all(np.isfinite(dval), axis=1)
    print("%s: cells %d, alive %.2f, P in [%.3g, %.3g]" % (cfg.id, len(p["lower"]), alive.mean(), P.min(), P.max()))
    assert alive.mean() >= 0.5
    assert P.max() > P.min()  # not one constant
    # no row AT the small-variance guard sd / sqrt(sigma2) = 1e-6: a variance is either clipped to exactly 0 (deep inside on either
    # side of a rounding) or two decades clear of it
    ratio = np.sqrt(mse / np.asarray(st.sigma2, float).ravel())
    assert np.all((ratio == 0.0) | (ratio > 1e-4))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(dval))  # a gradient is never NaN where the value is finite
    dead = P == 0.0
    assert np.all(val[dead] == 0.0) and not np.any(np.signbit(val[dead])) and np.all(dval[dead] == 0.0)


def test_the_list_holds_both_ends_of_the_cell_count():
    counts = [len(cfg.build()["lower"]) for cfg in K.CONFIGS]
    assert len(K.CONFIGS) == 27 and min(counts) == 0 and max(counts) > 10_000
    assert {(c.m, c.c) for c in K.CONFIGS} == set(K.PAIRS) and {c.kernel for c in K.CONFIGS} == set(K.KERNELS)
    assert {c.B for c in K.CONFIGS} == {1, 33} and {c.noisy for c in K.CONFIGS} == {True, False}
    assert {(c.N, c.d) for c in K.CONFIGS} == {(N, d) for N in (37, 100, 157) for d in (2, 12, 23)}


POLISH_CASE = 20  # N = 157, d = 2, (m, c) = (2, 2), noiseless: the device test of the polish starts from its first 8 rows


def test_every_start_of_the_polish_case_has_a_projected_gradient():
    """What the device test's `sum(fout) > sum(f0)` rests on: inside the box each of the 8 starts has a non-zero gradient component that
    does not point out of the box, so a first step improves it."""
    cfg = K.CONFIGS[POLISH_CASE]
    assert (cfg.N, cfg.d, cfg.m, cfg.c) == (157, 2, 2, 2)
    p, st, ref = reference_of(cfg)
    x, g = p["rows"][:8], ref[1][:8]
    assert np.all(ref[0][:8] > 0)
    free = ((g > 0) & (x < BOX[1])) | ((g < 0) & (x > BOX[0]))
    assert np.all(np.any(free, axis=1))


# ----------------------------------------------------------------------------------------------------------------------
# 3. exact cases on the restatement and the stand-in
# ----------------------------------------------------------------------------------------------------------------------
def test_lo_equal_hi_is_plus_zero_with_a_zero_gradient():
    st, X, Y, lo, hi, lower, upper, rng = _state(3, 2, 2, O.KERNEL_MATERN52, seed=3)
    lo, hi = lo.copy(), hi.copy()
    lo[1] = hi[1] = float(np.median(Y[:, 4]))
    out = R.batch(st, rng.uniform(*BOX, size=(6, 2)), 3, lower, upper, lo, hi)
    assert np.array_equal(out[0], np.zeros(6)) and not np.any(np.signbit(out[0])) and np.array_equal(out[1], np.zeros((6, 2)))
    assert np.array_equal(out[2], np.zeros(6)) and np.array_equal(out[3], np.zeros((6, 2)))
    assert np.array_equal(out[4], np.zeros(6)) and np.array_equal(out[5], np.zeros((6, 2)))  # the cells are not read


def test_every_bound_infinite_is_ehvi_itself():
    from support import ehvi_grad_ref as ER

    st, X, Y, _, _, lower, upper, rng = _state(3, 2, 12, O.KERNEL_SE, seed=5)
    rows = rng.uniform(*BOX, size=(5, 12))
    val, dval, P, dP, E, dE = R.batch(st, rows, 3, lower, upper, np.full(2, -INF), np.full(2, INF))[:6]
    assert np.array_equal(P, np.ones(5)) and np.array_equal(dP, np.zeros((5, 12)))
    assert np.array_equal(val, E) and np.array_equal(dval, dE) and np.all(E > 0)
    for b, x in enumerate(rows):  # ... and E is the EHVI restatement of the objective columns' moments
        mu, mse, dmu, dmse = ER.moments(st, x)
        e, c_mu, c_sd, sd = ER.ehvi_and_coefficients(mu[:3], mse[:3], lower, upper)
        assert E[b] == e


def test_no_cells_is_the_gradient_of_the_probability():
    st, X, Y, lo, hi, _, _, rng = _state(2, 3, 12, O.KERNEL_MATERN32, seed=6, no_cells=True)
    none = np.zeros((0, 2))
    val, dval, P, dP, E, dE = R.batch(st, rng.uniform(*BOX, size=(5, 12)), 2, none, none, lo, hi)[:6]
    assert np.array_equal(val, P) and np.array_equal(dval, dP) and np.any(dP != 0) and np.all(E == 0) and np.all(dE == 0)


def test_the_clamp_at_a_training_row_of_a_noiseless_model():
    """On a training row of a noiseless model every MSE_k is rounding noise below the 1e-9 clamp: sd_k is the clamp's constant, the sd
    path is exactly absent, and the gradient is finite (the mean path alone)."""
    m, c, d = 2, 1, 2
    par, mode, X, Y, lo, hi = K.problem(O.KERNEL_MATERN52, False, 40, d, m, c, 0, seed=8)
    st = O.make_state(par, X, Y, O.KERNEL_MATERN52, mode, 0.0, beta=0.0)
    lo, hi = np.array([-INF]), np.array([INF])  # P = 1: the criterion is E
    ref, lower, upper, _ = K.cells(Y, m, lo, hi)
    out = R.at(st, X[3], m, lower, upper, lo, hi)
    val, dval, P, dP, E, dE, mu, mse, dmu, dmse = out
    assert np.all(mse <= 1e-9) and P == 1.0 and np.all(np.isfinite(dval)) and np.all(np.isfinite(dE))
    from support import ehvi_grad_ref as ER

    e, c_mu, c_sd, sd = ER.ehvi_and_coefficients(mu[:m], mse[:m], lower, upper)
    assert np.array_equal(dE, sum(R.CG._times(c_mu[k], dmu[k]) for k in range(m)))  # no sd path


# ----------------------------------------------------------------------------------------------------------------------
# 4. ConstrainedEHVI(input_gradient=True) on the stand-in engine
# ----------------------------------------------------------------------------------------------------------------------
def _gp(seed=1, engine=ConstrainedEhviGradOracleEngine):
    X, Y, Xs = H._toy(seed)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(2, beta=0.0), corr="matern52", thetaL=[1e-3] * 2, thetaU=[1e3] * 2, nugget=0)
    model._engine = engine()
    model.set_state(np.full(2, 60.0), X, Y)
    return model, Y, Xs


def _crit(model, Y, **kw):
    return bogp.ConstrainedEHVI(model=model, ref_point=Y[:, :2].min(0) - 0.1, **kw)


def _box(seed=None):
    return optim.Box([(0, 1), (0, 1)], random_seed=seed)


def test_return_shapes_and_values():
    model, Y, Xs = _gp()
    crit, plain = _crit(model, Y, input_gradient=True), _crit(model, Y)
    assert crit.input_gradient and not plain.input_gradient and optim.is_constrained_ehvi(crit) and optim.is_ehvi(crit)
    eng = model.engine
    C = len(crit.cell_lower_bounds)
    v1, g1 = crit(Xs[:1], return_dx=True)
    assert v1.shape == (1,) and g1.shape == (1, 2)  # EHVI(input_gradient=True)'s one-row shapes
    v5, g5 = crit(Xs[:5], return_dx=True)
    assert v5.shape == (5, 1) and g5.shape == (5, 2)  # ... and its M-row shapes
    assert v5[0, 0] == v1[0] and np.array_equal(g5[0], g1[0])
    eng.calls.clear()
    vals = crit(Xs[:5])  # at most 64 rows: the same call
    assert vals.shape == (5,) and eng.calls == [("point_eval_ehvi_constrained", 5, 2, C)]
    np.testing.assert_allclose(vals, plain(Xs[:5]), rtol=1e-10, atol=0)  # (the sweep path of the stand-in: the chunked posterior)
    eng.calls.clear()
    assert crit(Xs[:65]).shape == (65,) and eng.calls[-1][0] == "sweep_ehvi_constrained"
    vr, gr = R.at(eng.st, Xs[0], 2, crit.cell_lower_bounds, crit.cell_upper_bounds, crit.lo, crit.hi)[:2]
    assert v1[0] == vr and np.array_equal(g1[0], gr)
    # a feasibility-only criterion (no feasible row, no cells) has the gradient of P
    none = _crit(model, Y, lo=[-INF], hi=[Y[:, 2].min() - 1.0], input_gradient=True)
    assert none.feasibility_only
    v, g = none(Xs[:3], return_dx=True)
    want = R.batch(eng.st, Xs[:3], 2, none.cell_lower_bounds, none.cell_upper_bounds, none.lo, none.hi)
    assert eng.calls[-1] == ("point_eval_ehvi_constrained", 3, 2, 0)
    assert np.array_equal(v[:, 0], want[2]) and np.array_equal(g, want[3])


@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS", "sweep-device-BFGS"])
def test_polish_optimisers_reach_at_least_the_sweep_winner(optimizer):
    """The hybrids polish the sweep's own top rows (same candidates under the same seed), so their result is >= the sweep's winner by
    construction.  "BFGS" (10 restarts of L-BFGS-B from uniform starts) is compared with the best of as many uniform rows."""
    model, Y, Xs = _gp()
    crit = _crit(model, Y, input_gradient=True)
    eng = model.engine
    C = len(crit.cell_lower_bounds)
    sweep_of = {"BFGS": "sweep", "sweep-BFGS": "sweep", "sweep-device-BFGS": "sweep-device"}[optimizer]
    budget = 10 if optimizer == "BFGS" else 200
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, _box(seed=7), eval_budget=budget, optimizer=sweep_of)
    eng.calls.clear()
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, _box(seed=7), eval_budget=200, n_restart=10, optimizer=optimizer)
    print("%s: sweep winner %.6g, result %.6g" % (optimizer, fs, fp))
    assert fp >= fs
    assert all(0.0 <= v <= 1.0 for v in xp) and len(xp) == 2
    np.testing.assert_allclose(fp, crit(np.array([xp]))[0], rtol=1e-12)
    sweeps = [c for c in eng.calls if c[0] == "sweep_ehvi_constrained"]
    if optimizer != "BFGS":
        assert sweeps[0] == ("sweep_ehvi_constrained", 2, C, 10)  # crit.sweep(k), then the polish (sequential fall-back here)
    else:
        assert not sweeps
    assert ("point_eval_ehvi_constrained", 1, 2, C) in eng.calls
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in eng.calls)  # never without the constraints
    if optimizer == "sweep-BFGS":  # the reference's wrapper around the criterion (functools.partial, as MOBO._create_acquisition wraps it)
        np.random.seed(4)
        x2, f2 = optim.argmax_restart(functools.partial(crit, return_dx=False), _box(seed=7), eval_budget=200, n_restart=10, optimizer=optimizer)
        assert x2 == xp and f2 == fp


def test_polish_topk_dispatches_to_the_engine_polish():
    model, Y, Xs = _gp()
    crit = _crit(model, Y, input_gradient=True, lo=[-0.5], hi=[0.25])
    seen = {}

    def polish_ehvi_constrained(starts, box_lo, box_hi, lower, upper, lo, hi, max_evals=50):
        seen.update(starts=np.array(starts), box_lo=np.array(box_lo), box_hi=np.array(box_hi), lower=lower, upper=upper, lo=lo, hi=hi,
                    max_evals=max_evals)  # fmt: skip
        return np.array(starts) + 0.0, np.arange(len(starts), dtype=float), np.ones(len(starts), dtype=np.int32)

    def polish_ehvi(*a, **k):
        raise AssertionError("the EHVI polish would drop the constraints")

    model.engine.polish_ehvi_constrained, model.engine.polish_ehvi = polish_ehvi_constrained, polish_ehvi
    starts = np.array([[0.1, 0.2], [0.3, 0.4], [9.0, 9.0]])
    xs, fs = optim.polish_topk(crit, starts, np.array([[0.0, 1.0], [0.0, 1.0]]), max_iter=17)
    assert np.array_equal(xs, starts) and fs.tolist() == [0.0, 1.0, 2.0]
    assert seen["max_evals"] == 17 and seen["box_lo"].tolist() == [0.0, 0.0] and seen["box_hi"].tolist() == [1.0, 1.0]
    assert seen["lower"] is crit.cell_lower_bounds and seen["upper"] is crit.cell_upper_bounds
    assert seen["lo"] is crit.lo and seen["hi"] is crit.hi
    # without the flag the polish keeps its refusal even on an engine that has the entry
    with pytest.raises(NotImplementedError, match="has no polish"):
        optim.polish_topk(_crit(model, Y), starts, np.array([[0.0, 1.0], [0.0, 1.0]]))


# ----------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_default_object_still_refuses_in_its_present_words():
    model, Y, Xs = _gp()
    plain = _crit(model, Y)
    with pytest.raises(NotImplementedError, match=r"constrained EHVI \(bogp.ConstrainedEHVI\) has no input gradient: use 'sweep' or"):
        plain(Xs[:1], return_dx=True)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match=r"optimizer='%s' for constrained EHVI \(bogp.ConstrainedEHVI\): it has no input gradient "
                                                      r"and no polish; use 'sweep' or" % name):  # fmt: skip
            optim.argmax_restart(plain, _box(), eval_budget=10, optimizer=name)
    with pytest.raises(NotImplementedError, match=r"has no polish: bogp_polish_ehvi knows the objectives only and would drop the constraints"):
        optim.polish_topk(plain, Xs[:3], np.array([[0.0, 1.0], [0.0, 1.0]]))
    model.engine.calls.clear()
    plain(Xs[:3])  # the default object never takes the point call
    assert [c[0] for c in model.engine.calls] == ["upload", "sweep_ehvi_constrained"]


def test_refusals_by_name(monkeypatch):
    model, Y, Xs = _gp()
    crit = _crit(model, Y, input_gradient=True)
    masks, values = np.array([False, True, False]), [0.5]

    @functools.wraps(functools.partial(crit))
    def fixed(X):  # the shape of the reference's partial_argument wrapper (utils.py:184-213): `masks` / `values` in its closure
        full = np.empty((1, len(masks)))
        full[:, ~masks], full[:, masks] = X, values
        return crit(full)

    fixed.__wrapped__ = functools.partial(crit)
    assert optim.unwrap_criterion(fixed)[0] is crit and optim.unwrap_criterion(fixed)[1] is not None
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="%s.*fixed variables" % NAME):
            optim.argmax_restart(fixed, _box(), eval_budget=20, optimizer=name)
        with pytest.raises(NotImplementedError, match="%s.*cheap constraints h / g" % NAME):
            optim.argmax_restart(crit, _box(), g=lambda x: -1.0, eval_budget=20, optimizer=name)
        with pytest.raises(NotImplementedError, match="%s.*cheap constraints h / g" % NAME):
            optim.argmax_restart(crit, _box(), h=lambda x: 0.0, eval_budget=20, optimizer=name)
    for name in ("sweep-BFGS", "sweep-device-BFGS"):
        lifted = functools.partial(lambda x, **kw: 0.0, acquisition_func=functools.partial(crit), bounds=np.array([[0.0, 1.0]] * 2), pca=object())
        with pytest.raises(NotImplementedError, match="lift"):
            optim.argmax_restart(lifted, _box(), eval_budget=20, optimizer=name)
    # every batch strategy
    for call in (lambda: optim.believer_batch([crit, crit], _box(), 100), lambda: optim.batch_argmax([crit, crit], _box(), 100, strategy="believer"),
                 lambda: optim.ehvi_believer_batch(crit, _box(), 100, 2), lambda: optim.constrained_believer_batch(crit, _box(), 100, q=2),
                 lambda: optim.batch_argmax([crit, crit], _box(), 100, strategy="thompson"),
                 lambda: optim.thompson_batch(model, _box(), 100, 2, criteria=[crit])):  # fmt: skip
        with pytest.raises(NotImplementedError, match=NAME):
            call()
    monkeypatch.setattr(ConstrainedEhviGradOracleEngine, "comm_world", 2, raising=False)
    monkeypatch.setattr(ConstrainedEhviGradOracleEngine, "comm_rank", 0, raising=False)
    for name in ("BFGS", "sweep-BFGS", "sweep-device-BFGS"):
        with pytest.raises(NotImplementedError, match="%s.*one rank" % NAME):
            optim.argmax_restart(crit, _box(), eval_budget=20, optimizer=name)
    monkeypatch.undo()
    # an engine without the point call says so
    model2, Y2, _ = _gp(engine=ConstrainedEhviOracleEngine)
    with pytest.raises(NotImplementedError, match="point_eval_ehvi_constrained"):
        _crit(model2, Y2, input_gradient=True)(np.zeros((1, 2)), return_dx=True)
    assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in model.engine.calls)


# ----------------------------------------------------------------------------------------------------------------------
# 6. the reference's MOBO under install(expensive_constraints=True, constrained_mobo=True, constrained_mobo_gradient=True)
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def reference(monkeypatch):
    if not os.path.isdir(os.path.join(H.REF, "bayes_optim")):
        pytest.skip("reference tree not present")
    bayes_optim = H._ref_modules()
    monkeypatch.setattr(bogp._lib, "Engine", ConstrainedEhviGradOracleEngine)
    yield bayes_optim
    bogp.uninstall()


def test_install_keyword_rules():
    with pytest.raises(ValueError, match="constrained_mobo_gradient=True needs constrained_mobo=True"):
        bogp.install(object(), constrained_mobo_gradient=True)
    with pytest.raises(ValueError, match="constrained_mobo_gradient=True needs constrained_mobo=True"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo_gradient=True)
    from bogp import integration

    assert not integration._CONSTRAINTS.get("mobo_gradient") and not integration._ORIGINAL  # nothing was installed


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["sweep-device-BFGS", "BFGS"])
def test_the_reference_mobo_asks_through_the_new_calls(reference, optimizer):
    bayes_optim = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True, constrained_mobo_gradient=True)
    np.random.seed(4)
    opt, model = H._mobo(bayes_optim, optimizer=optimizer)
    assert type(model).__module__.startswith("bogp")
    X = opt.ask()  # the DoE
    f, g = H._evaluate(X)
    opt.tell(X, f, g_vals=g)
    assert model.y.shape == (8, 3)
    for _ in range(2):
        eng = model.engine
        eng.calls.clear()
        X = opt.ask(1)
        eng = model.engine
        assert len(X) == 1 and all(0.0 <= v <= 1.0 for v in X[0])
        assert any(c[0] == "point_eval_ehvi_constrained" and c[1] == 1 and c[2] == 2 for c in eng.calls)  # the gradient call served the ask ...
        sweeps = [c for c in eng.calls if c[0] == "sweep_ehvi_constrained"]
        assert (len(sweeps) == 1 and sweeps[0][1] == 2 and sweeps[0][3] > 1) if optimizer != "BFGS" else (not sweeps)
        assert not any(c[0] in ("sweep", "sweep_topk", "sweep_ehvi", "sweep_constrained") for c in eng.calls)  # ... never without the constraints
        f, g = H._evaluate(X)
        opt.tell(X, f, g_vals=g)
    wrapper = opt._create_acquisition()
    crit = optim.unwrap_criterion(wrapper)[0]
    assert isinstance(crit, bogp.ConstrainedEHVI) and crit.input_gradient and model.y.shape[1] == 3
    if optimizer == "BFGS":  # return_dx bound as BO._create_acquisition binds it: the reference's loop gets (value, gradient)
        out = wrapper(np.array([0.4, 0.6]))
        assert isinstance(out, tuple) and len(out) == 2 and np.asarray(out[1]).size == 2
    # the sweep family keeps the default object
    opt._optimizer = "sweep"
    assert not optim.unwrap_criterion(opt._create_acquisition())[0].input_gradient


@pytest.mark.timeout(900)
@pytest.mark.parametrize("optimizer", ["BFGS", "sweep-BFGS", "sweep-device-BFGS"])
def test_without_the_switch_the_driver_raises_as_before(reference, optimizer):
    bayes_optim = reference
    bogp.install(bayes_optim, expensive_constraints=True, constrained_mobo=True)
    np.random.seed(4)
    opt, model = H._mobo(bayes_optim, optimizer=optimizer)
    X = opt.ask()
    f, g = H._evaluate(X)
    opt.tell(X, f, g_vals=g)
    with pytest.raises(NotImplementedError, match=r"optimizer='%s' under expensive constraints of a multi-objective run: constrained EHVI "
                                                  r"\(bogp.ConstrainedEHVI\) is served by the sweep family only" % optimizer):  # fmt: skip
        opt.ask(1)
