"""The polish of Thompson batches under modelled constraints on the device: `bogp_point_eval_path_feasible`
(kernels_point_path_feasible.hip) against the dense restatement `thompson.feasible_merit_numpy` on the SAME draw, its y and J bit for bit
against `bogp_point_eval_path_hvi` and within T30's allowance of the constrained sweeps' paths, merit and gradient byte for byte from the
scalarisation restated on the device's own y and J; bit-identity across B, position, neighbours and outputs asked for;
`bogp_polish_path_feasible`; the two Python batches; the error returns.
Allowances (ledger T32's form, per target): |y - ref| <= ptol (|ref| + A_v), |J - ref| <= ptol (|ref| + A_g), ptol = max(1e-6, 100 cond(R)
eps), A the sums of the absolute terms.  Conditions, asserted per shape on the restatement alone: every y_k and c_i is farther than 1e3
allowances from every cell face and every polish bound, so the device's values lie in the same cells and on the same side of every
bound; at least a quarter of the points has P > 0 and at least a quarter F != 0 with a non-zero objective weight, so no term can be
missing.  The polish bounds are the middles of the widest gaps of the restated constraint values between their 0.3 and 0.7 quantiles
(odd constraints bounded below, even ones above), the cells and the short length scale tests/test_gpu_thompson_ehvi_polish.py's.
rho = 0 against `bogp_point_eval_path_hvi` / `bogp_polish_path_hvi`: the sibling takes cells of all m columns, so the objective cells
are extended by [l, l + 1] per constraint column, l an integer more than 1 below every drawn c: that factor is (l + 1) - l = 1.0
exactly and its weight 0.  The merit then is HVI f_scale bit for bit, at the start and at Xout.  Xout itself is NOT compared with
`polish_path_hvi`'s to the last bit: L-BFGS iterates survive a scaling bit for bit only by a power of two, which f_scale is not.
Measured on an MI355X (ledger T34): y <= 8.6e-10 of the allowance, J <= 1.9e-9, against the sweeps' paths <= 8.9e-10."""
import numpy as np
import pytest

import bogp
import thompson_constrained_cases as TC
from bogp import _lib, optim, thompson
from test_gpu_thompson_constrained import commit
from test_gpu_thompson_ehvi import eng  # noqa: F401  (its module-scoped engine fixture)
from test_gpu_thompson_ehvi_polish import AE, INVALID, M12, M32, M52, SE, SHORT, STATES, UNSUPPORTED, cells_of

pytestmark = pytest.mark.gpu
B, RHO = 33, 100.0
# (N, d, L, m_obj, n_con, q, C, kernel, minimize): N = 1024 / 1025 the row tile of m <= 4, 512 / 513 that of m > 4; d = 64 / 65 the k-pass;
# L = 1040 one step above the feature tile; C = 255 / 257 the two sides of one cell a thread; MT = 2, 3, 4 and 8; m_obj = 1 has no cells
ROWS = [(1, 1, 16, 1, 1, 8, 0, SE, True), (255, 2, 16, 1, 3, 4, 0, M52, False), (255, 63, 1040, 2, 1, 5, 1, SE, 0), (255, 64, 16, 3, 5, 2, 255, M52, 0),
        (255, 65, 16, 1, 1, 8, 0, SE, False), (512, 20, 16, 3, 5, 2, 257, SE, 0), (513, 20, 1040, 3, 5, 2, 1, M52, 0), (513, 65, 16, 3, 5, 2, 255, SE, 0),
        (1024, 20, 1040, 2, 1, 5, 255, SE, 0), (1025, 20, 16, 1, 3, 4, 0, M52, True), (1025, 5, 16, 2, 2, 4, 257, SE, 0), (1024, 5, 16, 3, 1, 4, 257, M52, 0),
        (1, 1, 1040, 3, 5, 2, 257, SE, 0), (255, 20, 16, 1, 1, 8, 0, M12, True), (255, 5, 16, 2, 1, 5, 257, M32, 0), (255, 5, 48, 2, 1, 5, 255, AE, 0)]  # fmt: skip


def polish_bounds(c, al):
    """(plo, phi) for the constraint values c (B, n_con) with allowances al: per constraint ONE finite bound, the middle of the widest gap
    between the 0.3 and 0.7 quantiles that stands farther than 1.2e3 allowances from every value -- a lower bound for odd i, an upper
    one for even i, so both signs of the penalty's weight occur."""
    plo, phi = np.full(c.shape[1], -np.inf), np.full(c.shape[1], np.inf)
    for i in range(c.shape[1]):
        v = np.sort(c[:, i])
        a, b = int(0.3 * len(v)), int(0.7 * len(v))
        mids = [(v[j] + v[j + 1]) / 2 for j in a + np.argsort(np.diff(v[a : b + 1]))[::-1]]
        f = [f for f in mids if np.all(np.abs(c[:, i] - f) > 1.2e3 * al[:, i])]
        assert f, "constraint %d: no bound stands clear of the values" % i
        (plo if i % 2 else phi)[i] = f[0]
    return plo, phi


def setup(eng, row, seed, Bn=B):  # noqa: F811
    N, d, L, mo, nc, q, C, kernel, minimize = row
    X, Y, theta, Xs = TC.problem(Bn, d, N, kernel, mo + nc)
    Xs[8 : 8 + min(N, 4)] = X[: min(N, 4)]  # rows 0 .. 7 stand 0.01 off a training row, these ON one
    st = commit(eng, X, Y, theta * SHORT.get(kernel, 1.0), kernel)
    dr = thompson.draw_multi(st, q, L, seed=seed)
    members = (np.arange(Bn)[::-1] * 7 + seed) % q  # repeated and out of order
    eng.upload_candidates(Xs)
    open_ = (np.full(nc, -np.inf), np.full(nc, np.inf))
    if mo == 1:
        sweep = eng.sweep_thompson_constrained(dr, q, *open_, minimize=bool(minimize), return_values=True)
    else:
        sweep = eng.sweep_thompson_ehvi_constrained(dr, q, np.zeros((1, mo)), np.full((1, mo), np.inf), *open_, return_values=True)
    return st, dr, Xs, members, sweep


def restated(st, dr, Xs, members, row):
    """The restatement of a shape: (parts of y and J with allowances, cells or None, faces, polish bounds)."""
    mo, C, m = row[3], row[6], row[3] + row[4]
    _, _, p = thompson.hvi_grad_numpy(st, dr, Xs, members, np.zeros((1, m)), np.full((1, m), np.inf), parts=True)
    ptol = max(1e-6, 100 * np.linalg.cond(thompson.correlation(st, st.X, st.X)) * TC.EPS)
    p["al_y"], p["al_J"] = ptol * (np.abs(p["y"]) + p["A_v"]), ptol * (np.abs(p["jac"]) + p["A_g"])
    lower, upper, faces = cells_of(p["y"][:, :mo], p["al_y"][:, :mo], C) if mo >= 2 else (None, None, np.empty((0, 3)))
    return p, lower, upper, faces, polish_bounds(p["y"][:, mo:], p["al_y"][:, mo:])


@pytest.mark.parametrize("cfg", range(len(ROWS)))
def test_values_and_gradients_against_the_restatement_the_sibling_and_the_sweep(eng, cfg):  # noqa: F811
    N, d, L, mo, nc, q, C, kernel, minimize = ROWS[cfg]
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)
    ref, b, m = TC.restate(st, dr, Xs), np.arange(B), mo + nc
    assert ref.cond <= 1e8, ref.cond
    p, lower, upper, faces, (plo, phi) = restated(st, dr, Xs, members, ROWS[cfg])
    merit, grad, s = thompson.feasible_scalarise_numpy(p["y"], p["jac"], mo, lower, upper, plo, phi, st.sigma2, minimize, RHO)
    # the conditions: no value near a face or a bound; penalty and objective term alive
    gaps = [np.abs(p["y"][:, mo:] - bd) / p["al_y"][:, mo:] for bd in (plo, phi)]
    gaps += [np.abs(p["y"][:, :mo, None] - faces[None]) / p["al_y"][:, :mo, None]] if mo >= 2 else []
    assert min(float(np.min(g)) for g in gaps) > 1e3
    assert np.count_nonzero(s["P"]) >= -(-B // 4) and np.count_nonzero((s["F"] != 0) & np.any(s["W"] != 0, axis=1)) >= -(-B // 4)
    ops = (dr, sweep["coef"], members, lower, upper, plo, phi)
    dm, dg, dy, dJ = eng.point_eval_path_feasible(Xs, *ops, minimize=minimize, rho=RHO)
    e_y, e_J = float(np.max(np.abs(dy - p["y"]) / p["al_y"])), float(np.max(np.abs(dJ - p["jac"]) / p["al_J"]))
    e_s = float(np.max(np.abs(dy - sweep["paths"][members, :, b]) / ref.tol[members, :, b]))  # the sweep's paths on the same rows (T30)
    print("cfg %2d %s ptol %.1e: ratio to the allowance y %.3g J %.3g sweep %.3g" % (cfg, ROWS[cfg], ref.ptol, e_y, e_J, e_s))
    assert max(e_y, e_J, e_s) <= 1.0, (e_y, e_J, e_s)
    rm, rg = thompson.feasible_merit_numpy(None, None, None, None, mo, lower, upper, plo, phi, minimize, RHO, from_device=(dy, dJ), sigma2=st.sigma2)
    np.testing.assert_array_equal(dm, rm), np.testing.assert_array_equal(dg, rg)  # byte for byte from the device's own y, J
    _, _, hy, hJ = eng.point_eval_path_hvi(Xs, dr, sweep["coef"], members, np.zeros((1, m)), np.full((1, m), np.inf))  # the same columns as m objectives
    np.testing.assert_array_equal(dy, hy), np.testing.assert_array_equal(dJ, hJ)


@pytest.mark.parametrize("cfg", [6, 9])
def test_a_points_outputs_do_not_depend_on_its_company(eng, cfg):  # noqa: F811
    mo, q = ROWS[cfg][3], ROWS[cfg][5]
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)
    y0 = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(B)]
    lower, upper = cells_of(y0[:, :mo], np.zeros_like(y0[:, :mo]), ROWS[cfg][6])[:2] if mo >= 2 else (None, None)
    plo, phi = polish_bounds(y0[:, mo:], np.zeros_like(y0[:, mo:]))
    ev = lambda X, mem, **kw: eng.point_eval_path_feasible(X, dr, sweep["coef"], mem, lower, upper, plo, phi, minimize=ROWS[cfg][8], **kw)  # noqa: E731
    full = ev(Xs, members)  # B = 33
    order = np.random.default_rng(cfg).permutation(17)  # B = 17: another position, beside other members
    beside = np.r_[members[order[0]], (members[order[1:]] + 1) % q]
    cases = [(i, ev(Xs[i], [members[i]])) for i in (0, 5, 32)] + [(order[0], ev(Xs[order], beside))]  # B = 1
    for i, got in cases:
        for a, f in zip(got, full):
            np.testing.assert_array_equal(a[0], f[i])
    bare = ev(Xs, members, jacobian=False)  # with and without jac_out
    assert bare[3] is None and all(np.array_equal(a, f) for a, f in zip(bare[:3], full[:3]))


@pytest.mark.parametrize("cfg", [1, 10, 11])
def test_polish(eng, cfg):  # noqa: F811
    d, mo, minimize, lo, hi, max_evals = ROWS[cfg][1], ROWS[cfg][3], ROWS[cfg][8], -2.0, 2.1, 25
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg, 40)  # rows in [-2.2, 2.2]: some starts lie outside the box and are clipped
    y0 = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(40)]
    lower = np.quantile(y0[:, :mo], 0.4, axis=0)[None] if mo >= 2 else None  # one cell above the 0.4 quantiles: many starts have HVI = 0
    upper, box = None if lower is None else np.full_like(lower, np.inf), (np.full(d, lo), np.full(d, hi))
    plo, phi = np.full(ROWS[cfg][4], -np.inf), np.quantile(y0[:, mo:], 0.6, axis=0)
    ops = (dr, sweep["coef"], members, lower, upper, plo, phi)
    ev = lambda X: eng.point_eval_path_feasible(X, *ops, minimize=minimize, rho=RHO)  # noqa: E731
    xp, fp, ne = eng.polish_path_feasible(Xs, *box, *ops, minimize=minimize, rho=RHO, max_evals=max_evals)
    x0 = np.clip(Xs, lo, hi)
    f0, yc = ev(x0)[::2]  # merit, y
    assert np.all(xp >= lo) and np.all(xp <= hi) and np.all(ne >= 1) and np.all(ne <= max_evals)
    np.testing.assert_array_equal(fp, ev(xp)[0])
    assert np.all(fp >= f0) and np.any(fp > f0)  # no start got worse, some climbed
    if mo >= 2:  # HVI = 0 and P = 0: a zero gradient; back unchanged after one evaluation
        flat = (f0 == 0.0) & np.all(yc[:, mo:] <= phi, axis=1)
        assert flat.any() and np.array_equal(xp[flat], x0[flat]) and np.all(ne[flat] == 1) and np.all(fp[flat] == 0.0)


@pytest.mark.parametrize("cfg", [2, 7, 10])
def test_without_a_penalty_the_merit_is_the_siblings_scaled_hvi(eng, cfg):  # noqa: F811
    d, mo, nc = ROWS[cfg][1], ROWS[cfg][3], ROWS[cfg][4]
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)
    y0 = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(B)]
    lower, upper, _ = cells_of(y0[:, :mo], np.zeros_like(y0[:, :mo]), ROWS[cfg][6])
    plo, phi = polish_bounds(y0[:, mo:], np.zeros_like(y0[:, mo:]))  # bounds that many points violate: rho = 0 must silence them
    lc = np.full((len(lower), nc), np.floor(y0[:, mo:].min()) - 20.0)  # 20 below the starts' values: every polished c stays above l + 1 (asserted)
    ext, box = (np.hstack([lower, lc]), np.hstack([upper, lc + 1.0])), (np.full(d, -2.0), np.full(d, 2.1))
    f_scale = np.multiply.accumulate(1.0 / np.sqrt(st.sigma2[:mo]))[-1]  # inv_sd_0, then times inv_sd_k in order, as the host forms it
    ops = (dr, sweep["coef"], members, lower, upper, plo, phi)
    hvi_at = lambda X: eng.point_eval_path_hvi(X, dr, sweep["coef"], members, *ext)[0]  # noqa: E731
    dm, dg, dy, dJ = eng.point_eval_path_feasible(Xs, *ops, rho=0.0)
    np.testing.assert_array_equal(dm, hvi_at(Xs) * f_scale)
    rm, rg, p = thompson.feasible_merit_numpy(None, None, None, None, mo, lower, upper, plo, phi, rho=0.0, from_device=(dy, dJ), sigma2=st.sigma2, parts=True)
    assert min(np.count_nonzero(dm), np.count_nonzero(p["P"])) >= -(-B // 4) and np.array_equal(dm, rm) and np.array_equal(dg, rg)  # P > 0 and yet no trace of it
    xp, fp, _ = eng.polish_path_feasible(Xs, *box, *ops, rho=0.0, max_evals=25)
    assert np.all(eng.point_eval_path_feasible(xp, *ops, rho=0.0, jacobian=False)[2][:, mo:] > lc[0] + 1.0)
    np.testing.assert_array_equal(fp, hvi_at(xp) * f_scale)
    f0 = hvi_at(np.clip(Xs, *box)) * f_scale
    assert np.all(fp >= f0) and np.any(fp > f0)  # no worse than f_scale HVI at the start, some climbed


def test_the_python_batches_on_the_device():
    X, Y, _, Xs = TC.problem(300, 3, 40, M52, 3, seed=9)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    model.set_state(np.r_[0.6, 0.6, 0.6], X, Y)
    hi = np.median(Y, axis=0)
    one = bogp.Constrained(model=model, fun="EI", lo=[-np.inf, -np.inf], hi=hi[1:])
    two = bogp.ConstrainedEHVI(model=model, ref_point=np.quantile(Y[:, :2], 0.3, axis=0), lo=[-np.inf], hi=hi[2:])
    box = lambda: optim.Box([(-2.2, 2.2)] * 3, random_seed=3)  # noqa: E731
    for fn, crit, q in ((bogp.constrained_thompson_batch, one, 5), (bogp.constrained_ehvi_thompson_batch, two, 5)):
        kw = dict(q=q, n_features=64, seed=4, Xs=Xs)
        plain = fn(crit, box(), 300, **kw)
        xs, fs = fn(crit, box(), 300, polish=True, n_starts=4, max_iter=30, **kw)
        pts = np.array(xs)
        assert len(pts) == q and np.all(np.abs(pts) <= 2.2) and np.all(np.isfinite(fs)) and not any(np.all(np.isclose(pts[i], pts[j])) for i in range(q) for j in range(i))
        assert any(x not in plain[0] for x in xs)  # some member took a polished point
    model.engine.close()


def _abi(e, entry, mo=1, nc=2, q=2, L=16, B_=2, C_=0, member=None, null=(), bad=None, lo=-1.0, max_evals=5, upper=np.inf, rho=1.0, plo=-1.0, phi=1.0):
    lib = _lib.load()
    d, N, Bn, Ln, qm = max(e.d, 1), max(e.N, 1), max(B_, 1), max(L, 1), max(q, 1) * max(mo + nc, 1)
    a = dict(X=np.zeros((Bn, d)), omega=np.ones((Ln, d)), phase=np.zeros(Ln), weights=np.ones((Ln, qm)), coef=np.zeros((N, qm)),
             lower=np.zeros((max(C_, 1), max(mo, 1))), upper=np.full((max(C_, 1), max(mo, 1)), upper), lo=np.full(d, lo), hi=np.ones(d),
             out=np.empty((Bn, d)), val=np.empty(Bn), plo=np.full(max(nc, 1), plo), phi=np.full(max(nc, 1), phi))  # fmt: skip
    mem, ne = np.zeros(Bn, dtype=np.int32) if member is None else np.asarray(member, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
    if bad is not None:
        a[bad].flat[-1] = np.inf
    cells = () if mo < 2 and C_ == 0 else ("lower", "upper")
    p = {k: None if k in null or (k in ("lower", "upper") and k not in cells) else _lib._ptr(v) for k, v in a.items()}
    draw = (mo, q, L, p["omega"], p["phase"], p["weights"], p["coef"], C_, p["lower"], p["upper"], nc, p["plo"], p["phi"], 1, rho)
    pm = None if "member" in null else mem.ctypes.data_as(_lib._ip)
    if entry == "eval":
        rc = lib.bogp_point_eval_path_feasible(e._h, p["X"], B_, pm, *draw, p["val"], p["out"], None, None)
    else:
        rc = lib.bogp_polish_path_feasible(e._h, p["X"], B_, pm, p["lo"], p["hi"], *draw, max_evals, 1e-8, 1e6, p["out"], p["val"], ne.ctypes.data_as(_lib._ip))
    return rc, lib.bogp_last_error(e._h).decode()


EHVI = dict(mo=2, nc=1, C_=1)  # the committed model has three targets
CODES = [("ok", {}, _lib.OK, ""), ("ok", EHVI, _lib.OK, ""), ("ok", dict(mo=0, nc=3), INVALID, "at least one of each"),
         ("ok", dict(mo=3, nc=0), INVALID, "at least one of each"), ("ok", dict(null=("plo",)), INVALID, "plo and phi"),
         ("ok", dict(rho=-1.0), INVALID, "rho = -1"), ("ok", dict(rho=np.nan), INVALID, "rho = nan"), ("ok", dict(rho=np.inf), INVALID, "rho = inf"),
         ("ok", dict(plo=np.nan), INVALID, "is NaN"), ("ok", dict(plo=2.0), INVALID, "below its lower bound"),
         ("ok", dict(C_=1), INVALID, "one objective has no cells"), ("forest", {}, UNSUPPORTED, "forest"),
         ("uncommitted", {}, INVALID, "no committed model"), ("lift", {}, UNSUPPORTED, "lift"), ("one target", {}, INVALID, "one target"),
         ("ok", dict(nc=3), INVALID, "m = 4 but"), ("ok", dict(q=0), INVALID, "q = 0 members"), ("ok", dict(q=6), INVALID, "q = 6 members"),
         ("ok", dict(L=24), INVALID, "L = 24"), ("ok", dict(B_=0), INVALID, "B = 0 outside"), ("ok", dict(B_=4097), INVALID, "B = 4097 outside"),
         ("ok", dict(null=("member",)), INVALID, "non-null"), ("ok", dict(null=("coef",)), INVALID, "non-null"),
         ("ok", dict(member=[0, 2]), INVALID, "member[1] = 2 outside"), ("ok", dict(EHVI, C_=0), INVALID, "C = 0 cells"),
         ("ok", dict(EHVI, null=("lower",)), INVALID, "non-null"), ("ok", dict(EHVI, bad="lower"), INVALID, "not finite"),
         ("ok", dict(EHVI, upper=-1.0), INVALID, "below its lower bound"), ("ok", dict(bad="omega"), INVALID, "omega has a non-finite entry"),
         ("ok", dict(bad="phase"), INVALID, "phase has a non-finite entry"), ("ok", dict(bad="weights"), INVALID, "weights has a non-finite entry"),
         ("ok", dict(bad="coef"), INVALID, "coef has a non-finite entry"), ("noisy", {}, UNSUPPORTED, "noisy mode"),
         ("noise-estimating", {}, UNSUPPORTED, "noise-estimating mode"), ("cubic", {}, UNSUPPORTED, "cubic"),
         ("generalized-exponential", {}, UNSUPPORTED, "generalized-exponential"),
         ("general-nu", {}, UNSUPPORTED, "general-nu Matern kernel has no input-derivative"),
         ("ok", dict(null=("X",)), INVALID, "null"),  # then the polish's own: the evaluation does not take them
         ("ok", dict(lo=2.0), INVALID, "lo[0] > hi[0]"), ("ok", dict(max_evals=0), INVALID, "max_evals"), ("ok", dict(null=("out",)), INVALID, "null")]  # fmt: skip


@pytest.mark.parametrize("entry", ["eval", "polish"])
@pytest.mark.parametrize("state,kw,code,words", CODES, ids=["%d-%s" % (i, c[0]) + "".join("-%s=%s" % kv for kv in c[1].items()) for i, c in enumerate(CODES)])
def test_return_codes(eng, entry, state, kw, code, words):  # noqa: F811
    """The union of `bogp_point_eval_path_hvi`'s and `bogp_sweep_thompson_ehvi_constrained`'s returns and the entries' own, but three:
    more than one rank cannot be built on one device, no model of d > BOGP_MAX_DIM commits, and a multi-target model commits with the
    constant trend only.  The committed model has three targets (one target under "one target")."""
    if entry == "eval" and (set(kw) & {"lo", "max_evals"} or kw.get("null") == ("out",)):
        code, words = _lib.OK, ""
    e = _lib.Engine(0) if state == "forest" else eng  # (a forest takes a handle of its own)
    X, Y, theta, _ = TC.problem(10, 3, 67, SE, 3)
    try:
        if state == "forest":
            e.forest_set(3, [0, 1, 2], [-2, -2], [-2.0, -2.0], [-1, -1], [-1, -1], [0.0, 1.0])
        else:
            e.set_train(X, Y[:, 0] if state == "one target" else Y)
        if state not in ("forest", "uncommitted"):
            kernel, mode, tail, nug = STATES[state]
            e.commit(kernel, mode, np.r_[np.full(3, 2.0) if state == "cubic" else theta, tail], nug, state == "one target", 0.0 if state == "one target" else 0.3)
        if state == "lift":
            e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))
        rc, msg = _abi(e, entry, **kw)
        assert rc == code and words in msg, (rc, msg)
    finally:
        e.clear_lift() if state == "lift" else None
        e.close() if state == "forest" else None
