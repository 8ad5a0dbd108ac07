"""The polish of multi-objective Thompson batches on the device: `bogp_point_eval_path_hvi` (kernels_point_path_hvi.hip) against the dense
restatement `thompson.hvi_grad_numpy` on the SAME draw, against `bogp_sweep_thompson_ehvi` on the same rows, byte for byte against the
scalarisation restated on the device's own y and J; bit-identity across B, position, neighbours and outputs asked for;
`bogp_polish_path_hvi`; `bogp.ehvi_thompson_batch(polish=True)`; the error returns.
Allowances (ledger T31's form, per target): |y - ref| <= ptol (|ref| + A_v), |J - ref| <= ptol (|ref| + A_g), ptol = max(1e-6, 100
cond(R) eps), A the sums of the absolute terms.  Through the multilinear form: HVI sum_k |w_k| allow_y[k]; gradient component k'
sum_t |w_t| allow_J[t, k'] + sum_t |J[t, k']| sum_{i != t} H[t, i] allow_y[i], H[t, i] = sum_c [in_t][in_i] prod_{j != t, i} t_j =
|d w_t / d y_i|.  Condition, asserted per row on the restatement alone: every y_k is farther from every cell face than 1e3 times its
allowance, so the device's y lies in the same cells.  The cells are boxes over up to 3 faces per objective, placed in the middle of the
widest gaps between the restated values (any boxes are valid input: the kernel sums over them as given), the models of TC.problem
with a shorter length scale (SHORT): the allowance grows with sum_n |r_n c_n|, and a long one leaves no gap 2e3 allowances wide.
Measured on an MI355X (ledger T32): y <= 9.7e-10 of the allowance, J <= 3.2e-9, HVI <= 3.7e-10, gradient <= 6.6e-10, sweep <= 8.9e-10."""
import numpy as np
import pytest

import thompson_constrained_cases as TC
from bogp import _lib, thompson
from test_gpu_thompson_constrained import commit
from test_gpu_thompson_ehvi import eng  # noqa: F401  (its module-scoped engine fixture)

pytestmark = pytest.mark.gpu
SE, M12, M32, M52, AE = _lib.KERNEL_SE, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP
B = 40  # points a row: the candidates of its sweep
# (N, d, L, m, q, C, kernel): N = 1024 / 1025 the row tile of m <= 4, 512 / 513 that of m > 4; d = 64 / 65 the k-pass; L = 1040 one step above
# the feature tile; C = 255 / 257 the two sides of one cell a thread
ROWS = [(1, 1, 16, 2, 8, 1, SE), (1, 2, 16, 3, 5, 255, M52), (255, 2, 16, 2, 8, 257, M52), (255, 63, 1040, 3, 5, 1, SE),
        (255, 64, 16, 8, 2, 255, M52), (255, 65, 16, 2, 8, 257, SE), (255, 63, 16, 3, 5, 257, M52), (1024, 20, 1040, 2, 8, 255, SE),
        (1025, 20, 16, 2, 8, 1, M52), (1025, 5, 16, 3, 5, 255, SE), (1025, 20, 1040, 3, 5, 257, M52), (1024, 5, 16, 2, 8, 257, SE),
        (512, 20, 16, 8, 2, 257, SE), (513, 20, 1040, 8, 2, 1, M52), (513, 65, 16, 8, 2, 255, SE), (512, 63, 16, 8, 2, 257, M52),
        (1, 1, 1040, 8, 2, 257, SE), (255, 2, 16, 4, 4, 255, M52), (300, 5, 48, 5, 3, 257, SE), (255, 20, 16, 2, 8, 255, M12),
        (255, 5, 16, 3, 5, 257, M32), (255, 20, 48, 3, 5, 255, AE), (67, 33, 1040, 4, 4, 1, M52), (1025, 33, 48, 4, 4, 257, SE)]  # fmt: skip
SHORT = {SE: 10.0, M32: 40.0, M52: 40.0}  # theta of TC.problem times this: a short length scale keeps sum_n |r_n c_n|, and so the allowance, small


def problem(row):
    N, d, L, m, q, C, kernel = row
    X, Y, theta, Xs = TC.problem(B, d, N, kernel, m)
    return X, Y, theta * SHORT.get(kernel, 1.0), Xs


def cells_of(y, al, C):
    """C boxes over the reference point min y - 1: per objective up to 3 faces, each the middle of one of the widest gaps of y's column
    and farther than 1.2e3 allowances from EVERY value (a missing face falls on the reference point: an empty interval), and +inf; the
    first three objectives walk their 4 intervals with the cell index, the others keep [reference, +inf)."""
    m = y.shape[1]
    edges = []
    for k in range(m):
        v = np.sort(y[:, k])
        mids = [(v[i] + v[i + 1]) / 2 for i in np.argsort(np.diff(v))[::-1]]
        f = [f for f in mids if np.all(np.abs(y[:, k] - f) > 1.2e3 * al[:, k])][:3]
        assert f or len(v) < 2, "objective %d: no face stands clear of the values" % k
        edges.append(np.r_[[v[0] - 1.0] * (4 - len(f)), np.sort(f), np.inf])
    lower, upper = np.empty((C, m)), np.empty((C, m))
    for c in range(C):
        for k in range(m):
            i = (c * 7 // 4**k) % 4 if k < 3 and C > 1 else None
            lower[c, k], upper[c, k] = (edges[k][0], np.inf) if i is None else (edges[k][i], edges[k][i + 1])
    return lower, upper, np.array([e[1:4] for e in edges])


def setup(eng, row, seed):  # noqa: F811
    N, d, L, m, q, C, kernel = row
    X, Y, theta, Xs = problem(row)
    st = commit(eng, X, Y, theta, kernel)
    dr = thompson.draw_multi(st, q, L, seed=seed)
    members = (np.arange(B)[::-1] * 7 + seed) % q  # repeated and out of order
    eng.upload_candidates(Xs)
    sweep = eng.sweep_thompson_ehvi(dr, q, np.zeros((1, m)), np.full((1, m), np.inf), return_values=True)
    return st, dr, Xs, members, sweep


@pytest.mark.parametrize("cfg", range(len(ROWS)))
def test_values_and_gradients_against_the_restatement_and_the_sweep(eng, cfg):  # noqa: F811
    N, d, L, m, q, C, kernel = ROWS[cfg]
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)
    ref, b = TC.restate(st, dr, Xs), np.arange(B)
    assert ref.cond <= 1e8, ref.cond
    _, _, p = thompson.hvi_grad_numpy(st, dr, Xs, members, np.zeros((1, m)), np.full((1, m), np.inf), parts=True)  # y, J and their absolute sums
    al_y, al_J = ref.ptol * (np.abs(p["y"]) + p["A_v"]), ref.ptol * (np.abs(p["jac"]) + p["A_g"])
    lower, upper, faces = cells_of(p["y"], al_y, C)
    hvi, grad, p["w"] = thompson.hvi_scalarise_numpy(p["y"], p["jac"], lower, upper)
    assert np.min(np.abs(p["y"][:, :, None] - faces[None]) / al_y[:, :, None]) > 1e3  # the condition: no value near a face
    assert np.count_nonzero(hvi) >= B // 4 and np.count_nonzero(p["w"]) >= B // 4  # the criterion and its weights are alive
    t = np.fmax(np.fmin(p["y"][:, None], upper[None]) - lower[None], 0.0)  # (B, C, m)
    ins = (lower[None] < p["y"][:, None]) & (p["y"][:, None] < upper[None])
    H = np.zeros((B, m, m))
    for k in range(m):
        for i in range(m):
            if i != k:
                H[:, k, i] = ((ins[:, :, k] & ins[:, :, i]) * np.prod(np.delete(t, [k, i], axis=2), axis=2)).sum(axis=1)
    tol_h = np.einsum("bk,bk->b", np.abs(p["w"]), al_y)
    tol_g = np.einsum("bt,btk->bk", np.abs(p["w"]), al_J) + np.einsum("btk,bti,bi->bk", np.abs(p["jac"]), H, al_y)
    dh, dg, dy, dJ = eng.point_eval_path_hvi(Xs, dr, sweep["coef"], members, lower, upper)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_y, e_J = float(np.max(np.abs(dy - p["y"]) / al_y)), float(np.max(np.abs(dJ - p["jac"]) / al_J))
        e_h = float(np.nanmax(np.where(tol_h > 0, np.abs(dh - hvi) / tol_h, np.where(dh == hvi, 0.0, np.inf))))
        e_g = float(np.nanmax(np.where(tol_g > 0, np.abs(dg - grad) / tol_g, np.where(dg == grad, 0.0, np.inf))))
    e_s = float(np.max(np.abs(dy - sweep["paths"][members, :, b]) / ref.tol[members, :, b]))  # the sweep's paths on the same rows (T30)
    print("cfg %2d %s ptol %.1e: ratio to the allowance y %.3g J %.3g hvi %.3g grad %.3g sweep %.3g" % (cfg, ROWS[cfg], ref.ptol, e_y, e_J, e_h, e_g, e_s))
    assert max(e_y, e_J, e_h, e_g, e_s) <= 1.0, (e_y, e_J, e_h, e_g, e_s)
    rh, rg = thompson.hvi_grad_numpy(None, None, None, None, lower, upper, from_device=(dy, dJ))  # byte for byte from the device's own y, J
    np.testing.assert_array_equal(dh, rh), np.testing.assert_array_equal(dg, rg)


@pytest.mark.parametrize("cfg", [10, 14])
def test_a_points_outputs_do_not_depend_on_its_company(eng, cfg):  # noqa: F811
    q = ROWS[cfg][4]
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)
    y0 = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(B)]
    lower, upper, _ = cells_of(y0, np.zeros_like(y0), ROWS[cfg][5])
    ev = lambda X, mem, **kw: eng.point_eval_path_hvi(X, dr, sweep["coef"], mem, lower, upper, **kw)  # noqa: E731
    full = ev(Xs[:33], members[:33])
    order = np.random.default_rng(cfg).permutation(33)  # another position, beside other members
    beside = (members[order] + 1) % q
    beside[0] = members[order[0]]
    cases = [(i, ev(Xs[i], [members[i]])) for i in (0, 5, 32)] + [(order[0], ev(Xs[order], beside))]
    for i, got in cases:
        for a, f in zip(got, full):
            np.testing.assert_array_equal(a[0], f[i])
    bare = ev(Xs[:33], members[:33], jacobian=False)  # with and without jac_out
    assert bare[3] is None and all(np.array_equal(a, f) for a, f in zip(bare[:3], full[:3]))


@pytest.mark.parametrize("cfg", [2, 11, 18])
def test_polish(eng, cfg):  # noqa: F811
    d, lo, hi, max_evals = ROWS[cfg][1], -2.0, 2.1, 25
    st, dr, Xs, members, sweep = setup(eng, ROWS[cfg], cfg)  # rows in [-2.2, 2.2]: some starts lie outside the box and are clipped
    y0 = thompson.paths_multi_numpy(st, dr, Xs)[0][members, :, np.arange(B)]
    lower = np.quantile(y0, 0.4, axis=0)[None]  # one cell above the 0.4 quantiles: a good part of the starts has HVI = 0
    upper, box = np.full_like(lower, np.inf), (np.full(d, lo), np.full(d, hi))
    ev = lambda X: eng.point_eval_path_hvi(X, dr, sweep["coef"], members, lower, upper)  # noqa: E731
    xp, fp, ne = eng.polish_path_hvi(Xs, *box, dr, sweep["coef"], members, lower, upper, max_evals=max_evals)
    f0, x0 = ev(np.clip(Xs, lo, hi))[0], np.clip(Xs, lo, hi)
    assert np.all(xp >= lo) and np.all(xp <= hi) and np.all(ne >= 1) and np.all(ne <= max_evals)
    np.testing.assert_array_equal(fp, ev(xp)[0])
    assert np.all(fp >= f0) and np.any(fp > f0)  # no start got worse, some climbed
    flat = f0 == 0.0  # HVI = 0: a zero gradient; back unchanged after one evaluation
    assert flat.any() and np.array_equal(xp[flat], x0[flat]) and np.all(ne[flat] == 1) and np.all(fp[flat] == 0.0)


def test_the_python_batch_on_the_device():
    import bogp
    from bogp import optim

    X, Y, _, Xs = TC.problem(300, 3, 40, M52, 3, seed=9)
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(3, beta=0.0), corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    model.set_state(np.r_[0.6, 0.6, 0.6], X, Y)
    crit = bogp.EHVI(model=model, ref_point=np.quantile(Y, 0.3, axis=0), Y=Y)
    box = lambda: optim.Box([(-2.2, 2.2)] * 3, random_seed=3)  # noqa: E731
    kw = dict(q=7, n_features=64, seed=4, Xs=Xs)
    plain = bogp.ehvi_thompson_batch(crit, box(), 300, **kw)
    assert bogp.ehvi_thompson_batch(crit, box(), 300, polish=False, **kw) == plain
    first, f1 = bogp.ehvi_thompson_batch(crit, box(), 300, polish=True, n_starts=4, max_iter=30, **kw)
    hist = np.array(first[:2])
    xs, fs = bogp.ehvi_thompson_batch(crit, box(), 300, polish=True, n_starts=4, max_iter=30, history=hist, **kw)
    for pts in (np.array(first), np.array(xs)):
        assert len(pts) == 7 and np.all(np.abs(pts) <= 2.2)
        assert not any(np.all(np.isclose(pts[i], pts[j])) for i in range(7) for j in range(i))
    assert not any(np.any(np.all(np.isclose(hist, x), axis=1)) for x in xs)
    assert all(a >= b for a, b in zip(f1, plain[1]) if b > 0) and any(a > b for a, b in zip(f1, plain[1]))  # polished: no worse than the row
    model.engine.close()


def _abi(e, entry, m=2, q=2, L=16, B_=2, C_=1, member=None, null=(), bad=None, lo=-1.0, max_evals=5, upper=np.inf):
    lib = _lib.load()
    d, N, Bn, Ln, qm = max(e.d, 1), max(e.N, 1), max(B_, 1), max(L, 1), max(q, 1) * max(m, 1)
    a = dict(X=np.zeros((Bn, d)), omega=np.ones((Ln, d)), phase=np.zeros(Ln), weights=np.ones((Ln, qm)), coef=np.zeros((N, qm)),
             lower=np.zeros((max(C_, 1), max(m, 1))), upper=np.full((max(C_, 1), max(m, 1)), upper), lo=np.full(d, lo), hi=np.ones(d),
             out=np.empty((Bn, d)), val=np.empty(Bn))  # fmt: skip
    mem, ne = np.zeros(Bn, dtype=np.int32) if member is None else np.asarray(member, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
    if bad is not None:
        a[bad].flat[-1] = np.inf
    p = {k: None if k in null else _lib._ptr(v) for k, v in a.items()}
    draw = (m, q, L, p["omega"], p["phase"], p["weights"], p["coef"], C_, p["lower"], p["upper"])
    pm = None if "member" in null else mem.ctypes.data_as(_lib._ip)
    if entry == "eval":
        rc = lib.bogp_point_eval_path_hvi(e._h, p["X"], B_, pm, *draw, p["val"], p["out"], None, None)
    else:
        rc = lib.bogp_polish_path_hvi(e._h, p["X"], B_, pm, p["lo"], p["hi"], *draw, max_evals, 1e-8, 1e6, p["out"], p["val"], ne.ctypes.data_as(_lib._ip))
    return rc, lib.bogp_last_error(e._h).decode()


NL, INVALID, UNSUPPORTED = _lib.MODE_NOISELESS, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
STATES = {"ok": (SE, NL, [], 0.0), "lift": (SE, NL, [], 0.0), "one target": (SE, NL, [], 0.0), "noisy": (SE, _lib.MODE_NOISY, [0.7], 1e-6),
          "noise-estimating": (SE, _lib.MODE_NOISE_ESTIM, [0.9], 0.0), "cubic": (_lib.KERNEL_CUBIC, NL, [], 0.0),
          "generalized-exponential": (_lib.KERNEL_GENEXP, NL, [1.5], 0.0), "general-nu": (_lib.KERNEL_MATERN_NU, NL, [0.8], 0.0)}  # fmt: skip
CODES = [("ok", {}, _lib.OK, ""), ("forest", {}, UNSUPPORTED, "forest"), ("uncommitted", {}, INVALID, "no committed model"),
         ("lift", {}, UNSUPPORTED, "lift"), ("one target", {}, INVALID, "one target"), ("ok", dict(m=3), INVALID, "m = 3 but"),
         ("ok", dict(q=0), INVALID, "q = 0 members"), ("ok", dict(q=9), INVALID, "q = 9 members"), ("ok", dict(L=24), INVALID, "L = 24"),
         ("ok", dict(B_=0), INVALID, "B = 0 outside"), ("ok", dict(B_=4097), INVALID, "B = 4097 outside"), ("ok", dict(null=("member",)), INVALID, "non-null"),
         ("ok", dict(null=("coef",)), INVALID, "non-null"), ("ok", dict(member=[0, 2]), INVALID, "member[1] = 2 outside"),
         ("ok", dict(C_=0), INVALID, "C = 0 cells"), ("ok", dict(null=("lower",)), INVALID, "non-null"), ("ok", dict(bad="lower"), INVALID, "not finite"),
         ("ok", dict(upper=-1.0), INVALID, "below its lower bound"), ("ok", dict(bad="omega"), INVALID, "omega has a non-finite entry"),
         ("ok", dict(bad="phase"), INVALID, "phase has a non-finite entry"), ("ok", dict(bad="weights"), INVALID, "weights has a non-finite entry"),
         ("ok", dict(bad="coef"), INVALID, "coef has a non-finite entry"), ("noisy", {}, UNSUPPORTED, "noisy mode"),
         ("noise-estimating", {}, UNSUPPORTED, "noise-estimating mode"), ("cubic", {}, UNSUPPORTED, "cubic"),
         ("generalized-exponential", {}, UNSUPPORTED, "generalized-exponential"), ("general-nu", {}, UNSUPPORTED, "general-nu Matern kernel has no input-derivative"),
         ("ok", dict(null=("X",)), INVALID, "null"),  # then the polish's own: the evaluation does not take them
         ("ok", dict(lo=2.0), INVALID, "lo[0] > hi[0]"), ("ok", dict(max_evals=0), INVALID, "max_evals"), ("ok", dict(null=("out",)), INVALID, "null")]  # fmt: skip


@pytest.mark.parametrize("entry", ["eval", "polish"])
@pytest.mark.parametrize("state,kw,code,words", CODES, ids=[c[0] + "".join("-%s=%s" % kv for kv in c[1].items()) for c in CODES])
def test_return_codes(eng, entry, state, kw, code, words):  # noqa: F811
    """All but three: more than one rank cannot be built on one device, no model of d > BOGP_MAX_DIM = BOGP_POINT_MAX_D commits, and a
    multi-target model commits with the constant trend only."""
    if entry == "eval" and (set(kw) & {"lo", "max_evals"} or kw.get("null") == ("out",)):
        code, words = _lib.OK, ""
    e = _lib.Engine(0) if state == "forest" else eng  # (a forest takes a handle of its own)
    X, Y, theta, _ = TC.problem(10, 3, 67, SE, 2)
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
