"""The Thompson polish on the device: `bogp_point_eval_path` (kernels_point_path.hip) against the dense restatement
`thompson.path_grad_numpy` on the SAME draw and against `bogp_sweep_thompson` on the same rows; bit-identity across B, position and
neighbours; `bogp_polish_path`; every return code.  Tolerance (ledger T31, T16's form): |dev - ref| <= ptol (|ref| + A), ptol =
max(1e-6, 100 cond(R) eps), A the sum of the ABSOLUTE terms -- for the value as `test_gpu_thompson.restate` builds it (which asserts
cond(R) <= 1e8 and phases <= 1e6), for gradient component k  sum_n |c_n| |d r_n / d x_k| + sum_l |Wt_l| |omega_lk|.  Asserted per
configuration: the conditioning and the feature term each reach 1e-2 of A somewhere, so a missing term cannot pass.  Measured on an
MI355X (profiles/thompson_polish.txt): gradient <= 8.1e-9 of the allowance, value <= 4.9e-9, against the sweep <= 4.4e-9.
N = 1025 is one row above the kernel's n-tile, L = 1040 one step above its l-tile, d = 64 / 65 the two sides of its k-pass."""
import numpy as np
import pytest

import test_gpu_thompson as TT
from bogp import _lib, thompson
from test_gpu_thompson import eng  # noqa: F401  (its module-scoped engine fixture)

pytestmark = pytest.mark.gpu

KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP]
BS, NS, DS, LS, QS = [1, 2, 17, 33], [5, 64, 67, 257, 1025], [1, 4, 5, 20, 33, 65, 64], [16, 48, 1024, 1040], [1, 3, 16]
# 24 configurations: every value of every list, in changing company; cfg 7 is the prior path
CONFIGS = [(BS[i % 4], NS[i % 5], DS[(i + i // 5) % 7], LS[(i // 2 + 2) % 4], QS[(i // 3) % 3], KERNELS[(i + i // 6) % 5], bool((i // 4) % 2),
            bool((i + i // 8) % 2)) for i in range(24)]  # fmt: skip
PRIOR = 7  # this configuration evaluates the prior path (coef=None)


@pytest.mark.parametrize("cfg", range(24))
def test_value_and_gradient_against_the_restatement_and_the_sweep(eng, cfg):
    B, N, d, L, q, kernel, est, minimize = CONFIGS[cfg]
    X, y, theta, rows = TT.problem(B, d, N, kernel)  # rows 0.01 off training rows first
    if cfg % 2 == 0:
        rows[B - 1] = X[min(3, N - 1)]  # ... and one ON a training row (D = 0)
    members = (np.arange(B)[::-1] * 7 + cfg) % q  # repeated and out of order
    st = TT.commit(eng, X, y, theta, kernel, est)
    dr, conditioned = thompson.draw(st, q, L, seed=cfg), cfg != PRIOR
    ref, b = TT.restate(st, dr, rows, conditioned), np.arange(B)  # (asserts cond(R) and the phases)
    val, grad, parts = thompson.path_grad_numpy(st, dr, rows, members, conditioned=conditioned, parts=True)
    np.testing.assert_allclose(val, ref["paths"][members, b], rtol=1e-9, atol=1e-12)
    share = {t: max(np.max(parts[t + "_v"] / parts["A_v"]), np.max(parts[t + "_g"] / parts["A_g"])) for t in ("cond", "feat")}
    assert share["feat"] >= 1e-2 and (share["cond"] >= 1e-2 or not conditioned), share
    tol_v, tol_g, ptol = ref["tol"][members, b], ref["ptol"] * (np.abs(grad) + parts["A_g"]), ref["ptol"]
    eng.upload_candidates(rows)
    sweep = eng.sweep_thompson(dr, minimize=minimize, k=1, conditioned=conditioned, return_values=True)
    dv, dg = eng.point_eval_path(rows, dr, sweep["coef"] if conditioned else None, members, minimize=minimize)
    e_v, e_g = float(np.max(np.abs(dv - val) / tol_v)), float(np.max(np.abs(dg - grad) / tol_g))
    e_s = float(np.max(np.abs(dv - sweep["paths"][members, b]) / tol_v))  # the sweep's value on the same rows
    print("cfg %2d B %2d N %4d d %2d L %4d q %2d kernel %d est %d min %d ptol %.1e: excess value %.3g grad %.3g sweep %.3g"
          % (cfg, B, N, d, L, q, kernel, est, minimize, ptol, e_v, e_g, e_s))  # fmt: skip
    assert e_v <= 1.0 and e_g <= 1.0 and e_s <= 1.0, (e_v, e_g, e_s)


@pytest.mark.parametrize("N,d,L,q,kernel,est,minimize", [(1025, 20, 1040, 3, _lib.KERNEL_MATERN52, True, True),
                                                         (67, 65, 48, 16, _lib.KERNEL_MATERN32, False, False)])  # fmt: skip
def test_a_points_record_does_not_depend_on_its_company(eng, N, d, L, q, kernel, est, minimize):
    X, y, theta, rows = TT.problem(33, d, N, kernel)
    dr = thompson.draw(TT.commit(eng, X, y, theta, kernel, est), q, L, seed=N)
    eng.upload_candidates(rows)
    coef = eng.sweep_thompson(dr)["coef"]
    members = np.arange(33) % q
    full = eng.point_eval_path(rows, dr, coef, members, minimize=minimize)
    order = np.random.default_rng(N).permutation(33)  # another position, beside other members
    beside = (members[order] + 1) % q
    beside[0] = members[order[0]]
    moved = eng.point_eval_path(rows[order], dr, coef, beside, minimize=minimize)
    for b, got in [(b, eng.point_eval_path(rows[b], dr, coef, [members[b]], minimize=minimize)) for b in (0, 5, 32)] + [(order[0], moved)]:
        np.testing.assert_array_equal(got[0][0], full[0][b])  # B = 1 against B = 33; moved
        np.testing.assert_array_equal(got[1][0], full[1][b])


@pytest.mark.parametrize("N,d,kernel,est,minimize", [(67, 3, _lib.KERNEL_MATERN52, True, True), (300, 20, _lib.KERNEL_SE, False, False),
                                                     (67, 20, _lib.KERNEL_MATERN32, True, False)])  # fmt: skip
def test_polish(eng, N, d, kernel, est, minimize):
    q, B, lo, hi, max_evals = 4, 32, -2.0, 2.2, 25
    X, y, theta, rows = TT.problem(B, d, N, kernel, seed=2)  # rows in [-2.2, 2.2]: some starts lie outside the box and are clipped
    rows[5, 0], rows[6, :] = lo, hi  # starts on a bound, and in a corner
    dr = thompson.draw(TT.commit(eng, X, y, theta, kernel, est), q, 48, seed=N + d)
    eng.upload_candidates(rows)
    coef = eng.sweep_thompson(dr)["coef"]
    members, box = np.repeat(np.arange(q), B // q), (np.full(d, lo), np.full(d, hi))
    xp, fp, ne = eng.polish_path(rows, *box, dr, coef, members, minimize=minimize, max_evals=max_evals)
    assert np.all(xp >= lo) and np.all(xp <= hi) and np.all(ne >= 1) and np.all(ne <= max_evals)
    f0 = eng.point_eval_path(np.clip(rows, lo, hi), dr, coef, members, minimize=minimize)[0]
    assert (np.all(fp <= f0) if minimize else np.all(fp >= f0)) and np.any(fp != f0)  # no start got worse, some moved
    np.testing.assert_array_equal(fp, eng.point_eval_path(xp, dr, coef, members, minimize=minimize)[0])
    again = eng.polish_path(rows, *box, dr, coef, members, minimize=minimize, max_evals=max_evals)
    for a, b in zip((xp, fp, ne), again):
        np.testing.assert_array_equal(a, b)


def _abi(e, entry, q=2, L=16, B=2, member=None, null=(), bad=None, coef=True, lo=-1.0, max_evals=5):
    lib = _lib.load()
    d, N, Bn, Ln, qn = max(e.d, 1), max(e.N, 1), max(B, 1), max(L, 1), max(q, 1)
    a = dict(X=np.zeros((Bn, d)), omega=np.ones((Ln, d)), phase=np.zeros(Ln), weights=np.ones((Ln, qn)), coef=np.zeros((N + 1, qn)),
             lo=np.full(d, lo), hi=np.ones(d), out=np.empty((Bn, d)), val=np.empty(Bn))  # fmt: skip
    mem, ne = np.zeros(Bn, dtype=np.int32) if member is None else np.asarray(member, dtype=np.int32), np.zeros(Bn, dtype=np.int32)
    if bad is not None:
        a[bad].flat[-1] = np.inf
    p = {k: None if k in null or (k == "coef" and not coef) else _lib._ptr(v) for k, v in a.items()}
    pm = None if "member" in null else mem.ctypes.data_as(_lib._ip)
    if entry == "eval":
        rc = lib.bogp_point_eval_path(e._h, p["X"], B, pm, q, L, p["omega"], p["phase"], p["weights"], p["coef"], 1, p["val"], p["out"])
    else:
        rc = lib.bogp_polish_path(e._h, p["X"], B, pm, p["lo"], p["hi"], q, L, p["omega"], p["phase"], p["weights"], p["coef"], 1, max_evals,
                                  1e-8, 1e6, p["out"], p["val"], ne.ctypes.data_as(_lib._ip))  # fmt: skip
    return rc, lib.bogp_last_error(e._h).decode()


SE, NL = _lib.KERNEL_SE, _lib.MODE_NOISELESS  # a state below: (kernel, mode, what follows theta in the parameters, nugget, commit keywords)
STATES = {"ok": (SE, NL, [], 0.0, {}), "two targets": (SE, NL, [], 0.0, {}), "lift": (SE, NL, [], 0.0, {}), "noisy": (SE, _lib.MODE_NOISY, [0.7], 1e-6, {}),
          "noise-estimating": (SE, _lib.MODE_NOISE_ESTIM, [0.9], 0.0, {}), "cubic": (_lib.KERNEL_CUBIC, NL, [], 0.0, {}),
          "generalized-exponential": (_lib.KERNEL_GENEXP, NL, [1.5], 0.0, {}), "general-nu": (_lib.KERNEL_MATERN_NU, NL, [0.8], 0.0, {}),
          "linear trend": (SE, NL, [], 0.0, dict(trend=_lib.TREND_LINEAR))}  # fmt: skip


def _state(e, name):
    X, y, theta, _ = TT.problem(100, 3, 67, SE)
    if name == "forest":
        return e.forest_set(3, [0, 1, 2], [-2, -2], [-2.0, -2.0], [-1, -1], [-1, -1], [0.0, 1.0])
    e.set_train(X, np.column_stack([y, 2 * y + 1]) if name == "two targets" else y)
    if name != "uncommitted":
        kernel, mode, tail, nug, kw = STATES[name]
        e.commit(kernel, mode, np.r_[np.full(3, 2.0) if name == "cubic" else theta, tail], nug, name != "two targets", 0.0, **kw)
    if name == "lift":
        e.set_lift(np.eye(3), np.zeros(3), None, -np.ones(3), np.ones(3))


INVALID, UNSUPPORTED = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
CODES = [("ok", {}, _lib.OK, ""), ("ok", dict(coef=False), _lib.OK, ""), ("forest", {}, UNSUPPORTED, "forest"),
         ("uncommitted", {}, INVALID, "no committed model"), ("ok", dict(q=0), INVALID, "q = 0 outside"), ("ok", dict(q=17), INVALID, "q = 17 outside"),
         ("ok", dict(L=24), INVALID, "L = 24"), ("ok", dict(B=0), INVALID, "B = 0 outside"), ("ok", dict(B=4097), INVALID, "B = 4097 outside"),
         ("ok", dict(null=("member",)), INVALID, "non-null"), ("ok", dict(member=[0, 2]), INVALID, "member[1] = 2 outside"),
         ("ok", dict(bad="omega"), INVALID, "omega has a non-finite entry"), ("ok", dict(bad="phase"), INVALID, "phase has a non-finite entry"),
         ("ok", dict(bad="weights"), INVALID, "weights has a non-finite entry"), ("ok", dict(bad="coef"), INVALID, "coef has a non-finite entry"),
         ("noisy", {}, UNSUPPORTED, "noisy mode"), ("noise-estimating", {}, UNSUPPORTED, "noise-estimating mode"),
         ("linear trend", {}, UNSUPPORTED, "constant trend"), ("two targets", {}, UNSUPPORTED, "one target"),
         ("cubic", {}, UNSUPPORTED, "cubic kernel has no input-derivative"), ("generalized-exponential", {}, UNSUPPORTED, "generalized-exponential kernel"),
         ("general-nu", {}, UNSUPPORTED, "general-nu Matern kernel has no input-derivative"), ("lift", {}, UNSUPPORTED, "lift"),
         ("ok", dict(null=("X",)), INVALID, "null"),  # then the polish's own: the evaluation does not take them, and its grad_out may be null
         ("ok", dict(lo=2.0), INVALID, "lo[0] > hi[0]"), ("ok", dict(max_evals=0), INVALID, "max_evals"), ("ok", dict(null=("out",)), INVALID, "null")]  # fmt: skip


@pytest.mark.parametrize("entry", ["eval", "polish"])
@pytest.mark.parametrize("state,kw,code,words", CODES, ids=[c[0] + "".join("-%s=%s" % kv for kv in c[1].items()) for c in CODES])
def test_return_codes(eng, entry, state, kw, code, words):
    """All but two: more than one rank cannot be built on one device, and no model of d > BOGP_MAX_DIM = BOGP_POINT_MAX_D committed."""
    assert _lib.load().bogp_point_eval_path(None, None, 1, None, 1, 16, None, None, None, None, 1, None, None) == INVALID
    if entry == "eval" and (set(kw) & {"lo", "max_evals"} or kw.get("null") == ("out",)):
        code, words = _lib.OK, ""
    e = _lib.Engine(0) if state == "forest" else eng  # (a forest takes a handle of its own)
    try:
        _state(e, state)
        rc, msg = _abi(e, entry, **kw)
        assert rc == code and words in msg, (rc, msg)
    finally:
        e.clear_lift() if state == "lift" else None
        e.close() if state == "forest" else None
