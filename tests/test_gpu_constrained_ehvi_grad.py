"""Feasibility-weighted EHVI and its input gradient at B points on the device (`bogp_point_eval_ehvi_constrained`,
`bogp_polish_ehvi_constrained`; kernels_point_ehvi_constrained.hip) against the NumPy restatement of
tests/support/constrained_ehvi_grad_ref.py over the 27 shared configurations (tests/constrained_ehvi_grad_cases.py, whose conditions the
CPU twin asserts), the byte identities the ABI states (the moments and P of `bogp_point_eval_constrained`, independence of B and of the
launch, every bound infinite, no cells), `bogp_sweep_ehvi_constrained` on the same rows, the exact +0.0 of lo == hi, the polish's
guarantees, `ConstrainedEHVI(input_gradient=True)` under `optim.argmax_restart` on the real engine, the error returns and the cells'
cache.  Every call takes at most 33 points against N <= 157.

Tolerances (README ledger): values, P and E at T25 / T19's form, rtol 1e-6 beside 1e-12 max|ref| of the batch; gradients at T14's
(`_excess` <= 1); mu / MSE at T1 / T2.  Measured on an MI355X over the 27 configurations: ledger line T26."""
import ctypes as C

import numpy as np
import pytest

import constrained_ehvi_grad_cases as K
from bogp import _lib, optim
from support import constrained_ehvi_grad_ref as R
from test_constrained_ehvi_grad_host import POLISH_CASE, reference_of
from test_gpu_constrained_grad import _excess, _tiny_forest, _tri_split

import bogp

pytestmark = pytest.mark.gpu

BOX = K.BOX
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _commit(eng, cfg, p):
    eng.set_train(p["X"], p["Y"])
    eng.commit(cfg.kernel, p["mode"], p["par"], 0.0, False, 0.0)


def _eval(eng, rows, p, B=33, lo=None, hi=None, lower=None, upper=None):
    """The ten arrays for `rows`: one B-point call, or for B = 1 one one-point call per row, stacked."""
    lo, hi = (p["lo"], p["hi"]) if lo is None else (lo, hi)
    lower, upper = (p["lower"], p["upper"]) if lower is None else (lower, upper)
    if B != 1:
        return eng.point_eval_ehvi_constrained(rows, lower, upper, lo, hi, moments=True)
    ones = [eng.point_eval_ehvi_constrained(r[None, :], lower, upper, lo, hi, moments=True) for r in rows]
    return tuple(np.concatenate([o[j] for o in ones]) for j in range(10))


def _t25(v, ref):
    """Largest |v - ref| in units of the allowance 1e-6 |ref| + 1e-12 max|ref| of the batch (T25 / T19's form): <= 1 passes."""
    v, ref = np.asarray(v, float), np.asarray(ref, float)
    assert np.all(np.isfinite(v[np.isfinite(ref)]))
    return float((np.abs(v - ref) / (1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max() + 1e-300)).max())


@pytest.mark.parametrize("cfg", K.CONFIGS, ids=K.IDS)
def test_agrees_with_the_restatement(eng, cfg):
    """Values, P and E at T25 / T19's form; the gradients of the value, of P and of E and dmu, dMSE at T14's rule; mu / MSE at T1 / T2; no
    NaN anywhere the restatement is finite.  Measured on an MI355X over the 27 configurations: ledger line T26 of the README."""
    p, st, ref = reference_of(cfg)
    _commit(eng, cfg, p)
    out = _eval(eng, p["rows"], p, cfg.B)
    assert [a.shape for a in out] == [np.shape(r) for r in ref]
    val, dval, pof, dpof, ehvi, dehvi, mu, mse, dmu, dmse = out
    tv = [_t25(val, ref[0]), _t25(pof, ref[2]), _t25(ehvi, ref[4])]
    ex = [_excess(dval, ref[1]), _excess(dpof, ref[3]), _excess(dehvi, ref[5]), _excess(dmu, ref[8]), _excess(dmse, ref[9])]
    print("T26 %s cells=%d: errors in units of the tolerance: val %.3g pof %.3g ehvi %.3g | dval %.3g dpof %.3g dehvi %.3g dmu %.3g dmse %.3g"
          % (cfg.id, len(p["lower"]), *tv, *ex))  # fmt: skip
    np.testing.assert_allclose(mu, ref[6], rtol=1e-6, atol=1e-9)  # T1
    sigma2 = np.asarray(st.sigma2, float).ravel()
    for k in range(mu.shape[1]):
        np.testing.assert_allclose(mse[:, k], ref[7][:, k], rtol=1e-6, atol=1e-12 * sigma2[k])  # T2
    assert max(tv) <= 1.0 and max(ex) <= 1.0
    dead = pof == 0.0  # the device's own dead rows: exactly +0.0 with a zero gradient, by definition
    assert np.all(ref[2][dead] < 1e-300)
    assert np.array_equal(val[dead], np.zeros(dead.sum())) and not np.any(np.signbit(val[dead])) and not np.any(dval[dead])
    assert not np.any(ehvi[dead]) and not np.any(dehvi[dead])  # the cells were not read
    # without the second block the record is the same
    if cfg.B == 33:
        v2, g2 = eng.point_eval_ehvi_constrained(p["rows"], p["lower"], p["upper"], p["lo"], p["hi"])
        assert v2.tobytes() == val.tobytes() and g2.tobytes() == dval.tobytes()
    if len(p["lower"]) == 0:  # no cells: the value is P and the gradient dP, the same bytes
        assert val.tobytes() == pof.tobytes() and dval.tobytes() == dpof.tobytes()


IDENTITY_CASES = [16, 22, 4]  # (3, 1) at N = 100, d = 23; (3, 2) at N = 157, d = 12; (2, 6) without cells at N = 37, d = 12: all B = 33


@pytest.mark.parametrize("i", IDENTITY_CASES)
def test_moments_and_P_are_the_bytes_of_the_constrained_point_call(eng, i):
    """mu, MSE, dmu, dMSE and P against bogp_point_eval_constrained on the same model with infinite bounds on columns 1 .. m - 1 and the
    same bounds on the constraint columns: the moments come from the shared header, and a factor of exactly 1.0 changes no product.  dP
    is compared at T14's rule and its bytes are reported only; so is the C == 0 value against the ACQ_NONE criterion."""
    cfg = K.CONFIGS[i]
    p, st, ref = reference_of(cfg)
    _commit(eng, cfg, p)
    out = _eval(eng, p["rows"], p, 33)
    clo, chi = np.r_[np.full(cfg.m - 1, -INF), p["lo"]], np.r_[np.full(cfg.m - 1, INF), p["hi"]]
    acq, dacq, pof, dpof, mu, mse, dmu, dmse = eng.point_eval_constrained(p["rows"], [(_lib.ACQ_NONE, 0.0)], 0.0, True, clo, chi, moments=True)
    for name, a, b in (("mu", out[6], mu), ("mse", out[7], mse), ("dmu", out[8], dmu), ("dmse", out[9], dmse), ("pof", out[2], pof)):
        assert a.tobytes() == b.tobytes(), name
    same = out[3].tobytes() == dpof.tobytes()
    print("%s: dpof against bogp_point_eval_constrained: %.3g of T14's allowance, bytes %s" % (cfg.id, _excess(out[3], dpof), "equal" if same else "differ"))
    assert _excess(out[3], dpof) <= 1.0
    if len(p["lower"]) == 0:
        print("%s: the C == 0 value against the ACQ_NONE criterion: bytes %s" % (cfg.id, "equal" if out[0].tobytes() == acq[:, 0].tobytes() else "differ"))
        assert _t25(out[0], acq[:, 0]) <= 1.0


@pytest.mark.parametrize("i", [1, 13, 22])
def test_bits(eng, i):
    """Identical inputs give identical bytes; row b of the B = 33 call equals the one-point call bit for bit where point_tri_geometry gives
    both the same row-block split (N = 37, d = 2 and N = 100, d = 12), and to the tolerances of the first test where it does not
    (N = 157, d = 12)."""
    cfg = K.CONFIGS[i]
    p, st, ref = reference_of(cfg)
    same = _tri_split(cfg.N, cfg.d, 1) == _tri_split(cfg.N, cfg.d, 33)
    assert same == (cfg.N != 157)
    _commit(eng, cfg, p)
    batch = _eval(eng, p["rows"], p, 33)
    again = _eval(eng, p["rows"], p, 33)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, again))
    for b in (0, 7, 32):
        one = _eval(eng, p["rows"][b : b + 1], p, 1)
        one2 = _eval(eng, p["rows"][b : b + 1], p, 1)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(one, one2))
        if same:
            assert all(np.ascontiguousarray(o[0]).tobytes() == np.ascontiguousarray(a[b]).tobytes() for o, a in zip(one, batch)), b
        else:
            assert max(_excess(np.asarray(o[0]), np.asarray(a[b])) for o, a in zip(one, batch)) <= 1.0


@pytest.mark.parametrize("i", [16, 10, 4])
def test_every_bound_infinite_and_no_cells(eng, i):
    """Every bound infinite: pof == 1.0, dpof == 0, val the bytes of ehvi and dval the bytes of dehvi (a product with an exact 1.0 and a sum
    with an exact 0).  No cells: val the bytes of pof, dval the bytes of dpof, ehvi and dehvi 0."""
    cfg = K.CONFIGS[i]
    p, st, ref = reference_of(cfg)
    _commit(eng, cfg, p)
    none = np.zeros((0, cfg.m))
    val, dval, pof, dpof, ehvi, dehvi = _eval(eng, p["rows"], p, 33, lower=none, upper=none)[:6]
    assert val.tobytes() == pof.tobytes() and dval.tobytes() == dpof.tobytes() and not np.any(ehvi) and not np.any(dehvi)
    assert _t25(pof, ref[2]) <= 1.0 and _excess(dpof, ref[3]) <= 1.0
    if len(p["lower"]) == 0:
        return
    val, dval, pof, dpof, ehvi, dehvi = _eval(eng, p["rows"], p, 33, lo=np.full(cfg.c, -INF), hi=np.full(cfg.c, INF))[:6]
    assert np.array_equal(pof, np.ones(33)) and np.array_equal(dpof, np.zeros((33, cfg.d)))
    assert val.tobytes() == ehvi.tobytes() and dval.tobytes() == dehvi.tobytes() and np.any(ehvi > 0) and np.all(np.isfinite(dehvi))
    want = R.batch(st, p["rows"], cfg.m, p["lower"], p["upper"], np.full(cfg.c, -INF), np.full(cfg.c, INF))
    assert _t25(ehvi, want[4]) <= 1.0 and _excess(dehvi, want[5]) <= 1.0


@pytest.mark.parametrize("i", [1, 13, 25])
def test_agrees_with_the_sweep_and_lo_equal_hi_is_plus_zero(eng, i):
    """val against bogp_sweep_ehvi_constrained's stored values on the same 33 rows at T25 (the two paths sum in different orders: no bit
    identity is claimed).  lo == hi on one constraint: every value exactly +0.0 (the sign bit too), every gradient component 0, and the
    polish returns the clipped starts with fout == 0."""
    cfg = K.CONFIGS[i]
    p, st, ref = reference_of(cfg)
    _commit(eng, cfg, p)
    rows = p["rows"]
    val, _, pof = _eval(eng, rows, p, 33)[:3]
    eng.upload_candidates(rows)
    _, _, svals, spof = eng.sweep_ehvi_constrained(p["lower"], p["upper"], p["lo"], p["hi"], return_values=True, return_pof=True)
    print("%s: against the sweep, in units of T25: val %.3g pof %.3g" % (cfg.id, _t25(val, svals), _t25(pof, spof)))
    assert _t25(val, svals) <= 1.0 and _t25(pof, spof) <= 1.0
    assert eng.point_eval_ehvi_constrained(rows, p["lower"], p["upper"], p["lo"], p["hi"])[0].tobytes() == val.tobytes()  # cells uploaded again
    lo2, hi2 = p["lo"].copy(), p["hi"].copy()
    lo2[-1] = hi2[-1] = float(np.median(p["Y"][:, -1]))
    out = _eval(eng, rows, p, 33, lo=lo2, hi=hi2)
    assert np.array_equal(out[0], np.zeros(33)) and not np.any(np.signbit(out[0]))
    assert not np.any(out[1]) and not np.any(out[2]) and not np.any(out[3]) and not np.any(out[4]) and not np.any(out[5])
    one = _eval(eng, rows[:1], p, 1, lo=lo2, hi=hi2)
    assert one[0][0] == 0.0 and not np.signbit(one[0][0]) and not np.any(one[1])
    starts = rows[:8] * 1.2  # some outside the box: clipped first
    blo, bhi = np.full(cfg.d, BOX[0]), np.full(cfg.d, BOX[1])
    xs, fs, ne = eng.polish_ehvi_constrained(starts, blo, bhi, p["lower"], p["upper"], lo2, hi2, max_evals=50)
    assert np.array_equal(xs, np.clip(starts, blo, bhi)) and np.array_equal(fs, np.zeros(8)) and not np.any(np.signbit(fs))
    assert np.all(ne >= 1) and np.all(ne <= 50)


def test_polish(eng):
    """8 starts, max_evals = 50: Xout lies in the box, fout[b] >= the device's own value at clip(X0[b]), n_evals <= max_evals, fout is
    reproduced by a point call at Xout, and sum(fout) > sum(f0) on the case for which the CPU twin asserts that every start has a
    non-zero projected gradient."""
    cfg = K.CONFIGS[POLISH_CASE]
    p, st, ref = reference_of(cfg)
    _commit(eng, cfg, p)
    blo, bhi = np.full(cfg.d, BOX[0]), np.full(cfg.d, BOX[1])
    starts = p["rows"][:8]
    assert np.all(starts >= blo) and np.all(starts <= bhi)
    f0 = eng.point_eval_ehvi_constrained(starts, p["lower"], p["upper"], p["lo"], p["hi"])[0]
    xs, fs, ne = eng.polish_ehvi_constrained(starts, blo, bhi, p["lower"], p["upper"], p["lo"], p["hi"], max_evals=50)
    assert np.all(xs >= blo) and np.all(xs <= bhi) and np.all(ne >= 1) and np.all(ne <= 50)
    assert np.all(fs >= f0)  # exact: a start never moves to a worse point
    again = eng.point_eval_ehvi_constrained(xs, p["lower"], p["upper"], p["lo"], p["hi"])[0]
    assert fs.tobytes() == again.tobytes()  # fout is the value AT Xout, bit for bit (N = 157, d = 2: one split for 8 points either way)
    print("polish: %d of 8 starts improved; sum %.6g -> %.6g, best %.6g -> %.6g" % ((fs > f0).sum(), f0.sum(), fs.sum(), f0.max(), fs.max()))
    assert fs.sum() > f0.sum()
    # starts outside the box are clipped first; max_evals = 1 returns them with their values
    wide = starts * 1.5
    clipped = np.clip(wide, blo, bhi)
    fc = eng.point_eval_ehvi_constrained(clipped, p["lower"], p["upper"], p["lo"], p["hi"])[0]
    x1, f1, n1 = eng.polish_ehvi_constrained(wide, blo, bhi, p["lower"], p["upper"], p["lo"], p["hi"], max_evals=1)
    assert np.array_equal(x1, clipped) and f1.tobytes() == fc.tobytes() and np.all(n1 == 1)
    xw, fw, _ = eng.polish_ehvi_constrained(wide, blo, bhi, p["lower"], p["upper"], p["lo"], p["hi"], max_evals=50)
    assert np.all(fw >= fc) and np.all(xw >= blo) and np.all(xw <= bhi)


def test_criterion_on_the_real_engine():
    """`ConstrainedEHVI(input_gradient=True)` under the polish hybrid against "sweep-device" with the same seed and budget: the polish
    starts from the sweep's top k, so its result is at least the sweep's winner -- exactly so against the point call's own value at the
    winner, and within 1e-6 relative of the sweep's stored value (the two paths sum in different orders, T25)."""
    rng = np.random.default_rng(9)
    X = rng.uniform(*BOX, size=(30, 2))
    Y = np.sin(X @ rng.normal(size=(2, 3))) * (1.0 + np.arange(3)) + 0.3 * rng.normal(size=(30, 3))
    model = bogp.GaussianProcess(mean=bogp.trend.constant_trend(2, beta=0.0), corr="matern", thetaL=[1e-3] * 2, thetaU=[1e2] * 2, nugget=1e-6)
    model.set_state(np.r_[10.0, 10.0, 0.9], X, Y)
    ref = Y[:, :2].min(0) - 0.1
    crit = bogp.ConstrainedEHVI(model=model, ref_point=ref, lo=[-INF], hi=[float(np.median(Y[:, 2]))], input_gradient=True)
    assert crit.n_feasible > 0 and not crit.feasibility_only
    v, g = crit(X[:1] + 0.1, return_dx=True)
    assert v.shape == (1,) and g.shape == (1, 2) and np.all(np.isfinite(g))
    v5, g5 = crit(X[:5] + 0.1, return_dx=True)
    assert v5.shape == (5, 1) and g5.shape == (5, 2) and v5[0, 0] == v[0]
    np.random.seed(4)
    xs, fs = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, optimizer="sweep-device")
    np.random.seed(4)
    xp, fp = optim.argmax_restart(crit, optim.Box([BOX] * 2, random_seed=7), eval_budget=500, n_restart=10, optimizer="sweep-device-BFGS")
    at_winner = float(crit(np.array([xs]))[0])
    print("sweep-device %.9g (point call at its winner %.9g), sweep-device-BFGS %.9g" % (fs, at_winner, fp))
    assert fs > 0 and fp >= at_winner and fp >= (1 - 1e-6) * fs and all(BOX[0] <= t <= BOX[1] for t in xp)
    with pytest.raises(NotImplementedError, match="has no polish"):
        optim.polish_topk(bogp.ConstrainedEHVI(model=model, ref_point=ref, lo=[-INF], hi=[0.0]), X[:2], np.array([BOX, BOX]))
    model.engine.close()


def test_cell_cache(eng):
    """Two cell sets alternated, a bogp_sweep_ehvi_constrained (which writes the same device buffer) in between, cells of the same (m, C)
    and other bytes, and no cells at all: every result equals that of a fresh handle, bit for bit (as tests/test_gpu_ehvi_grad.py
    observes the skipped upload of bogp_point_eval_ehvi)."""
    cfg = K.CONFIGS[1]
    p, st, ref = reference_of(cfg)
    rows = p["rows"][:4]
    sets = dict(a=(p["lower"], p["upper"]), b=(p["lower"][:1] - 0.5, np.full((1, cfg.m), INF)), c=(p["lower"] + 0.01, p["upper"] + 0.01),
                n=(np.zeros((0, cfg.m)), np.zeros((0, cfg.m))))  # fmt: skip
    fresh = {}
    for name, (lower, upper) in sets.items():
        e = _lib.Engine(0)
        _commit(e, cfg, p)
        fresh[name] = e.point_eval_ehvi_constrained(rows, lower, upper, p["lo"], p["hi"])
        e.close()
    _commit(eng, cfg, p)
    eng.upload_candidates(rows)

    def same(name):
        out = eng.point_eval_ehvi_constrained(rows, *sets[name], p["lo"], p["hi"])
        return out[0].tobytes() == fresh[name][0].tobytes() and out[1].tobytes() == fresh[name][1].tobytes()

    assert same("a") and same("a") and same("b") and same("a") and same("c") and same("a") and same("n") and same("a")
    eng.sweep_ehvi_constrained(*sets["b"], p["lo"], p["hi"])  # overwrites the resident cells
    assert same("a")
    eng.sweep_ehvi_constrained(*sets["c"], p["lo"], p["hi"])  # same (m, C) as set a
    assert same("a") and same("b")
    blo, bhi = np.full(cfg.d, BOX[0]), np.full(cfg.d, BOX[1])
    xs, fs, _ = eng.polish_ehvi_constrained(rows, blo, bhi, *sets["c"], p["lo"], p["hi"], max_evals=1)
    assert fs.tobytes() == fresh["c"][0].tobytes() and same("a")


def test_error_returns(eng):
    """One call per line of the ABI's INVALID / UNSUPPORTED lists; afterwards the handle still sweeps and evaluates as before."""
    lib, dp = eng._lib, C.POINTER(C.c_double)
    cfg = K.CONFIGS[1]  # N = 37, d = 2, (m, c) = (2, 2)
    p, st, ref = reference_of(cfg)
    rows, lower, upper, lo, hi = p["rows"][:3], p["lower"], p["upper"], p["lo"], p["hi"]
    blo, bhi = np.full(2, BOX[0]), np.full(2, BOX[1])

    def ptr(a):
        return None if a is None else np.ascontiguousarray(a, dtype=float).ctypes.data_as(dp)

    def ev(e, Xb=rows, B=3, m_obj=2, Cn=len(lower), lower_=lower, upper_=upper, n_con=2, lo_=lo, hi_=hi, out=True):
        v, g = np.empty(max(B, 1)), np.empty((max(B, 1), 2))
        return lib.bogp_point_eval_ehvi_constrained(e._h, ptr(Xb), B, m_obj, Cn, ptr(lower_), ptr(upper_), n_con, ptr(lo_), ptr(hi_),
                                                    ptr(v) if out else None, ptr(g), None, None, None, None, None, None, None, None)

    def po(e, X0=rows, B=3, blo_=blo, bhi_=bhi, m_obj=2, Cn=len(lower), lower_=lower, upper_=upper, n_con=2, lo_=lo, hi_=hi, max_evals=5, out=True):
        xo, fo = np.empty((max(B, 1), 2)), np.empty(max(B, 1))
        return lib.bogp_polish_ehvi_constrained(e._h, ptr(X0), B, ptr(blo_), ptr(bhi_), m_obj, Cn, ptr(lower_), ptr(upper_), n_con, ptr(lo_),
                                                ptr(hi_), max_evals, 1e-8, 1e6, ptr(xo) if out else None, ptr(fo), None)

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    fresh = _lib.Engine(0)
    fresh.set_train(p["X"], p["Y"])
    assert ev(fresh) == INV and po(fresh) == INV  # no committed model
    fresh.close()
    _commit(eng, cfg, p)
    eng.upload_candidates(rows)
    assert ev(eng) == 0 and po(eng) == 0
    before = eng.point_eval_ehvi_constrained(rows, lower, upper, lo, hi)
    sweep_before = eng.sweep_ehvi_constrained(lower, upper, lo, hi, return_values=True)[2]
    assert ev(eng, m_obj=1, n_con=3, lo_=np.r_[lo, 0.0], hi_=np.r_[hi, 1.0]) == INV and po(eng, m_obj=1, n_con=3, lo_=np.r_[lo, 0.0], hi_=np.r_[hi, 1.0]) == INV
    assert ev(eng, m_obj=4, n_con=0) == INV and po(eng, m_obj=4, n_con=0) == INV  # n_con < 1
    assert ev(eng, n_con=1) == INV and po(eng, n_con=1) == INV and ev(eng, m_obj=3) == INV and po(eng, m_obj=3) == INV  # m_obj + n_con != n_targets
    assert ev(eng, Cn=-1) == INV and po(eng, Cn=-1) == INV and ev(eng, Cn=_lib.MAX_EHVI_CELLS + 1) == INV and po(eng, Cn=_lib.MAX_EHVI_CELLS + 1) == INV
    bad = lower.copy()
    bad[0, 0] = -INF
    assert ev(eng, lower_=bad) == INV and po(eng, lower_=bad) == INV  # a lower cell bound that is not finite
    bad = upper.copy()
    bad[0, 1] = np.nan
    assert ev(eng, upper_=bad) == INV and po(eng, upper_=bad) == INV
    assert ev(eng, upper_=lower - 1.0) == INV and po(eng, upper_=lower - 1.0) == INV  # upper below lower
    assert ev(eng, lower_=None) == INV and ev(eng, upper_=None) == INV and po(eng, lower_=None) == INV  # C >= 1 needs the cells
    assert ev(eng, Cn=0, lower_=None, upper_=None) == 0 and po(eng, Cn=0, lower_=None, upper_=None) == 0  # ... C == 0 does not
    for l_, h_ in (([np.nan, 0.0], [0.0, 1.0]), ([0.0, 0.0], [np.nan, 1.0]), ([1.0, 0.0], [0.0, 1.0])):  # NaN bounds, hi < lo
        assert ev(eng, lo_=l_, hi_=h_) == INV and po(eng, lo_=l_, hi_=h_) == INV
    assert ev(eng, lo_=[0.5, 0.0], hi_=[0.5, 1.0]) == 0  # (hi == lo is allowed)
    assert ev(eng, Xb=None) == INV and ev(eng, out=False) == INV and ev(eng, lo_=None) == INV and ev(eng, hi_=None) == INV  # null pointers
    assert po(eng, X0=None) == INV and po(eng, out=False) == INV and po(eng, blo_=None) == INV and po(eng, bhi_=None) == INV and po(eng, lo_=None) == INV
    assert ev(eng, B=0) == INV and po(eng, B=0) == INV and ev(eng, B=-1) == INV
    assert po(eng, blo_=bhi, bhi_=blo) == INV and po(eng, max_evals=0) == INV
    # a polynomial basis: unsupported (check_multi_model's words)
    lin = _lib.Engine(0)
    lin.set_train(p["X"], p["Y"][:, :1])
    lin.commit(cfg.kernel, p["mode"], p["par"], 0.0, True, 0.0, trend=_lib.TREND_LINEAR)
    assert ev(lin) == UNS and po(lin) == UNS
    assert "constant trend only" in lib.bogp_last_error(lin._h).decode()
    lin.close()
    # kernels without corr_dx
    k2 = _lib.Engine(0)
    k2.set_train(p["X"], p["Y"])
    k2.commit(_lib.KERNEL_MATERN_NU, _lib.MODE_NOISELESS, np.r_[np.full(2, 100.0), 1.7], 0.0, False, 0.0)
    assert ev(k2) == UNS and po(k2) == UNS
    k2.commit(_lib.KERNEL_CUBIC, _lib.MODE_NOISELESS, np.full(2, 100.0), 0.0, False, 0.0)
    assert ev(k2) == UNS and po(k2) == UNS
    k2.close()
    # a forest on the handle
    fo = _lib.Engine(0)
    fo.forest_set_multi(**_tiny_forest(4))
    assert ev(fo) == UNS and po(fo) == UNS
    fo.close()
    # the handle is as it was: active target, candidates, sweeps, the evaluation itself
    after = eng.point_eval_ehvi_constrained(rows, lower, upper, lo, hi)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert eng.sweep_ehvi_constrained(lower, upper, lo, hi, return_values=True)[2].tobytes() == sweep_before.tobytes()
    mu1, _ = eng.predict()
    eng.select_target(1)
    eng.point_eval_ehvi_constrained(rows, lower, upper, lo, hi)
    eng.polish_ehvi_constrained(rows, blo, bhi, lower, upper, lo, hi, max_evals=3)
    assert not np.array_equal(eng.predict()[0], mu1)  # still target 1
    eng.select_target(0)
    assert np.array_equal(eng.predict()[0], mu1)
    best, idx = eng.sweep([(_lib.ACQ_EI, 0.0)], float(p["Y"][:, 0].min()), True)  # a single-target sweep on the active target still runs
    assert np.isfinite(best[0]) and 0 <= idx[0] < 3
