"""Constrained EHVI factored over the grid of the feasible front's cells, on the live rows only (`bogp_sweep_ehvi_constrained_grid`,
kernels_ehvi_constrained_grid.hip) against `bogp_sweep_ehvi_constrained` on the expanded cells (moments and P byte for byte, values to
T12) and the float64 restatement of EHVI on the device's own moments times the device's P; +0.0 on dead rows; the winners by
np.argmax's rule; a live row's bytes whatever its neighbours; chunks, the neighbouring sweeps, the refusals."""
import types

import numpy as np
import pytest

from bogp import _lib, pareto
from support.ehvi_ref64 import ehvi as ehvi_ref
from test_gpu_ehvi import _model as _noiseless_model
from test_gpu_ehvi_grid import _cell_terms, _grid, _model, _rank

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _bounds(Y, mo):
    """(-inf, q60] on the first constraint column, [q10, +inf) on the others"""
    q = [np.quantile(Y[:, mo + j], 0.6 if j == 0 else 0.1) for j in range(Y.shape[1] - mo)]
    return np.array([-INF] + q[1:]), np.array(q[:1] + [INF] * (len(q) - 1))


def _t12(v, ref):
    tol = 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()
    print("T12: max err / allowance = %.3g" % np.max(np.abs(v - ref) / tol))
    assert np.all(np.abs(v - ref) <= tol), np.max(np.abs(v - ref) / tol)


CASES = [  # (M, N, d, MO, MT, front): E -> the kernel's variant
    (1, 5, 1, 2, 3, "P0"),         # one column; k = 16 > M
    (255, 64, 1, 2, 3, "P95"),     # E = 192: the last 16-lane table
    (256, 67, 5, 2, 5, "P96"),     # E = 194: the first 64-lane table
    (257, 64, 20, 2, 3, "P383"),   # E = 768: the last table
    (257, 5, 5, 2, 5, "P384"),     # E = 770: no table
    (1000, 67, 5, 3, 4, "lopsided"),  # E = 801: no table, three objectives
    (1000, 67, 5, 3, 4, "P32"),    # 1089 columns
    (1000, 64, 1, 4, 5, "P6"),     # 343 columns
    (255, 67, 20, 7, 8, "m8"),     # n = (4, 2 x 5)
    (256, 64, 5, 2, 8, "P64"),     # six constraints
    (257, 67, 5, 3, 4, "P6"),
    (1, 67, 5, 4, 5, "P0"),
]


@pytest.mark.parametrize("M,N,d,mo,mt,front", CASES)
def test_grid_sweep_matches_the_loop_the_restatement_and_argmax(eng, M, N, d, mo, mt, front):
    rng = np.random.default_rng(M + N + d + mo + mt)
    X, Y = _model(eng, mt, N, d, seed=M + mt, ratio=0.98 if front == "P32" else 0.95)
    grid = _grid(front, mo, Y[:, :mo], rng, h=0.9 if front == "P32" else 0.7)
    lower, upper = pareto.expand_grid(grid)
    lo, hi = _bounds(Y, mo)
    eng.upload_candidates(rng.uniform(-2.2, 2.2, size=(M, d)))
    kw = dict(return_values=True, return_pof=True, return_moments=True)
    best, idx, vals, pof, mu, mse = eng.sweep_ehvi_constrained_grid(grid, lo, hi, **kw)
    lbest, lidx, lvals, lpof, lmu, lmse = eng.sweep_ehvi_constrained(lower, upper, lo, hi, **kw)
    assert mu.tobytes() == lmu.tobytes() and mse.tobytes() == lmse.tobytes() and pof.tobytes() == lpof.tobytes()
    e = ehvi_ref(mu[:, :mo], mse[:, :mo], lower, upper)
    ref = e * pof
    assert ref.max() > 0
    _t12(vals, lvals)
    _t12(vals, ref)
    dead = pof == 0
    assert np.all(vals[dead] == 0.0) and not np.any(np.signbit(vals[dead]))
    for k in (1, 16):
        bk, ik = eng.sweep_ehvi_constrained_grid(grid, lo, hi, k=k)
        wb, wi = _rank(vals, k)
        assert np.array_equal(ik, wi) and np.array_equal(bk, wb), (k, ik, wi)
    if front == "P32":  # rtol 1e-6 cannot hide a dropped column: each one carries 1e-3 of some row's EHVI
        assert len(lower) == 1089
        share = _cell_terms(mu[:, :mo], mse[:, :mo], lower, upper)[e > 0] / e[e > 0, None]
        assert share.max(axis=0).min() >= 1e-3, share.max(axis=0).min()


def _patterns():
    """name -> the live rows among 512 (two workgroups); NG = 16 groups of 16 lanes or 4 groups of 64 take NG listed rows at a time"""
    rng = np.random.default_rng(4)
    pat = {"none": [], "only 255": [255], "alternating": range(0, 512, 2), "all": range(512), "dead block, live block": range(256, 512)}
    for n in (3, 4, 5, 15, 16, 17):
        pat["%d live" % n] = np.sort(rng.choice(256, n, replace=False))
    return {k: np.isin(np.arange(512), np.asarray(list(v), dtype=int)) for k, v in pat.items()}


@pytest.mark.parametrize("mo,front", [(3, "P32"), (2, "P96")])  # 16 lanes per row (E = 99), 64 lanes per row (E = 194)
def test_a_live_row_has_the_same_bytes_whatever_its_neighbours(eng, mo, front):
    # an interpolating model: P is exactly 0 or 1 on its training rows (the variance guard) and strictly between on rows far from them
    X, Y, _, _ = _noiseless_model(eng, mo + 1, 300, 5, _lib.KERNEL_MATERN52, False, seed=11)
    grid = _grid(front, mo, Y[:, :mo], np.random.default_rng(1))
    col = np.sort(Y[:, mo])
    j = 65 + int(np.argmax(np.diff(col[65:86])))  # about three quarters of the training rows infeasible, the bound in a wide gap
    hi = np.array([0.5 * (col[j] + col[j + 1])])
    lo = np.array([-INF])
    pool = np.vstack([X, np.random.default_rng(5).uniform(-2.5, 2.5, size=(480, 5))])
    eng.upload_candidates(pool)
    pof = eng.sweep_ehvi_constrained_grid(grid, lo, hi, return_pof=True)[2]
    dead_rows, live_rows = pool[pof == 0], pool[pof != 0]
    assert 0.2 <= np.mean(pof == 0) <= 0.8 and len(live_rows) >= 512, (np.mean(pof == 0), len(live_rows))
    seen = {}
    for name, live in _patterns().items():
        Xs = dead_rows[np.arange(512) % len(dead_rows)]
        Xs[live] = live_rows[: live.sum()]  # live row j of the pool stands at the pattern's j-th live place
        eng.upload_candidates(Xs)
        _, _, vals, p = eng.sweep_ehvi_constrained_grid(grid, lo, hi, return_values=True, return_pof=True)
        assert np.array_equal(p != 0, live), name
        assert np.all(vals[~live] == 0.0) and not np.any(np.signbit(vals[~live])), name
        for j, v in enumerate(vals[live]):
            assert seen.setdefault(j, v.tobytes()) == v.tobytes(), (name, j)
    assert len(seen) == 512 and any(np.frombuffer(b)[0] > 0 for b in seen.values())


def test_chunks_and_the_sweeps_around_it(eng, monkeypatch):
    X, Y = _model(eng, 4, 700, 5, seed=3)
    grid = _grid("P32", 3, Y[:, :3], np.random.default_rng(0))
    lower, upper = pareto.expand_grid(grid)
    lo, hi = _bounds(Y, 3)
    g4 = _grid("P6", 4, Y, np.random.default_rng(0))
    eng.upload_candidates(np.random.default_rng(2).uniform(-2.2, 2.2, size=(1000, 5)))
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 1.0)]
    kw = dict(return_values=True, return_pof=True, return_moments=True)

    def around():
        return (eng.sweep(acq, float(Y[:, 0].min()), True, return_values=True) + eng.sweep_ehvi_constrained(lower, upper, lo, hi, k=3, **kw)
                + eng.sweep_ehvi_grid(g4, k=3, return_values=True, return_moments=True))  # fmt: skip

    before = around()
    one = eng.sweep_ehvi_constrained_grid(grid, lo, hi, k=5, **kw)
    assert eng.last_timing()["acquisition_ms"] > 0
    after = around()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 candidates per chunk at Np = 704: 8 chunks
    chunked = eng.sweep_ehvi_constrained_grid(grid, lo, hi, k=5, **kw)
    assert eng.last_timing()["n_chunks"] >= 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, chunked))


def test_refusals_through_the_abi(eng):
    _model(eng, 3, 67, 5, seed=9)
    eng.upload_candidates(np.zeros((8, 5)))

    def call(edges=([0.0, 1.0, INF],), last_val=(0.0, 1.0), last_idx=(0, 1), lo=(-INF,), hi=(0.0,)):
        return eng.sweep_ehvi_constrained_grid(types.SimpleNamespace(edges=list(edges), last_val=last_val, last_idx=last_idx), lo, hi)

    call()
    for match, kw in [
        ("m_obj \\+ n_con = 3 \\+ 1", dict(edges=([0.0, 1.0, INF], [0.0, INF]))),  # every column an objective: no constraint column left
        ("upper bound of constraint 0 \\(0\\) is below", dict(lo=(1.0,), hi=(0.0,))),
        ("a bound of constraint 0 is NaN", dict(hi=(np.nan,))),
        ("axis 0: edge 1", dict(edges=([0.0, 0.0, INF],))),
    ]:
        with pytest.raises(_lib.BogpError, match=match) as err:
            call(**kw)
        assert err.value.code == _lib.ERR_INVALID
    n, best, idx, b = np.array([2], dtype=np.int32), np.empty(1), np.empty(1, dtype=np.int64), np.zeros(1)  # a null array: the raw call only
    args = [eng._h, 2, n.ctypes.data_as(_lib._ip), None, 2, None, None, 1, _lib._ptr(b), _lib._ptr(b), 1, _lib._ptr(best),
            idx.ctypes.data_as(_lib._lp), None, None, None, None]  # fmt: skip
    assert eng._lib.bogp_sweep_ehvi_constrained_grid(*args) == _lib.ERR_INVALID
    assert b"bogp_sweep_ehvi_constrained_grid: edges, last_val and last_idx must be non-null" in eng._lib.bogp_last_error(eng._h)
    call()
