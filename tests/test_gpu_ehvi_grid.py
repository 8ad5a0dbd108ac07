"""EHVI factored over the grid of the front's cells on the device (`bogp_sweep_ehvi_grid`, kernels_ehvi_grid.hip) against the
float64 restatement of the reference's algebra on the device's own moments and the expanded cells, against `bogp_sweep_ehvi` on
those cells (T12, moments byte for byte), the winners by np.argmax's rule; chunks, the neighbouring sweeps, the refusals.  The
fronts are synthetic: the kernel deals 16 lanes per row up to E = sum n_k + V = 192 table entries, 64 up to 768, no table beyond."""
import types

import numpy as np
import pytest
from scipy.special import ndtr

from bogp import _lib
from bogp import pareto
from support.ehvi_ref64 import ehvi as ehvi_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _model(eng, m, N, d, seed, ratio=0.95):
    """An m-target model at fixed hyper-parameters: across candidate rows the means spread over most of the targets' range and the
    deviations are a fraction of it."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, size=(N, d))
    Y = X @ rng.normal(size=(d, m)) / np.sqrt(d) + 0.2 * np.sin(X @ rng.normal(size=(d, m)))
    Y *= 10.0 + 2.5 * np.arange(m)  # (scaled up: the commit refuses a likelihood above 1, which so few smooth rows reach)
    eng.set_train(X, Y)
    theta = 0.3 / d if d > 1 else 30.0  # (d = 1: 64 rows on a line want a short length scale)
    eng.commit(_lib.KERNEL_SE, _lib.MODE_NOISE_ESTIM, np.r_[np.full(d, theta), ratio], 0.0, False, 0.0)
    return X, Y


def _grid(front, m, Y, rng, h=0.7):
    """The grid of a named front, in units of the targets' spread s around their mean c."""
    c, s = Y.mean(axis=0), Y.std(axis=0) + 1e-3
    ref = c - (h + 0.5) * s
    if front == "lopsided":  # no front gives it: one interval on axis 0, 400 on axis 1, 400 last-axis values (E = 801: no table, m = 3)
        e1 = np.r_[c[1] + s[1] * np.linspace(-1, 1, 400), np.inf]
        last = c[2] + s[2] * np.linspace(-1.0, 0.0, 400)
        return pareto.HypercellGrid([np.array([ref[0], np.inf]), e1], last, rng.permutation(400))
    P = int(front[1:]) if front[0] == "P" else 3
    F = np.empty((P, m))
    up = np.linspace(-h, h, P) if P else np.empty(0)
    F[:, 0], F[:, -1] = up, up[::-1] * 0.4 - 0.6  # axis 0 rises, the last axis falls (and stays low): no point dominates another
    for k in range(1, m - 1):
        F[:, k] = rng.permutation(up)
    if front == "m8":  # three points that share their coordinate on axes 1 .. 6: n = (4, 2, 2, 2, 2, 2, 2), 256 columns
        F[:, 1:-1] = 0.3
    if front == "unequal":  # m = 5: n = (4, 3, 2, 4)
        F[:, 1], F[:, 2], F[:, 3] = [0.1, 0.1, 0.5], 0.2, [0.6, -0.2, 0.3]
    return pareto.hypercell_grid(c + s * F, ref)


def _rank(v, k):
    """np.argmax's rule, k times: the first maximum, a NaN maximal; slots beyond the rows are (-inf, -1)."""
    order = sorted(range(len(v)), key=lambda j: (not np.isnan(v[j]), -v[j] if not np.isnan(v[j]) else 0.0, j))[:k]
    idx = np.r_[order, np.full(k - len(order), -1)].astype(np.int64)
    return np.r_[v[order], np.full(k - len(order), -np.inf)], idx


def _cell_terms(mu, mse, lower, upper):
    """M x C: the term of every cell, prod_k sd_k (G(a) - G(b)), in NumPy."""
    sd = np.sqrt(np.maximum(mse, 1e-9))[:, None, :]
    G = lambda z: np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi) - z * ndtr(-z)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):  # (rows at the variance floor: z^2 overflows where G is 0 or -z anyway)
        gu = np.where(np.isinf(upper)[None], 0.0, G((np.minimum(upper, 1e300)[None] - mu[:, None, :]) / sd))
        return np.prod(sd * (G((lower[None] - mu[:, None, :]) / sd) - gu), axis=2)


CASES = [  # (M, N, d, m, front): columns, E -> the kernel's variant
    (1, 5, 1, 2, "P0"),          # 1 column, V = 1; k = 16 > M
    (63, 64, 5, 2, "P62"),       # 63 columns
    (64, 67, 20, 2, "P63"),      # 64
    (65, 5, 5, 2, "P64"),        # 65
    (255, 64, 1, 2, "P95"),      # E = 192: the last 16-lane table
    (256, 67, 5, 2, "P96"),      # E = 194: the first 64-lane table
    (257, 64, 20, 2, "P383"),    # E = 768: the last table
    (257, 5, 5, 2, "P384"),      # E = 770: no table
    (255, 67, 5, 3, "lopsided"),  # E = 801: no table, three objectives
    (1000, 67, 5, 3, "P32"),     # 1089 columns
    (1000, 64, 1, 4, "P6"),      # 343 columns; two identical rows
    (255, 67, 20, 5, "unequal"),  # n = (4, 3, 2, 4)
    (65, 64, 5, 8, "m8"),        # n = (4, 2 x 6), P = 3
]


@pytest.mark.parametrize("M,N,d,m,front", CASES)
def test_grid_sweep_matches_restatement_loop_and_argmax(eng, M, N, d, m, front):
    rng = np.random.default_rng(M + N + d + m)
    X, Y = _model(eng, m, N, d, seed=M + m, ratio=0.98 if front == "P32" else 0.95)  # (P32: a smaller nugget and a wider front,
    grid = _grid(front, m, Y, rng, h=0.9 if front == "P32" else 0.7)                 # what the share asserted below takes)
    lower, upper = pareto.expand_grid(grid)
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    if front == "P6":
        Xs[7] = Xs[3]
    eng.upload_candidates(Xs)
    best, idx, vals, mu, mse = eng.sweep_ehvi_grid(grid, k=1, return_values=True, return_moments=True)
    lbest, lidx, lvals, lmu, lmse = eng.sweep_ehvi(lower, upper, k=1, return_values=True, return_moments=True)
    assert mu.tobytes() == lmu.tobytes() and mse.tobytes() == lmse.tobytes()
    ref = ehvi_ref(mu, mse, lower, upper)
    tol = 1e-6 * np.abs(ref) + 1e-12 * np.abs(ref).max()  # T12
    assert np.all(np.abs(vals - ref) <= tol), np.max(np.abs(vals - ref) / tol)
    assert np.all(np.abs(vals - lvals) <= tol), np.max(np.abs(vals - lvals) / tol)
    assert ref.max() > 0
    for k in (1, 16):
        bk, ik = eng.sweep_ehvi_grid(grid, k=k)
        wb, wi = _rank(vals, k)
        assert np.array_equal(ik, wi) and np.array_equal(bk, wb), (k, ik, wi)
    assert best[0] == vals[idx[0]] and idx[0] == int(np.argmax(vals))
    assert front != "P6" or vals[7] == vals[3]
    if front == "P32":  # rtol 1e-6 cannot hide a dropped column: each one carries 1e-3 of some row's EHVI
        assert len(lower) == 1089
        share = _cell_terms(mu, mse, lower, upper)[ref > 0] / ref[ref > 0, None]
        assert share.max(axis=0).min() >= 1e-3, share.max(axis=0).min()


def test_chunks_and_the_sweeps_around_it(eng, monkeypatch):
    X, Y = _model(eng, 3, 700, 5, seed=3)
    grid = _grid("P32", 3, Y, np.random.default_rng(0))
    lower, upper = pareto.expand_grid(grid)
    eng.upload_candidates(np.random.default_rng(2).uniform(-2.2, 2.2, size=(1000, 5)))
    acq = [(_lib.ACQ_EI, 0.0), (_lib.ACQ_UCB, 1.0)]
    before = eng.sweep(acq, float(Y[:, 0].min()), True, return_values=True) + eng.sweep_ehvi(lower, upper, k=3, return_values=True, return_moments=True)
    one = eng.sweep_ehvi_grid(grid, k=5, return_values=True, return_moments=True)
    assert eng.last_timing()["acquisition_ms"] > 0
    after = eng.sweep(acq, float(Y[:, 0].min()), True, return_values=True) + eng.sweep_ehvi(lower, upper, k=3, return_values=True, return_moments=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")  # 128 candidates per chunk at Np = 704: 8 chunks
    chunked = eng.sweep_ehvi_grid(grid, k=5, return_values=True, return_moments=True)
    assert eng.last_timing()["n_chunks"] >= 3
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, chunked))


def test_refusals_through_the_abi(eng):
    X, Y = _model(eng, 3, 67, 5, seed=9)
    eng.upload_candidates(np.zeros((8, 5)))
    inf = np.inf

    def call(edges=([0.0, 1.0, inf], [0.0, inf]), last_val=(0.0, 1.0), last_idx=(0, 1), k=1):
        return eng.sweep_ehvi_grid(types.SimpleNamespace(edges=list(edges), last_val=last_val, last_idx=last_idx), k=k)

    call()
    wide = np.r_[np.arange(300.0), inf]
    for match, kw in [
        ("m = 2", dict(edges=([0.0, inf],), last_idx=(0,), last_val=(0.0,))),  # bogp_sweep_ehvi's own, in its order
        ("k = 33", dict(k=33)),
        ("axis 1 has 0", dict(edges=([0.0, 1.0, inf], [inf]))),
        ("up to axis 1", dict(edges=(wide, wide), last_idx=np.zeros(90000, dtype=np.int32))),
        ("axis 0: the first edge", dict(edges=([-inf, 1.0, inf], [0.0, inf]))),
        ("axis 0: edge 1", dict(edges=([0.0, 0.0, inf], [0.0, inf]))),
        ("axis 0: edge 2", dict(edges=([0.0, 1.0, np.nan], [0.0, inf]))),
        ("axis 1: the last edge", dict(edges=([0.0, 1.0, inf], [0.0, 2.0]))),
        ("V = 3", dict(last_val=(0.0, 1.0, 2.0))),
        ("V = 0", dict(last_val=())),
        (r"last_val\[1\] is not finite", dict(last_val=(0.0, inf))),
        (r"last_val\[1\] \(0\) is not above", dict(last_val=(0.0, 0.0))),
        (r"last_idx\[1\] = 2", dict(last_idx=(0, 2))),
        (r"last_idx\[0\] = -1", dict(last_idx=(-1, 0))),
    ]:
        with pytest.raises(_lib.BogpError, match=match) as err:
            call(**kw)
        assert err.value.code == _lib.ERR_INVALID
    n, best, idx = np.array([2, 1], dtype=np.int32), np.empty(1), np.empty(1, dtype=np.int64)  # a null array: the raw call only
    args = [eng._h, 3, n.ctypes.data_as(_lib._ip), None, 2, None, None, 1, _lib._ptr(best), idx.ctypes.data_as(_lib._lp), None, None, None]
    assert eng._lib.bogp_sweep_ehvi_grid(*args) == _lib.ERR_INVALID and b"non-null" in eng._lib.bogp_last_error(eng._h)
    call()
