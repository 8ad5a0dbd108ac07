"""EHVI over forests with several outputs on the device (`bogp_forest_set_multi` / `_predict_multi` / `_leaves_multi` / `_sweep_ehvi`,
csrc/kernels_forest_ehvi.hip) against the reference's multi-output `RandomForest` and its `EHVI` as recorded in
tests/golden/G42_forest_ehvi.npz (tests/support/make_forest_ehvi_golden.py): per-tree, per-output predictions bit for bit, mu / MSE at
the ledger's T1 / T2, EHVI at T12 against the float64 restatement and at 1e-5 of the batch maximum against the reference's own float32
values, argmax / top 16 exactly (ties included); cell and output shapes, the kernel's size edges and the ABI's error returns against a
NumPy restatement (tests/support/forest_ehvi_engine.py); the generated sweep end to end.

Figures measured on an MI355X: this file's parity tests print them and profiles/forest_ehvi_parity.txt keeps them."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

from bogp import _lib
from bogp import forest as F
from support import ehvi_ref64
from support import forest_ehvi_engine as S

pytestmark = pytest.mark.gpu

PARITY = os.path.join(ROOT, "profiles", "forest_ehvi_parity.txt")
MODELS = ["mx2_", "mx3_", "ds2_"]
LABELS = {"mx2_": (["red", "green", "blue", "cyan", "black"], ["x", "y", "z"]), "mx3_": (["red", "green", "blue", "cyan", "black"], ["x", "y", "z"]),
          "ds2_": (["x", "y", "z"],)}


@pytest.fixture(scope="module")
def g():
    return load_golden("G42_forest_ehvi")


@pytest.fixture()
def eng():
    e = _lib.Engine(0)
    yield e
    e.close()


def _packed(g, p):
    cat_idx = [int(v) for v in g[p + "cat_idx"]]
    cats = [list(range(int(n))) for n in g[p + "cat_sizes"]]
    d_raw = int(g[p + "d_raw"])
    noncat = [v for v in range(d_raw) if v not in cat_idx]
    return F.PackedForest(g[p + "tree_offset"], g[p + "feature"], g[p + "threshold"], g[p + "left"], g[p + "right"], g[p + "value"],
                          d_raw, noncat, cat_idx, cats)


def _raw_rows(pk, enc):
    """Encoded rows -> raw rows (level indices in the categorical columns)."""
    enc = np.asarray(enc, dtype=np.float64)
    out = np.zeros((len(enc), pk.d_raw))
    for c, (v, l) in enumerate(pk.enc_cols):
        if l < 0:
            out[:, v] = enc[:, c]
        else:
            out[:, v] += l * enc[:, c]
    return out


def _set(eng, pk, raw):
    if raw:
        f, t, test = pk.raw()
        eng.forest_set_multi(pk.d_raw, pk.m, pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
    else:
        eng.forest_set_multi(pk.d_enc, pk.m, pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value)


def _upload(eng, g, p, pk, raw):
    enc = g[p + "Xenc"]
    eng.upload_candidates(_raw_rows(pk, enc) if raw else enc.astype(np.float64))


_SECTIONS = {}


def _write_parity(section, lines):
    """profiles/forest_ehvi_parity.txt: the figures of this run, one section per parity test."""
    _SECTIONS[section] = lines
    try:
        with open(PARITY, "w") as f:
            f.write("Observed errors of the device forest EHVI against tests/golden/G42_forest_ehvi.npz (tests/test_gpu_forest_ehvi.py, MI355X)\n")
            for name, ls in _SECTIONS.items():
                f.write("## %s\n%s\n" % (name, "\n".join(ls)))
    except OSError:
        pass


def _check_moments_and_ehvi(mu, mse, vals, rmu, rmse, rvals):
    """T1 / T2 / T12; returns the observed errors."""
    np.testing.assert_allclose(mu, rmu, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(mse, rmse, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(vals, rvals, rtol=1e-6, atol=1e-12 * float(np.max(np.abs(rvals))))
    return (float(np.max(np.abs(mu - rmu))), float(np.max(np.abs(mse - rmse))),
            float(np.max(np.abs(vals - rvals)) / max(float(np.max(np.abs(rvals))), 1e-300)))


@pytest.mark.parametrize("raw", [False, True], ids=["encoded", "raw-columns"])
@pytest.mark.parametrize("p", MODELS)
def test_per_tree_per_output_predictions_are_bit_identical(eng, g, p, raw):
    """`bogp_forest_leaves_multi` == `estimators_[t].predict` (256, T, m) for the recorded rows, in the forest's own encoded columns and
    rewritten onto the raw columns; the same bits at other offsets of the launch."""
    pk = _packed(g, p)
    _set(eng, pk, raw)
    assert eng.forest_outputs() == pk.m == g[p + "mu"].shape[1]
    _upload(eng, g, p, pk, raw)
    want = g[p + "per_tree"]
    assert np.array_equal(eng.forest_leaves_multi(0, 256), want)
    for first, n in ((37, 150), (255, 1)):
        assert np.array_equal(eng.forest_leaves_multi(first, n), want[first : first + n])


def test_moments_match_the_reference(eng, g):
    """mu at rtol 1e-6 / atol 1e-9 (ledger T1), MSE at rtol 1e-6 / atol 1e-12 (T2; y lies in [-1, 0]), all three forests, encoded and raw
    columns; `predict_multi` without MSE gives the same mu bits.  Observed on an MI355X: profiles/forest_ehvi_parity.txt."""
    lines = []
    for p in MODELS:
        pk = _packed(g, p)
        for raw in (False, True):
            _set(eng, pk, raw)
            _upload(eng, g, p, pk, raw)
            mu, mse = eng.forest_predict_multi()
            rmu, rmse = g[p + "mu"], g[p + "mse"]
            assert mu.shape == mse.shape == rmu.shape
            lines.append("%s %s: max rel err mu %.3e, max abs err MSE %.3e (MSE in [%.3e, %.3e])"
                         % (p, "raw" if raw else "encoded", float(np.max(np.abs(mu - rmu) / np.abs(rmu))), float(np.max(np.abs(mse - rmse))),
                            rmse.min(), rmse.max()))
            print(lines[-1])
            np.testing.assert_allclose(mu, rmu, rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(mse, rmse, rtol=1e-6, atol=1e-12)
            mu_only, none = eng.forest_predict_multi(eval_MSE=False)
            assert none is None and np.array_equal(mu_only, mu)
    _write_parity("moments", lines)


def test_ehvi_matches_the_float64_values_and_the_reference_class(eng, g):
    """EHVI of all rows at rtol 1e-6 / atol 1e-12 max|EHVI| (T12) against tests/support/ehvi_ref64.py on the reference's moments; the first
    256 rows within 1e-5 of the batch maximum of the reference's own float32 values (its casts cost up to 1.9e-6, as recorded).
    Observed on an MI355X: within 3e-15 of the batch maximum of the float64 values (1.8e-9 relative over the rows above 1e-6 of it)."""
    lines = []
    for p in MODELS:
        pk = _packed(g, p)
        _set(eng, pk, True)
        _upload(eng, g, p, pk, True)
        best, idx, vals, mu, mse = eng.forest_sweep_ehvi(g[p + "lower"], g[p + "upper"], return_values=True, return_moments=True)
        ref = g[p + "ehvi64"]
        scale = float(np.max(np.abs(ref)))
        e64 = float(np.max(np.abs(vals - ref)) / scale)
        big = np.abs(ref) > 1e-6 * scale  # (below that the tail terms' relative error is unbounded: T12's atol)
        r64 = float(np.max(np.abs(vals - ref)[big] / np.abs(ref)[big]))
        e32 = float(np.max(np.abs(vals[:256] - g[p + "ehvi32"])) / scale)
        lines.append("%s: %d cells, max err against float64 %.3e of the batch maximum (max rel err %.3e over the %d rows above 1e-6 of it), "
                     "against the reference's float32 values %.3e of the batch maximum" % (p, len(g[p + "lower"]), e64, r64, int(big.sum()), e32))
        print(lines[-1])
        _check_moments_and_ehvi(mu, mse, vals, g[p + "mu"], g[p + "mse"], ref)
        assert e32 <= 1e-5
        assert best[0] == vals[idx[0]]
    _write_parity("ehvi", lines)


@pytest.mark.parametrize("raw", [False, True], ids=["encoded", "raw-columns"])
@pytest.mark.parametrize("p", MODELS)
def test_argmax_and_top16_are_exact(eng, g, p, raw):
    """Argmax and the 16 best rows are those of the float64 values on the reference's moments; on the all-discrete forest the tied maximum
    comes back at its lowest index and equal rows carry identical bits."""
    pk = _packed(g, p)
    _set(eng, pk, raw)
    _upload(eng, g, p, pk, raw)
    lo, hi = g[p + "lower"], g[p + "upper"]
    best, idx, vals = eng.forest_sweep_ehvi(lo, hi, k=16, return_values=True)
    b1, i1 = eng.forest_sweep_ehvi(lo, hi, k=1)
    want = g[p + "top16"]
    assert np.array_equal(idx, want), (idx, want)
    assert i1[0] == want[0] == int(g[p + "argmax"]) == int(np.argmax(vals)) and b1[0] == best[0]
    assert np.array_equal(best, vals[idx])
    if p == "ds2_":
        tied = np.flatnonzero(vals == vals.max())
        assert len(tied) == int(g["ds2_ties"]) >= 2 and idx[0] == tied[0]
        _, first, inv = np.unique(g[p + "Xenc"], axis=0, return_index=True, return_inverse=True)
        assert np.array_equal(vals.view(np.int64), vals[first[inv.ravel()]].view(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# without the reference: scikit-learn forests and synthetic ones against the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _cells(rng, C, m):
    """C cells in the range of y in [-1, 0]: widths >= 0.05 (no cancelling thin cells), every fifth upper bound +inf."""
    lower = rng.uniform(-1.2, -0.2, size=(C, m))
    upper = lower + rng.uniform(0.05, 0.5, size=(C, m))
    upper[rng.uniform(size=(C, m)) < 0.2] = np.inf
    return lower, upper


def _against_restatement(eng, forest, d, m, X, lower, upper, k=16):
    """Leaves bit for bit, T1 / T2 / T12 above them, the winners' order; returns the device values."""
    eng.forest_set_multi(d, m, *forest[:6], forest[6])
    eng.upload_candidates(X)
    M = len(X)
    P = S.leaves_multi(forest, X)
    assert np.array_equal(eng.forest_leaves_multi(0, M), P)
    rmu, rmse = S.moments_multi(P)
    best, idx, vals, mu, mse = eng.forest_sweep_ehvi(lower, upper, k=k, return_values=True, return_moments=True)
    errs = _check_moments_and_ehvi(mu, mse, vals, rmu, rmse, ehvi_ref64.ehvi(rmu, rmse, lower, upper))
    wb, wi = S.topk(vals, k)
    assert np.array_equal(idx, wi) and np.array_equal(best, wb)  # first maximum, ties to the lower index, (-inf, -1) beyond M
    return vals, mse, errs


@pytest.fixture(scope="module")
def sk_forests():
    """One small scikit-learn forest per m, fitted once: y in [-1, 0], constant (-0.5 in every output) for x0 < -1, so that all trees
    agree on rows well inside that region."""
    ens = pytest.importorskip("sklearn.ensemble")
    rng = np.random.default_rng(8)
    X = rng.uniform(-3, 3, size=(90, 4))
    out = {}
    for m in (2, 3, 8):
        W = rng.normal(size=(4, m))
        y = -1.0 / (1.0 + np.exp(-(X @ W)))
        y[X[:, 0] < -1] = -0.5
        rf = ens.RandomForestRegressor(n_estimators=7, min_samples_leaf=2, random_state=m).fit(X, y)
        pk = F.pack(rf, multi_output=True)
        out[m] = (pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value, None)
    return out


@pytest.mark.parametrize("m", [2, 3, 8])
def test_cell_and_output_shapes(eng, sk_forests, m):
    """m = 2, 3, 8 x C = 1, 300 x M = 1, 255, 257, 1000 (a partial last workgroup; slots beyond M are (-inf, -1)) against the NumPy
    per-tree restatement + ehvi_ref64, with +inf upper bounds; rows on which all trees agree give MSE exactly 0 and sd = sqrt(1e-9)."""
    rng = np.random.default_rng(100 + m)
    forest = sk_forests[m]
    lines = []
    for C in (1, 300):
        lower, upper = _cells(rng, C, m)
        assert np.isinf(upper).any() or C == 1
        for M in (1, 255, 257, 1000):
            X = rng.uniform(-3, 3, size=(M, 4))
            X[::3, 0] = rng.uniform(-3, -2.5, size=len(X[::3]))  # well inside the constant region
            vals, mse, errs = _against_restatement(eng, forest, 4, m, X, lower, upper)
            P = S.leaves_multi(forest, X)
            agree = np.all(P == P[:, :1, :], axis=(1, 2))  # rows on which every tree predicts the same m values
            assert np.all(mse[agree] == 0.0) and (agree.sum() >= 10 or M == 1)
            # sd = sqrt(1e-9) there: the value is the restatement's on MSE = 0 exactly (T12 above has checked it at the real one)
            want = ehvi_ref64.ehvi(P[agree][:, 0, :], np.zeros((int(agree.sum()), m)), lower, upper)
            np.testing.assert_allclose(vals[agree], want, rtol=1e-6, atol=1e-12 * float(np.max(np.abs(vals))))
            lines.append("m %d C %3d M %4d: max abs err mu %.2e, MSE %.2e, EHVI %.2e of the maximum" % ((m, C, M) + errs))
    print("\n".join(lines))
    _write_parity("shapes m = %d" % m, lines)


def _complete_forest(rng, T, depth, d, m):
    """T complete trees of `depth` levels as arrays (node i has the children 2 i + 1 and 2 i + 2), m values a leaf."""
    n = 2 ** (depth + 1) - 1
    inner = np.arange(n) < 2**depth - 1
    off = np.arange(T + 1, dtype=np.int64) * n
    feat = np.where(np.tile(inner, T), rng.integers(0, d, size=T * n), -2).astype(np.int32)
    thr = np.where(np.tile(inner, T), rng.uniform(-2, 2, size=T * n), -2.0)
    left = np.tile(np.where(inner, 2 * np.arange(n) + 1, -1), T).astype(np.int32)
    right = np.tile(np.where(inner, 2 * np.arange(n) + 2, -1), T).astype(np.int32)
    val = rng.uniform(-1, 0, size=(T * n, m))
    return (off, feat, thr, left, right, val, None)


@pytest.mark.parametrize("depth,m,lds_path", [(9, 2, False), (11, 2, True)], ids=["tree-above-1024-words", "lds-above-64KB"])
def test_size_edges_of_the_kernel(eng, depth, m, lds_path):
    """Synthetic forests built as arrays: trees of 1023 nodes + 512 x 2 values = 2047 words (past the 1024 words the lanes stage in
    registers) and of 4095 + 2048 x 2 = 8191 words (two buffers = 128 KB of LDS: the raised dynamic-LDS limit), against the restatement."""
    rng = np.random.default_rng(depth)
    d = 4
    forest = _complete_forest(rng, 3, depth, d, m)
    X = rng.uniform(-3, 3, size=(600, d))
    lower, upper = _cells(rng, 5, m)
    _, _, errs = _against_restatement(eng, forest, d, m, X, lower, upper)
    info = eng.forest_info()
    words = (2 ** (depth + 1) - 1) + m * 2**depth
    assert words > 1024 and info["lds_bytes"] == 2 * words * 8 + d * 1024 and (info["lds_bytes"] > 64 * 1024) == lds_path
    _write_parity("size edge depth %d" % depth, ["%d words a tree, %d bytes of LDS: max abs err mu %.2e, MSE %.2e, EHVI %.2e of the maximum"
                                                 % ((words, info["lds_bytes"]) + errs)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the generated sweep end to end
# ---------------------------------------------------------------------------------------------------------------------------------
class _Var:
    def __init__(self, bounds, name):
        self.bounds, self.name = bounds, name


class Real(_Var):
    scale, precision = "linear", None


class Integer(_Var):
    step = 1


class Discrete(_Var):
    pass


class _Space:
    def __init__(self, data):
        self.data = data
        self.var_name = [v.name for v in data]


class _Model:  # what forest.pack reads of a fitted forest with several outputs
    class _Tree:
        pass

    def __init__(self, g, p, labels):
        self.estimators_ = []
        off = g[p + "tree_offset"]
        m = g[p + "value"].shape[1]
        for t in range(len(off) - 1):
            e, tr = _Model._Tree(), _Model._Tree()
            s = slice(int(off[t]), int(off[t + 1]))
            tr.children_left, tr.children_right, tr.feature = g[p + "left"][s], g[p + "right"][s], g[p + "feature"][s]
            tr.threshold, tr.value = g[p + "threshold"][s], g[p + "value"][s].reshape(-1, m, 1)
            e.tree_ = tr
            self.estimators_.append(e)
        self.n_outputs_, self.n_features_in_ = m, int(g[p + "Xenc"].shape[1])
        self._cat_idx = [int(v) for v in g[p + "cat_idx"]]
        self._categories = [list(l) for l in labels]

    def predict(self, X, eval_MSE=False):
        return F.predict(self, X, eval_MSE)


_Model.__name__ = "RandomForest"


def test_generated_sweep_end_to_end(g):
    """`sweep-device` on the mixed space with M = 20 000: the winner, decoded to the reference's row format and re-evaluated through
    `criterion(X)`, gives the returned value; the same seed gives the same winner; the host-sampled sweep agrees with `criterion(X)`."""
    import bogp

    p = "mx2_"
    model = _Model(g, p, LABELS[p])
    space = _Space([Real((-5.0, 5.0), "r%d" % k) for k in range(3)] + [Integer((0, 10), "i0"), Discrete(LABELS[p][0], "c0"),
                                                                     Discrete(LABELS[p][1], "c1")])
    crit = bogp.EHVI(model=model, ref_point=g[p + "ref_point"], cells=(g[p + "lower"], g[p + "upper"]))
    np.random.seed(11)
    x, f = bogp.argmax_restart(crit, space, eval_budget=20_000, optimizer="sweep-device")
    assert len(x) == 6 and all(isinstance(v, float) for v in x[:3]) and isinstance(x[3], int) and 0 <= x[3] <= 10
    assert x[4] in LABELS[p][0] and x[5] in LABELS[p][1]
    again = crit([x])
    assert again.shape == (1,) and again[0] == f  # a row's result depends on the row and the forest alone
    pk = F.pack(model, multi_output=True)
    mu, mse = S.moments_multi(S.leaves_multi((pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value, None), pk.encode([x])))
    np.testing.assert_allclose(f, ehvi_ref64.ehvi(mu, mse, g[p + "lower"], g[p + "upper"])[0], rtol=1e-6)
    np.random.seed(11)
    x2, f2 = bogp.argmax_restart(crit, space, eval_budget=20_000, optimizer="sweep-device")
    assert x2 == x and f2 == f
    # the model's own moments in the reference's shapes, and the host-sampled sweep over the device's rows
    dev = F.device_of(model)
    rows = F.decode_rows(F.space_columns(space, dev.packed), dev.engine.read_candidates(np.arange(2000)))
    pm, pv = model.predict(rows, eval_MSE=True)
    assert pm.shape == pv.shape == (2000, 2)
    vals, idx, pts = bogp.optim.sweep_topk([crit], rows, 3)
    assert pts[0][0] == rows[int(idx[0, 0])]
    assert np.array_equal(vals[0], crit(rows)[idx[0]])
    with pytest.raises(NotImplementedError, match="EI on a forest with 2 outputs"):
        bogp.EI(model=model, plugin=0.0)(rows[:2])
    dev.engine.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# error returns
# ---------------------------------------------------------------------------------------------------------------------------------
def _tiny(m=2):
    """Two trees of three nodes over two columns, m values a node."""
    v = np.array([0, 1.0, 2.0, 0, 3.0, 5.0])
    return dict(d=2, m=m, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=np.stack([v + k for k in range(m)], axis=1))


def test_error_returns_launch_nothing(eng):
    """Every refusal is a code and a message from the host side of the ABI: no kernel runs (the handle's kernel-time stamp stays
    untouched); afterwards a one-output forest set on the same handle sweeps as before."""
    def refused(fn, *a, **k):
        with pytest.raises(_lib.BogpError) as e:
            fn(*a, **k)
        assert e.value.code in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED) and len(str(e.value)) > 30
        return str(e.value)

    lo, hi = np.array([[-1.0, -1.0]]), np.array([[-0.5, np.inf]])
    assert "bogp_forest_set_multi first" in refused(eng.forest_sweep_ehvi, lo, hi)
    assert eng.forest_outputs() == 0
    one = _tiny(1)
    assert "outside [2, 8]" in refused(eng.forest_set_multi, **one)  # m = 1 at set time
    assert "outside [2, 8]" in refused(eng.forest_set_multi, **_tiny(9))
    assert "child outside" in refused(eng.forest_set_multi, **dict(_tiny(), right=[2, -1, -1, 3, -1, -1]))  # the same validation walk
    bad = _tiny()
    bad["value"][4, 1] = np.nan
    assert "non-finite value" in refused(eng.forest_set_multi, **bad)
    assert eng.forest_info()["T"] == 0
    stamp = eng.last_timing()
    assert stamp["acquisition_ms"] == 0.0 and stamp["n_chunks"] == 0
    eng.forest_set_multi(**_tiny())
    assert eng.forest_outputs() == 2 and eng.forest_info()["leaves"] == 4
    assert "no candidates" in refused(eng.forest_sweep_ehvi, lo, hi)
    eng.upload_candidates(np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.6, 0.3]]))
    # the one-output calls on a forest with several outputs
    assert "2 outputs" in refused(eng.forest_predict)
    assert "2 outputs" in refused(eng.forest_leaves, 0, 2)
    assert "2 outputs" in refused(eng.forest_sweep_topk, [(_lib.ACQ_EI, 0.0)], 0.0, True, 1)
    assert "no committed model" in refused(eng.sweep_ehvi, lo, hi)  # bogp_sweep_ehvi refuses every forest handle
    # m mismatch, cell counts, NaN bounds, k
    assert "m = 3 but the forest has 2 outputs" in refused(eng.forest_sweep_ehvi, np.full((1, 3), -1.0), np.full((1, 3), 0.0))
    assert "cells outside" in refused(eng.forest_sweep_ehvi, np.zeros((0, 2)), np.zeros((0, 2)))
    big = _lib.MAX_EHVI_CELLS + 1
    assert "cells outside" in refused(eng.forest_sweep_ehvi, np.full((big, 2), -1.0), np.zeros((big, 2)))
    assert "NaN" in refused(eng.forest_sweep_ehvi, lo, np.array([[np.nan, 0.0]]))
    assert "not finite" in refused(eng.forest_sweep_ehvi, np.array([[np.nan, -1.0]]), hi)
    assert "below its lower bound" in refused(eng.forest_sweep_ehvi, lo, np.array([[-2.0, 0.0]]))
    assert "outside [1," in refused(eng.forest_sweep_ehvi, lo, hi, k=99)
    assert "outside the 4 candidates" in refused(eng.forest_leaves_multi, 3, 2)
    assert eng.last_timing()["n_chunks"] == 0  # nothing has been launched on this handle so far
    # a Gaussian-process handle, with and without a lift
    e2 = _lib.Engine(0)
    e2.set_train(np.zeros((4, 2)) + np.arange(4)[:, None], np.arange(4.0))
    assert "training set" in refused(e2.forest_set_multi, **_tiny())
    assert "bogp_forest_set_multi first" in refused(e2.forest_sweep_ehvi, lo, hi)
    e2.set_lift(np.eye(2), np.zeros(2), None, -np.ones(2), np.ones(2))
    assert "a lift is set" in refused(e2.forest_sweep_ehvi, lo, hi)
    e2.close()
    # the served calls, by hand: per-tree values (1, 3) / (2, 5) in output 0, one more in output 1
    per_tree = np.array([[1.0, 3.0], [2.0, 5.0], [1.0, 3.0], [2.0, 5.0]])
    mu, mse = eng.forest_predict_multi()
    assert np.array_equal(mu[:, 0], [2.0, 3.5, 2.0, 3.5]) and np.array_equal(mu[:, 1], mu[:, 0] + 1)
    assert np.array_equal(mse[:, 0], np.std(per_tree, axis=1, ddof=1) ** 2.0) and np.array_equal(mse[:, 1], mse[:, 0])
    best, idx = eng.forest_sweep_ehvi(lo, hi, k=6)  # fewer candidates than k: padded
    assert np.array_equal(idx[4:], [-1, -1]) and np.all(np.isneginf(best[4:])) and idx[0] == 1 and idx[1] == 3 and best[0] == best[1]
    # M = 5, k = 8: the ties in index order, three padded ranks
    eng.upload_candidates(np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.6, 0.3], [0.0, 0.0]]))
    best, idx = eng.forest_sweep_ehvi(lo, hi, k=8)
    assert idx.tolist() == [1, 3, 0, 2, 4, -1, -1, -1] and np.all(np.isneginf(best[5:])) and best[0] == best[1] > best[2]
    # M = 257, the maximum in rows 255 and 256 alone (around the boundary of the partial second workgroup): the lower index first
    X257 = np.zeros((257, 2))
    X257[255:] = 1.0
    eng.upload_candidates(X257)
    for k in (1, 2):
        best, idx = eng.forest_sweep_ehvi(lo, hi, k=k)
        assert idx.tolist() == [255, 256][:k] and np.all(best == best[0])
    eng.upload_candidates(np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.6, 0.3]]))  # (the four rows the lines below read)
    # a one-output forest on the same handle sweeps as before, and the multi-output calls refuse it
    t1 = dict(_tiny(1), value=_tiny(1)["value"][:, 0])
    t1.pop("m")
    eng.forest_set(**t1)
    assert eng.forest_outputs() == 1
    mu1, mse1 = eng.forest_predict()
    assert np.array_equal(mu1, mu[:, 0]) and np.array_equal(mse1, mse[:, 0])
    b, i = eng.forest_sweep_topk([(_lib.ACQ_UCB, 0.5)], 0.0, True, 2)
    assert i[0, 0] == 1 and i[0, 1] == 3
    assert "one output" in refused(eng.forest_sweep_ehvi, lo, hi)
    assert "one output" in refused(eng.forest_predict_multi)
