"""The packed regression forest on the device (`bogp_forest_*`, csrc/kernels_forest.hip) against the reference's `RandomForest` as
recorded in tests/golden/G40_forest.npz (tests/support/make_forest_golden.py): per-tree predictions bit for bit, mu / MSE and the five
criteria at the project's standing tolerances, argmax / top 16 exactly (ties included), the mixed candidate generator against its
NumPy restatement (tests/support/philox_mixed.py), the generated sweep end to end, and the ABI's error returns.

Figures measured on an MI355X (this file's parity tests print them; profiles/forest_parity.txt keeps them): see the docstrings."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

from bogp import _lib
from bogp import forest as F
from support import forest_engine as S
from support import philox_mixed

pytestmark = pytest.mark.gpu

PARITY = os.path.join(ROOT, "profiles", "forest_parity.txt")


@pytest.fixture(scope="module")
def g():
    return load_golden("G40_forest")


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
        eng.forest_set(pk.d_raw, pk.tree_offset, f, t, pk.left, pk.right, pk.value, test)
    else:
        eng.forest_set(pk.d_enc, pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value)


def _acq(g):
    return [(int(a), float(p)) for a, p in zip(g["acq_id"], g["acq_par"])]


@pytest.mark.parametrize("raw", [False, True], ids=["encoded", "raw-columns"])
@pytest.mark.parametrize("p", ["mx_", "ds_"])
def test_per_tree_predictions_are_bit_identical(eng, g, p, raw):
    """`bogp_forest_leaves` == `estimators_[t].predict` for the 256 recorded rows, in the forest's own encoded columns and rewritten
    onto the raw columns; the same bits when the rows sit in other lanes and workgroups (other offsets of the launch)."""
    pk = _packed(g, p)
    _set(eng, pk, raw)
    enc = g[p + "Xenc"]
    X = _raw_rows(pk, enc) if raw else enc.astype(np.float64)
    eng.upload_candidates(X)
    want = g[p + "per_tree"]
    got = eng.forest_leaves(0, 256)
    assert np.array_equal(got, want)
    for first, n in ((37, 150), (255, 1), (1, 255)):
        assert np.array_equal(eng.forest_leaves(first, n), want[first : first + n])
    # the rows uploaded at another position of the candidate array
    eng.upload_candidates(np.vstack([X[300:811], X[:256]]))
    assert np.array_equal(eng.forest_leaves(511, 256), want)


def test_thresholds_that_float32_cannot_hold(eng):
    """The packed node keeps the threshold rounded toward -inf to float32; rows one float32 step either side of such thresholds, and
    exactly on representable ones, reach the leaves of the double comparison."""
    rng = np.random.default_rng(5)
    T, d = 4, 3
    off, feat, thr, left, right, val = [0], [], [], [], [], []
    grid = []
    for t in range(T):  # a depth-2 complete tree: 7 nodes
        th = rng.uniform(-3, 3, size=3) * (1 + 1e-9)
        th[1] = float(np.float32(th[1]))  # one representable threshold
        f = rng.integers(0, d, size=3)
        feat += [f[0], f[1], -2, -2, f[2], -2, -2]
        thr += [th[0], th[1], -2, -2, th[2], -2, -2]
        left += [1, 2, -1, -1, 5, -1, -1]
        right += [4, 3, -1, -1, 6, -1, -1]
        val += list(rng.normal(size=7))
        off.append(off[-1] + 7)
        grid += list(th)
    grid = np.asarray(grid)
    f32 = grid.astype(np.float32)
    pts = np.concatenate([f32, np.nextafter(f32, np.float32(-np.inf)), np.nextafter(f32, np.float32(np.inf))]).astype(np.float64)
    X = np.stack(np.meshgrid(pts[::3], pts[1::3], pts[2::3], indexing="ij"), -1).reshape(-1, 3)
    forest = (np.asarray(off), np.asarray(feat), np.asarray(thr, float), np.asarray(left), np.asarray(right), np.asarray(val, float), None)
    assert np.any(grid != f32.astype(np.float64))
    eng.forest_set(d, *forest[:6])
    eng.upload_candidates(X)
    assert np.array_equal(eng.forest_leaves(0, len(X)), S.leaves(forest, X))


def test_moments_match_the_reference(eng, g):
    """mu at rtol 1e-6 / atol 1e-9 (ledger T1), MSE at rtol 1e-6 / atol 1e-12 var(y) (T2), both forests, encoded and raw columns.
    Observed on an MI355X: see profiles/forest_parity.txt (the sequential NumPy restatement is at 2e-15)."""
    lines = []
    for p in ("mx_", "ds_"):
        pk = _packed(g, p)
        for raw in (False, True):
            _set(eng, pk, raw)
            enc = g[p + "Xenc"]
            eng.upload_candidates(_raw_rows(pk, enc) if raw else enc.astype(np.float64))
            mu, mse = eng.forest_predict()
            rmu, rmse = g[p + "mu"], g[p + "mse"]
            e_mu = float(np.max(np.abs(mu - rmu) / np.abs(rmu)))
            pos = rmse > 0
            e_mse = float(np.max(np.abs(mse - rmse)[pos] / rmse[pos]))
            lines.append("%s %s: max rel err mu %.3e, MSE %.3e (rows with MSE > 0: %d of %d; max abs err on the others %.3e)"
                         % (p, "raw" if raw else "encoded", e_mu, e_mse, pos.sum(), len(pos), float(np.max(np.abs(mse - rmse)[~pos], initial=0.0))))
            print(lines[-1])
            np.testing.assert_allclose(mu, rmu, rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(mse, rmse, rtol=1e-6, atol=1e-12 * float(g[p + "var_y"]))
            mu_only, none = eng.forest_predict(eval_MSE=False)
            assert none is None and np.array_equal(mu_only, mu)
    _write_parity("moments", lines)


_SECTIONS = {}


def _write_parity(section, lines):
    """profiles/forest_parity.txt: the figures of this run, one section per parity test."""
    _SECTIONS[section] = lines
    try:
        with open(PARITY, "w") as f:
            f.write("Observed errors of the device forest against tests/golden/G40_forest.npz (tests/test_gpu_forest.py, MI355X)\n")
            for name, ls in _SECTIONS.items():
                f.write("## %s\n%s\n" % (name, "\n".join(ls)))
    except OSError:
        pass


def test_criteria_match_the_reference_classes(eng, g):
    """EI, PI, EpsilonPI, UCB, MGFI at rtol 1e-6 against the reference's own class values on the rows that have them.  EpsilonPI and
    MGFI fall under ledger rule T3 only on rows with reference MSE <= 1e-12 var(y): the fixture has none, the excluded share is zero."""
    lines = []
    for p in ("mx_", "ds_"):
        pk = _packed(g, p)
        _set(eng, pk, True)
        eng.upload_candidates(_raw_rows(pk, g[p + "Xenc"]))
        cls = g[p + "class_values"]
        n = cls.shape[1]
        excluded = g[p + "mse"][:n] <= 1e-12 * float(g[p + "var_y"])
        if p == "mx_":
            assert excluded.mean() == 0.0
        _, _, vals = eng.forest_sweep_topk(_acq(g), float(g[p + "plugin"]), True, 1, return_values=True)
        for c, name in enumerate(g["criteria"]):
            ok = ~excluded if str(name) in ("EpsilonPI", "PI", "MGFI") else np.ones(n, dtype=bool)
            ref, got = cls[c][ok], vals[c][:n][ok]
            nz = ref != 0
            err = float(np.max(np.abs(got - ref)[nz] / np.abs(ref)[nz], initial=0.0))
            lines.append("%s %s: max rel err %.3e over %d rows (%d excluded)" % (p, name, err, ok.sum(), (~ok).sum()))
            print(lines[-1])
            np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0)
    _write_parity("criteria", lines)


@pytest.mark.parametrize("raw", [False, True], ids=["encoded", "raw-columns"])
@pytest.mark.parametrize("p", ["mx_", "ds_"])
def test_argmax_and_top16_are_exact(eng, g, p, raw):
    """Argmax and the 16 best rows of every criterion are those of the reference's moments; on the all-discrete forest the tied
    maximum comes back at its lowest index and tied rows carry identical bits."""
    pk = _packed(g, p)
    _set(eng, pk, raw)
    enc = g[p + "Xenc"]
    eng.upload_candidates(_raw_rows(pk, enc) if raw else enc.astype(np.float64))
    acq = _acq(g)
    best, idx, vals = eng.forest_sweep_topk(acq, float(g[p + "plugin"]), True, 16, return_values=True)
    b1, i1 = eng.forest_sweep_topk(acq, float(g[p + "plugin"]), True, 1)
    for c, name in enumerate(g["criteria"]):
        want = g[p + "top16_" + str(name)]
        assert np.array_equal(idx[c], want), (name, idx[c], want)
        assert i1[c, 0] == want[0] and b1[c, 0] == best[c, 0]
        assert np.array_equal(best[c], vals[c][idx[c]])
        assert int(np.argmax(vals[c])) == want[0]
    if p == "ds_":
        ties = g["ds_ties"]
        assert ties.max() >= 2
        for c in range(len(acq)):
            tied = np.flatnonzero(vals[c] == vals[c].max())
            assert len(tied) == ties[c] and idx[c, 0] == tied[0]
            assert len({vals[c][i].tobytes() for i in tied}) == 1
        # rows that are equal get equal bits in every criterion
        _, first, inv = np.unique(enc, axis=0, return_index=True, return_inverse=True)
        assert np.array_equal(vals.view(np.int64), vals[:, first[inv.ravel()]].view(np.int64))


def test_mixed_generator_matches_its_restatement(eng, g):
    """Every column against tests/support/philox_mixed.py: integers and level indices exact; reals exact on linear columns, rtol 5e-16
    behind a transcendental scale, and within one rounding step where 2 ulp straddle a rounding boundary (the rule of the uniform
    generator's test); shards drawn with first_row equal the rows of the whole design; level frequencies of 1e6 draws within 5 sigma."""
    from oracle import philox as P

    pk = _packed(g, "mx_")
    _set(eng, pk, True)
    d = pk.d_raw
    kind = [0, 0, 0, 0, 1, 1, 1, 1]
    scales = ["linear", "log10", "linear", "log", "linear", "linear", "linear", "linear"]
    precs = [None, None, 2, 3, None, None, None, None]
    lo = np.array([-5.0, 1e-3, -5.0, 0.5, 0.0, -3.0, 0.0, 0.0])
    hi = np.array([5.0, 10.0, 5.0, 50.0, 10.0, 3.0, 4.0, 4.0])
    lo_t = np.array([-5.0, np.log10(1e-3), -5.0, np.log(0.5), 0.0, -3.0, 0.0, 0.0])
    hi_t = np.array([5.0, np.log10(10.0), 5.0, np.log(50.0), 10.0, 3.0, 4.0, 4.0])
    nl = [0, 0, 0, 0, 11, 7, 5, 5]
    M = 20000
    eng.set_candidate_transform(scales, precs, lo, hi)
    eng.generate_candidates_mixed(kind, lo_t, hi_t, nl, M, seed=77, first_row=123)
    got = eng.read_candidates(np.arange(M))
    want = P.transform(philox_mixed.mixed_box(lo_t, hi_t, nl, M, 77, first_row=123), scales, precs, lo, hi)
    for k in range(d):
        assert np.all(got[:, k] >= lo[k]) and np.all(got[:, k] <= hi[k])
        if kind[k] == 1 or (scales[k] == "linear"):
            np.testing.assert_array_equal(got[:, k], want[:, k])
        elif precs[k] is None:
            np.testing.assert_allclose(got[:, k], want[:, k], rtol=5e-16, atol=0)
        else:
            differ = got[:, k] != want[:, k]
            assert differ.mean() < 1e-3 and np.all(np.abs(got[differ, k] - want[differ, k]) <= 10.0 ** -precs[k] * 1.0000001)
    idx = philox_mixed.level_indices(nl, M, 77, first_row=123)
    for k in range(4, 8):
        np.testing.assert_array_equal(got[:, k], lo[k] + idx[:, k])
        assert set(np.unique(idx[:, k])) == set(range(nl[k]))
    # shards
    for first, n in ((123, 1000), (123 + 7001, 999), (123 + 19999, 1)):
        eng.generate_candidates_mixed(kind, lo_t, hi_t, nl, n, seed=77, first_row=first)
        np.testing.assert_array_equal(eng.read_candidates(np.arange(n)), got[first - 123 : first - 123 + n])
    # level frequencies: a count is Binomial(n, 1 / L), sd = sqrt(n (1 / L) (1 - 1 / L)); 5 sd bounds each of the 28 counts
    n = 1_000_000
    eng.set_candidate_transform()
    eng.generate_candidates_mixed(kind, lo_t, hi_t, nl, n, seed=2024)
    big = eng.read_candidates(np.arange(n))
    for k in range(4, 8):
        L = nl[k]
        counts = np.bincount((big[:, k] - lo[k]).astype(np.int64), minlength=L)
        assert len(counts) == L
        sd = np.sqrt(n * (1.0 / L) * (1.0 - 1.0 / L))
        assert np.all(np.abs(counts - n / L) <= 5.0 * sd), (k, counts)
    # one level, and a stepped column: lo + index * (hi - lo) / (L - 1)
    eng.generate_candidates_mixed([1] * 8, [2.0] * 8, [2.0] * 4 + [4.0] * 4, [1] * 4 + [5] * 4, 64, seed=3)
    small = eng.read_candidates(np.arange(64))
    assert np.all(small[:, :4] == 2.0) and set(np.unique(small[:, 4:])) <= {2.0, 2.5, 3.0, 3.5, 4.0}
    np.testing.assert_array_equal(small, philox_mixed.mixed_box([2.0] * 8, [2.0] * 4 + [4.0] * 4, [1] * 4 + [5] * 4, 64, 3))


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


class _Model:  # what forest.pack reads of a fitted forest
    class _Tree:
        pass

    def __init__(self, g, p, labels):
        self.estimators_ = []
        off = g[p + "tree_offset"]
        for t in range(len(off) - 1):
            e, tr = _Model._Tree(), _Model._Tree()
            s = slice(int(off[t]), int(off[t + 1]))
            tr.children_left, tr.children_right, tr.feature = g[p + "left"][s], g[p + "right"][s], g[p + "feature"][s]
            tr.threshold, tr.value = g[p + "threshold"][s], g[p + "value"][s].reshape(-1, 1, 1)
            e.tree_ = tr
            self.estimators_.append(e)
        self.n_outputs_, self.n_features_in_ = 1, int(g[p + "Xenc"].shape[1])
        self._cat_idx = [int(v) for v in g[p + "cat_idx"]]
        self._categories = [list(labels) for _ in self._cat_idx]
        self.y = np.array([float(g[p + "plugin"])])

    def predict(self, X, eval_MSE=False):
        return F.predict(self, X, eval_MSE)


_Model.__name__ = "RandomForest"


def test_generated_sweep_end_to_end(g):
    """`sweep-device` on the mixed forest with M = 1e5: the winner read back through candidates_read, decoded to the reference's row
    format and pushed through the CPU stand-in gives the reported value at rtol 1e-6."""
    import bogp

    labels = ["red", "green", "blue", "cyan", "black"]
    model = _Model(g, "mx_", labels)
    space = _Space([Real((-5.0, 5.0), "r%d" % k) for k in range(4)] + [Integer((0, 10), "i0"), Integer((-3, 3), "i1"),
                                                                     Discrete(labels, "c0"), Discrete(labels, "c1")])
    pk = F.pack(model)
    forest = (pk.tree_offset, pk.feature, pk.threshold, pk.left, pk.right, pk.value, None)
    for name, kw in (("EI", {}), ("MGFI", {"t": 2.0}), ("UCB", {"alpha": 0.5})):
        crit = getattr(bogp, name)(model=model, minimize=True, **kw)
        np.random.seed(11)
        x, f = bogp.argmax_restart(crit, space, eval_budget=100_000, optimizer="sweep-device")
        assert len(x) == 8 and all(isinstance(v, float) for v in x[:4]) and all(isinstance(v, int) for v in x[4:6])
        assert x[6] in labels and x[7] in labels and 0 <= x[4] <= 10 and -3 <= x[5] <= 3
        mu, mse = S.moments(S.leaves(forest, pk.encode([x])))
        from oracle import gp_oracle as O

        want = O.acquisition(crit.acq_id, crit.acq_par(), mu, mse, crit.effective_plugin(), 1e8, True)[0]
        np.testing.assert_allclose(f, want, rtol=1e-6)
        # the host-sampled sweep of the same criterion over the device's own rows agrees on the winner's value
        dev = F.device_of(model)
        rows = F.decode_rows(F.space_columns(space, dev.packed), dev.engine.read_candidates(np.arange(2000)))
        vals, idx, pts = bogp.optim.sweep_topk([crit], rows, 3)
        assert pts[0][0] == rows[int(idx[0, 0])]
        np.testing.assert_allclose(vals[0], crit(rows).ravel()[idx[0]], rtol=0, atol=0)
    F.device_of(model).engine.close()


def _tiny():
    """Two trees of three nodes over two columns."""
    return dict(d=2, tree_offset=[0, 3, 6], feature=[0, -2, -2, 1, -2, -2], threshold=[0.5, -2, -2, 0.25, -2, -2],
                left=[1, -1, -1, 1, -1, -1], right=[2, -1, -1, 2, -1, -1], value=[0, 1.0, 2.0, 0, 3.0, 5.0])


def test_error_returns_launch_nothing(eng):
    """Malformed forests, a discrete column without levels and calls before `bogp_forest_set` return a code and a message; validation
    is on the host side of the ABI, so no kernel runs (the kernel-time stamp of the handle stays untouched)."""
    def refused(fn, *a, **k):
        with pytest.raises(_lib.BogpError) as e:
            fn(*a, **k)
        assert e.value.code in (_lib.ERR_INVALID, _lib.ERR_UNSUPPORTED) and len(str(e.value)) > 30
        return str(e.value)

    assert "bogp_forest_set first" in refused(eng.forest_sweep_topk, [(_lib.ACQ_EI, 0.0)], 0.0, True, 1)
    assert "bogp_forest_set first" in refused(eng.forest_predict)
    eng.d = 2
    assert "d is unknown" in refused(eng.generate_candidates_mixed, [0, 1], [0, 0], [1, 1], [0, 3], 8)
    t = _tiny()
    bad = dict(t, right=[2, -1, -1, 3, -1, -1])
    assert "child outside" in refused(eng.forest_set, **bad)
    bad = dict(t, left=[-4, -1, -1, 1, -1, -1])
    assert "child outside" in refused(eng.forest_set, **bad)
    bad = dict(t, feature=[2, -2, -2, 1, -2, -2])
    assert "feature 2 outside" in refused(eng.forest_set, **bad)
    bad = dict(t, left=[0, -1, -1, 1, -1, -1])  # the root as its own child
    assert "already reached" in refused(eng.forest_set, **bad)
    bad = dict(t, left=[1, -1, -1, 1, -1, -1], right=[1, -1, -1, 2, -1, -1])  # both children the same node
    assert "already reached" in refused(eng.forest_set, **bad)
    one = dict(d=2, tree_offset=[0, 3], feature=[0, -2, -2], threshold=[0.5, -2, -2], left=[1, -1, -1], right=[2, -1, -1], value=[0, 1.0, 2.0])
    assert "T >= 2" in refused(eng.forest_set, **one)
    bad = dict(t, threshold=[np.nan, -2, -2, 0.25, -2, -2])
    assert "NaN threshold" in refused(eng.forest_set, **bad)
    assert eng.forest_info()["T"] == 0  # nothing was accepted
    stamp = eng.last_timing()  # forest calls stamp (kernel time, 1 chunk) after every launch: none has happened on this handle
    assert stamp["acquisition_ms"] == 0.0 and stamp["n_chunks"] == 0
    eng.forest_set(**t)
    assert eng.forest_info()["T"] == 2 and eng.forest_info()["nodes"] == 6
    assert "no candidates" in refused(eng.forest_predict)
    assert eng.last_timing()["n_chunks"] == 0
    assert "n_levels = 0" in refused(eng.generate_candidates_mixed, [0, 1], [0, 0], [1, 1], [0, 0], 8)
    assert "n_levels = -3" in refused(eng.generate_candidates_mixed, [0, 1], [0, 0], [1, 1], [0, -3], 8)
    assert "kind 7" in refused(eng.generate_candidates_mixed, [0, 7], [0, 0], [1, 1], [0, 3], 8)
    eng.upload_candidates(np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.6, 0.3]]))
    mu, mse = eng.forest_predict()
    per_tree = np.array([[1.0, 3.0], [2.0, 5.0], [1.0, 3.0], [2.0, 5.0]])
    assert np.array_equal(mu, [2.0, 3.5, 2.0, 3.5]) and np.array_equal(mse, np.std(per_tree, axis=1, ddof=1) ** 2.0)
    assert "unknown acquisition id" in refused(eng.forest_sweep_topk, [(9, 1.0)], 0.0, True, 1)
    assert "outside [1," in refused(eng.forest_sweep_topk, [(_lib.ACQ_EI, 0.0)], 0.0, True, 99)
    assert "outside the 4 candidates" in refused(eng.forest_leaves, 3, 2)
    # a handle is a Gaussian process or a forest
    assert "holds a forest" in refused(eng.set_train, np.zeros((4, 2)) + np.arange(4)[:, None], np.arange(4.0))
    e2 = _lib.Engine(0)
    e2.set_train(np.zeros((4, 2)) + np.arange(4)[:, None], np.arange(4.0))
    assert "training set" in refused(e2.forest_set, **t)
    e2.close()
    # fewer candidates than k: padded
    best, idx = eng.forest_sweep_topk([(_lib.ACQ_UCB, 0.5)], 0.0, True, 6)
    assert np.array_equal(idx[0, 4:], [-1, -1]) and np.all(np.isneginf(best[0, 4:])) and idx[0, 0] == 1
    # M = 5, k = 8: the ties in index order, three padded ranks
    eng.upload_candidates(np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.6, 0.3], [0.0, 0.0]]))
    best, idx = eng.forest_sweep_topk([(_lib.ACQ_UCB, 0.5)], 0.0, True, 8)
    assert idx[0].tolist() == [1, 3, 0, 2, 4, -1, -1, -1] and np.all(np.isneginf(best[0, 5:])) and best[0, 0] == best[0, 1] > best[0, 2]
    # M = 257, the maximum in rows 255 and 256 alone (around the boundary of the partial second workgroup): the lower index first
    X257 = np.zeros((257, 2))
    X257[255:] = 1.0
    eng.upload_candidates(X257)
    for k in (1, 2):
        best, idx = eng.forest_sweep_topk([(_lib.ACQ_UCB, 0.5)], 0.0, True, k)
        assert idx[0].tolist() == [255, 256][:k] and np.all(best[0] == best[0, 0])
