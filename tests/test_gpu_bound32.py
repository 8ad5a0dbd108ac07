"""The FP32 bounding stage of the one-pass pruned sweep on the device (csrc/kernels_bound32.hip): with
the stage on and off the sweep returns the same bytes, indices, path, survivors, rounds and contracted rows; the per-row sums it
reads back lie within their margins of the oracle's; and bogp_last_bound32 shows the route -- the exact stage on S1 alone, the exact
pass over the whole segment where S1 is more than a quarter of it, nothing where the stage does not apply.  Shapes of
tests/prune_cases.py: N = 544, d = 3, M = 3001, BOGP_CHUNK_MB=1 -> 192 rows a chunk = the pilot, 2809 rows behind it."""
import numpy as np
import pytest

import bound32_cases as BC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
NONE, CHUNKS, ONEPASS, FALLBACK = (_lib.PRUNE_PATH_NONE, _lib.PRUNE_PATH_CHUNKS, _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK)
PILOT = PC.CHUNK_ROWS
BEHIND = PC.M_CAND - PILOT
UCB2 = [(UCB, 8.0), (UCB, 0.5)]
KERNELS = [O.KERNEL_SE, O.KERNEL_MATERN32, O.KERNEL_MATERN52]


@pytest.fixture(scope="module")
def models():
    """engine and oracle state per (kernel, ordinary), built on first use"""
    cache = {}

    def get(kernel, ordinary, **kw):
        key = (kernel, ordinary, tuple(sorted(kw.items())))
        if key not in cache:
            X, y, par, st = BC.model(kernel, ordinary, **kw)
            eng = _lib.Engine(0)
            eng.set_train(X, y)
            eng.commit(kernel, _lib.MODE_NOISY, par, kw.get("nugget", PC.NOISE), ordinary, 0.0)
            cache[key] = (eng, X, y, st)
        return cache[key]

    yield get
    for eng, *_ in cache.values():
        eng.close()


@pytest.fixture()
def small_chunks(monkeypatch):
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")


def on_off(eng, Xs, acq, plugin, minimize=True, upload=True):
    """the sweep with the stage off, then on: everything the caller sees is identical -> (values, indices, path, survivors, rounds,
    (rows bounded in FP32, rows kept, segments that fell back))"""
    if upload:
        eng.upload_candidates(Xs)
    eng.set_prune(True)
    eng.set_prune_bound32(False)
    v0, i0 = eng.sweep(acq, plugin, minimize)
    p0, n0 = eng.last_prune_path(), eng.last_contracted_rows()
    assert eng.last_bound32() == (0, 0, 0)
    eng.set_prune_bound32(True)
    v1, i1 = eng.sweep(acq, plugin, minimize)
    p1, n1, rep = eng.last_prune_path(), eng.last_contracted_rows(), eng.last_bound32()
    print("path %s, %d rows contracted; FP32 stage: %s" % (p1, n1, rep))
    assert v1.tobytes() == v0.tobytes() and np.array_equal(i1, i0), (v0, v1, i0, i1)
    assert p1 == p0 and n1 == n0
    return v1, i1, p1[0], p1[1], p1[2], rep


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("minimize", [True, False])
def test_on_and_off_are_identical(models, small_chunks, kernel, ordinary, minimize):
    """(the oracle's counts: UCB2 leaves 12 of the pilot's rows when minimising -- one pass -- and 28 .. 32 when maximising -- the
    per-chunk path, where the stage does not run; UCB 0.5 leaves 1 either way)"""
    eng, X, y, st = models(kernel, ordinary)
    pl = float(y.min()) if minimize else -1.0 * float(y.max())
    Xs = PC.candidates()
    v, i, path, surv, rounds, rep = on_off(eng, Xs, UCB2, pl, minimize)
    assert (path == ONEPASS and rep[0] == BEHIND and rep[1] >= surv) if minimize else (path == CHUNKS and rep == (0, 0, 0))
    v, i, path, surv, rounds, rep = on_off(eng, Xs, [(UCB, 0.5)], pl, minimize, upload=False)
    assert path == ONEPASS and rep[0] == BEHIND and rep[1] >= surv and rep[2] == 0
    if kernel == O.KERNEL_MATERN52:
        v, i, path, surv, rounds, rep = on_off(eng, Xs, [(MGFI, 2.0), (EI, 0.0)], pl, minimize, upload=False)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ordinary", [False, True])
def test_read_back_lies_within_the_margins_of_the_oracle(models, small_chunks, kernel, ordinary):
    eng, X, y, st = models(kernel, ordinary)
    Xs = PC.candidates()
    Xs[700] = X[17]            # a training point itself, a point 1e-4 from one, a box corner, a row at 1e3
    Xs[701] = X[40] + 1e-4 / np.sqrt(3)
    Xs[702] = [5.0, -5.0, 5.0]
    Xs[703] = 1e3
    eng.upload_candidates(Xs)
    eng.set_prune(True)
    eng.set_prune_bound32(True)
    eng.sweep([(UCB, 0.5)], float(y.min()), True)
    path, surv, rounds = eng.last_prune_path()
    rows, kept, fb = eng.last_bound32()
    assert path == ONEPASS and (rows, fb) == (BEHIND, 0)
    mu32, e_mu, wd32, e_w, flags = eng.debug_bound32()
    assert len(mu32) == BEHIND and int(flags.sum()) == kept >= surv
    g, w = BC.vectors(st)
    with np.errstate(all="ignore"):
        r = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs[PILOT:], st.X)).reshape(BEHIND, -1)
    err_mu, err_w = np.abs(mu32 - r.dot(g)), np.abs(wd32 - r.dot(w))
    print("kernel %d ordinary %d: E_mu %.3g .. %.3g, max error %.3g, smallest margin / error %.3g; %d kept, %d survive"
          % (kernel, ordinary, e_mu.min(), np.sort(e_mu)[-2], err_mu.max(), (e_mu / np.maximum(err_mu, 1e-300)).min(), kept, surv))  # fmt: skip
    assert np.all(err_mu <= e_mu) and np.all(err_w <= e_w)
    # the margins are the host function's at the row's squared norm
    na = ((Xs[PILOT:] * np.sqrt(st.theta)) ** 2).sum(axis=1)
    nb_max = float(((X * np.sqrt(st.theta)) ** 2).sum(axis=1).max())
    h_mu, h_w = BC.margins(kernel, 3, na, nb_max, float(np.abs(g).sum()), float(np.abs(w).sum()))
    np.testing.assert_allclose(e_mu, h_mu, rtol=1e-8)
    np.testing.assert_allclose(e_w, h_w, rtol=1e-8)
    # every row the exact test keeps is flagged
    f32, f64 = BC.stage1_flags(st, Xs, [(UCB, 0.5)], float(y.min()))
    assert not np.any(f64[PILOT:] & (flags == 0))


@pytest.mark.parametrize("ordinary", [False, True])
def test_route_exact_stage_on_s1_alone(models, small_chunks, ordinary):
    eng, X, y, st = models(O.KERNEL_MATERN52, ordinary)
    Xs = PC.candidates()
    for k, alpha in enumerate((0.5, 8.0)):
        v, i, path, surv, rounds, rep = on_off(eng, Xs, [(UCB, alpha)], float(y.min()), upload=k == 0)
        assert path == ONEPASS and rep[0] == BEHIND and rep[2] == 0 and surv <= rep[1] and 4 * rep[1] <= BEHIND
        assert surv == int(round(PC.surviving_fraction(st, Xs, [(UCB, alpha)], float(y.min())) * len(Xs)))


@pytest.mark.parametrize("ordinary", [False, True])
def test_route_exact_segment_pass_where_s1_is_more_than_a_quarter(models, small_chunks, ordinary):
    """tests/test_gpu_prune_onepass.py's forced fall-back: the pilot holds the winner and the 191 rows with the lowest bounds, and more
    than a quarter of the segment reaches the winner's value with the reference's own bound (UCB, alpha = 30) -- so S1, a superset,
    is more than a quarter too: the FP32 pass is wasted, the exact pass runs over the whole segment and decides as ever."""
    eng, X, y, st = models(O.KERNEL_MATERN52, ordinary)
    pl = float(y.min())
    acq = [(UCB, 30.0)]
    Xs = PC.candidates()
    mu, mse, sd_ub = PC.oracle_rows(st, Xs)
    s2 = float(st.sigma2[0])
    w = int(np.argmax(O.acquisition(UCB, 30.0, mu, mse, pl, s2, True)))
    b = PC.upper_bounds(UCB, 30.0, mu, sd_ub, pl, s2)
    low = [int(r) for r in np.argsort(b, kind="stable") if r != w][: PILOT - 1]
    head = np.array([w] + low)
    Xr = Xs[np.r_[head, np.setdiff1d(np.arange(len(Xs)), head)]]
    f32, f64 = BC.stage1_flags(st, Xr, acq, pl)
    assert 8 * int(f64[:PILOT].sum()) <= PILOT and 4 * int(f64[PILOT:].sum()) > BEHIND and 4 * int(f32[PILOT:].sum()) > BEHIND
    v, i, path, surv, rounds, rep = on_off(eng, Xr, acq, pl)
    assert path == FALLBACK and i[0] == 0 and rep[0] == BEHIND and 4 * rep[1] > BEHIND and rep[2] == 1


def test_nothing_is_bounded_in_fp32_where_the_stage_does_not_apply(models, small_chunks, monkeypatch):
    Xs = PC.candidates()
    eng, X, y, st = models(O.KERNEL_MATERN12, False)  # no bounded slope in the squared distance
    v, i, path, surv, rounds, rep = on_off(eng, Xs, [(UCB, 0.5)], float(y.min()))
    assert rep == (0, 0, 0) and path != NONE
    eng, X, y, st = models(O.KERNEL_MATERN52, False)
    eng.set_prune_bound32(True)
    eng.upload_candidates(Xs, lazy=True)               # a lazy upload keeps the per-chunk path
    eng.sweep([(UCB, 0.5)], float(y.min()), True)
    assert eng.last_prune_path()[0] == CHUNKS and eng.last_bound32() == (0, 0, 0)
    monkeypatch.delenv("BOGP_CHUNK_MB")                # one chunk: nothing to save
    eng.upload_candidates(Xs)
    eng.sweep([(UCB, 0.5)], float(y.min()), True)
    assert eng.last_prune_path()[0] == CHUNKS and eng.last_bound32() == (0, 0, 0)
    assert len(eng.debug_bound32()[0]) == 0
    with pytest.raises(_lib.BogpError):
        eng._check(eng._lib.bogp_set_prune_bound32(eng._h, 2))


def test_nan_inf_and_huge_rows_behind_the_pilot(models, small_chunks):
    eng, X, y, st = models(O.KERNEL_MATERN52, True)
    pl = float(y.min())
    Xs = PC.candidates()
    Xs[2500, 0] = 1e200   # overflows FP32: the stage cannot bound the row, the exact stage decides
    v, i, path, surv, rounds, rep = on_off(eng, Xs, UCB2, pl)
    assert path == ONEPASS and rep[1] >= 1
    flags = eng.debug_bound32()[4]
    assert flags[2500 - PILOT] == 1
    Xs[1200, 2] = np.inf
    v, i, path, surv, rounds, rep = on_off(eng, Xs, UCB2, pl)
    assert eng.debug_bound32()[4][1200 - PILOT] == 1
    Xs[2000, 1] = np.nan  # no bound exists: the row survives and wins at its index
    v, i, path, surv, rounds, rep = on_off(eng, Xs, UCB2, pl)
    assert eng.debug_bound32()[4][2000 - PILOT] == 1
    v, i, path, surv, rounds, rep = on_off(eng, Xs, [(EI, 0.0), (PI, 0.0), (UCB, 0.5), (MGFI, 2.0)], pl, upload=False)


def test_a_margin_wider_than_the_means_range_still_agrees(models, small_chunks):
    """Squared exponential, theta = 0.01, nugget 1e-10: |gamma|_1 = 1.7e6, so that every row's E_mu (6.8 at least) exceeds the whole
    range of the posterior mean (5.3): the stage rules nothing out with UCB, and the exact pass decides as ever."""
    X, y, par, st = BC.model(O.KERNEL_SE, True, nugget=1e-10)
    par = np.r_[np.full(3, 0.01), 0.01]
    st = O.make_state(par, X, y, O.KERNEL_SE, O.MODE_NOISY, 1e-10, estimate_trend=True)
    eng = _lib.Engine(0)
    try:
        eng.set_train(X, y)
        eng.commit(O.KERNEL_SE, _lib.MODE_NOISY, par, 1e-10, True, 0.0)
        Xs = PC.candidates()
        v, i, path, surv, rounds, rep = on_off(eng, Xs, [(UCB, 0.5)], float(y.min()))
        mu = PC.oracle_rows(st, Xs)[0]
        if rep[0]:
            e_mu = eng.debug_bound32()[1]
            print("E_mu >= %.3g, range of the mean %.3g; kept %d of %d" % (e_mu.min(), np.ptp(mu), rep[1], rep[0]))
            assert e_mu.min() > np.ptp(mu) and rep[1] == rep[0] and rep[2] == 1
        assert rep[0] in (0, BEHIND)
    finally:
        eng.close()


def test_two_runs_give_the_same_bytes_and_the_same_report(models, small_chunks):
    eng, X, y, st = models(O.KERNEL_MATERN52, True)
    eng.upload_candidates(PC.candidates())
    eng.set_prune(True)
    eng.set_prune_bound32(True)
    runs = []
    for _ in range(2):
        v, i = eng.sweep(UCB2, float(y.min()), True)
        dbg = eng.debug_bound32()
        runs.append((v.tobytes(), i.tobytes(), eng.last_prune_path(), eng.last_contracted_rows(), eng.last_bound32(), tuple(a.tobytes() for a in dbg)))
    assert runs[0] == runs[1] and runs[0][2][0] == ONEPASS and runs[0][4][0] == BEHIND
