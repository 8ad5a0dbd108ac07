"""The one-pass pruned sweep (csrc/bogp_api_sweep.hip) on the device: pruning off, the per-chunk path
("chunks") and the automatic mode give identical value bytes and indices, the path the automatic mode took is the one
bogp_prune_decide gives for survivor counts computed on the host with the oracle, and on the one-pass path the rows that went through
the contraction are the pilot plus exactly those survivors -- the pilot's thresholds are all the one-pass flow bounds against within
a segment.  Model and candidates of tests/prune_cases.py: N = 544, d = 3, M = 3001, BOGP_CHUNK_MB=1 -> 192 rows a chunk = the pilot =
the survivor buffer, 2809 rows behind the pilot.  A second segment (more than 2 Mi rows at this N) cannot be reached at test sizes and
no switch was added to fake one: the segment loop runs once here."""
import numpy as np
import pytest

import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
MIX8 = [(EI, 0.0), (PI, 0.05), (UCB, 0.5), (MGFI, 1.0), (MGFI, 2.0), (EI, 0.0), (PI, 0.0), (UCB, 2.0)]
# the improvement criteria leave 28 of this model's 192 pilot rows within reach of the pilot's best (more than an eighth: per-chunk path);
# UCB with a moderate multiplier leaves 1 .. 23, so the placement cases below use it to stay on the one-pass path
UCB2 = [(UCB, 8.0), (UCB, 0.5)]
UCB8 = [(UCB, a) for a in (0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 10.0)]
NONE, CHUNKS, ONEPASS, FALLBACK = (_lib.PRUNE_PATH_NONE, _lib.PRUNE_PATH_CHUNKS, _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK)
PILOT = PC.CHUNK_ROWS


@pytest.fixture(scope="module")
def models():
    out = {}
    for ordinary in (False, True):
        X, y, par, st = PC.model(ordinary)
        eng = _lib.Engine(0)
        eng.set_train(X, y)
        eng.commit(PC.KERNEL, _lib.MODE_NOISY, par, PC.NOISE, ordinary, 0.0)
        out[ordinary] = (eng, X, y, st)
    yield out
    for eng, *_ in out.values():
        eng.close()


@pytest.fixture()
def small_chunks(monkeypatch):
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")


def host_counts(st, Xs, acq, plugin, minimize=True, pilot=PILOT):
    """(survivors among the pilot's rows, survivors behind the pilot) of the prune test against the pilot's own best values, with the
    oracle; the second count is PC.surviving_fraction's."""
    nan = np.isnan(Xs).any(axis=1)  # (the oracle's triangular solve refuses them: no bound exists for such a row, it survives)
    assert not nan[:pilot].any()
    if nan.any():
        Xs = Xs.copy()
        Xs[nan] = Xs[0]
    mu, mse, sd_ub = PC.oracle_rows(st, Xs)
    s2 = float(st.sigma2[0])
    y_hat = mu if minimize else -1 * mu
    keep = nan.copy()
    for a_id, a_par in acq:
        vals = O.acquisition(a_id, a_par, mu, mse, plugin, s2, minimize)
        thr = vals[:pilot][int(np.argmax(vals[:pilot]))]
        b = PC.upper_bounds(a_id, a_par, y_hat, sd_ub, plugin, s2)
        keep |= ~(np.isfinite(thr) & (b + PC.prune_margin(b, thr) < thr))
    behind = int(np.count_nonzero(keep[pilot:]))
    if not nan.any():
        assert behind == int(round(PC.surviving_fraction(st, Xs, acq, plugin, minimize, pilot) * len(Xs)))
    return int(np.count_nonzero(keep[:pilot])), behind


def three(eng, st, Xs, acq, plugin, minimize=True, pilot=PILOT, upload=True, buffer_rows=PC.CHUNK_ROWS):
    """The sweep with pruning off, on the per-chunk path and in the automatic mode: identical bytes and indices; the automatic mode's
    path against the host's decision; on the one-pass path the exact survivor count.  -> (values, indices, path, survivors, rounds)"""
    M = len(Xs)
    if upload:
        eng.upload_candidates(Xs)
    eng.set_prune(False)
    v0, i0 = eng.sweep(acq, plugin, minimize)
    assert eng.last_contracted_rows() == M and eng.last_prune_path() == (NONE, 0, 0)
    eng.set_prune("chunks")
    v2, i2 = eng.sweep(acq, plugin, minimize)
    assert eng.last_prune_path() == (CHUNKS, 0, 0)
    assert v2.tobytes() == v0.tobytes() and np.array_equal(i2, i0), (v0, v2, i0, i2)
    eng.set_prune(True)
    v1, i1 = eng.sweep(acq, plugin, minimize)
    path, surv, rounds = eng.last_prune_path()
    n1 = eng.last_contracted_rows()
    n_pilot, n_behind = host_counts(st, Xs, acq, plugin, minimize, pilot)
    print("M = %d, q = %d: path %d, %d survivors in %d rounds, %d rows contracted; host: %d of the pilot's %d, %d behind it"
          % (M, len(acq), path, surv, rounds, n1, n_pilot, pilot, n_behind))  # fmt: skip
    assert v1.tobytes() == v0.tobytes() and np.array_equal(i1, i0), (v0, v1, i0, i1)
    assert path == _lib.load().bogp_prune_decide(pilot, n_pilot, M - pilot, n_behind)
    if path == ONEPASS:
        assert surv == n_behind and n1 == pilot + n_behind
        assert rounds == (n_behind + buffer_rows - 1) // buffer_rows  # rounds of at most one survivor buffer = one chunk's rows
    elif path == CHUNKS:
        assert (surv, rounds) == (0, 0) and 0 < n1 <= M
    else:
        assert 0 < n1 <= M
    return v1, i1, path, surv, rounds


# survivors behind the pilot with the oracle (simple / ordinary kriging); no row's bound lies within 1e-6 relative of its threshold
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("alpha,expect,rounds", [(0.5, (31, 33), 1), (8.0, (174, 179), 1), (10.0, (252, 252), 2), (15.0, (474, 475), 3)])
def test_ucb_survivors_fill_one_two_and_three_rounds(models, small_chunks, ordinary, alpha, expect, rounds):
    eng, X, y, st = models[ordinary]
    v, i, path, surv, n_rounds = three(eng, st, PC.candidates(), [(UCB, alpha)], float(y.min()))
    assert path == ONEPASS and surv == expect[int(ordinary)] and n_rounds == rounds
    assert eng.last_contracted_rows() == PILOT + surv


@pytest.mark.parametrize("ordinary", [False, True])
def test_ucb_20_and_50_take_the_path_the_pilot_share_decides(models, small_chunks, ordinary):
    eng, X, y, st = models[ordinary]
    Xs = PC.candidates()
    three(eng, st, Xs, [(UCB, 20.0)], float(y.min()))  # 786 of 2809 behind the pilot: more than a quarter, if the pilot lets it get there
    v, i, path, surv, rounds = three(eng, st, Xs, [(UCB, 50.0)], float(y.min()), upload=False)
    assert path == CHUNKS and eng.last_contracted_rows() == PC.M_CAND  # everything survives: the per-chunk path, contracted in place


@pytest.mark.parametrize("ordinary", [False, True])
def test_forced_segment_fall_back(models, small_chunks, ordinary):
    """The pilot holds the winner and the 191 rows with the lowest bounds: one survivor of 192, so the sweep goes on -- into a segment
    of which more than a quarter reaches the winner's value (UCB, alpha = 30).  That segment runs chunk by chunk."""
    eng, X, y, st = models[ordinary]
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
    n_pilot, n_behind = host_counts(st, Xr, acq, pl)
    assert 8 * n_pilot <= PILOT and 4 * n_behind > len(Xs) - PILOT
    v, i, path, surv, rounds = three(eng, st, Xr, acq, pl)
    assert path == FALLBACK and i[0] == 0 and (surv, rounds) == (0, 0)


@pytest.mark.parametrize("ordinary", [False, True])
def test_winner_in_the_pilot_the_middle_and_the_ragged_end(models, small_chunks, ordinary):
    eng, X, y, st = models[ordinary]
    pl = float(y.min())
    Xs = PC.candidates()
    for where in (5, 1500, 2990):  # the pilot, chunk 7, the last chunk (121 rows)
        v, i, path, surv, rounds = three(eng, st, PC.place_winner(st, Xs, UCB2, pl, where), UCB2, pl)
        assert i[0] == where and path == ONEPASS
    acq = [(MGFI, 2.0), (EI, 0.0)]  # (28 of the pilot's 192 rows survive unless it holds the winner: per-chunk path)
    for where in (5, 1500):
        v, i, path, surv, rounds = three(eng, st, PC.place_winner(st, Xs, acq, pl, where), acq, pl)
        assert i[0] == where and path == (ONEPASS if where == 5 else CHUNKS)


def test_duplicate_rows_lowest_index_wins(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    Xw = PC.place_winner(st, PC.candidates(), UCB2, pl, 1500)
    Xw[[700, 2500, 2999]] = Xw[1500]
    v, i, path, surv, rounds = three(eng, st, Xw, UCB2, pl)
    assert i[0] == 700 and path == ONEPASS


def test_nan_row_behind_the_pilot_and_a_candidate_on_a_training_point(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    Xs = PC.candidates()
    Xs[1000] = X[int(np.argmin(y))]  # sd = 0 there: bound and value coincide
    Xs[100] = X[3]                   # ... and one inside the pilot
    v, i, path, surv, rounds = three(eng, st, Xs, UCB2, pl)
    assert path == ONEPASS
    Xs[2000, 1] = np.nan             # no bound exists: the row survives and wins at its index
    v, i, path, surv, rounds = three(eng, st, Xs, UCB2, pl)
    assert np.all(np.isnan(v)) and np.all(i == 2000) and path == ONEPASS
    Xs[300, 0] = np.nan              # ... the first of two
    v, i, path, surv, rounds = three(eng, st, Xs, UCB2, pl)
    assert np.all(i == 300) and path == ONEPASS
    acq = [(EI, 0.0), (PI, 0.0), (UCB, 0.5), (MGFI, 2.0)]  # the guards of EI and MGFI at sd = 0, Phi(+-inf) or 0 / 0 for PI; MGFI maps a NaN to 0
    v, i, path, surv, rounds = three(eng, st, Xs, acq, pl)
    assert np.all(i[:3] == 300) and np.isfinite(v[3]) and i[3] not in (300, 2000)


@pytest.mark.parametrize("ordinary", [False, True])
def test_q8_mix_on_a_ragged_candidate_count(models, small_chunks, ordinary):
    eng, X, y, st = models[ordinary]
    Xs = PC.candidates(seed=8, M=2500 + 37)  # M is no multiple of 64
    three(eng, st, Xs, MIX8, float(y.min()))
    v, i, path, surv, rounds = three(eng, st, Xs, UCB8, float(y.min()), upload=False)
    assert path == ONEPASS and rounds == 1


def test_minimize_false(models, small_chunks):
    eng, X, y, st = models[False]
    three(eng, st, PC.candidates(), [(EI, 0.0), (MGFI, 2.0)], -1.0 * float(y.max()), minimize=False)
    acq = [(UCB, 4.0), (UCB, 0.5)]  # (15 of the pilot's rows, 200 behind it: two rounds)
    v, i, path, surv, rounds = three(eng, st, PC.candidates(), acq, -1.0 * float(y.max()), minimize=False, upload=False)
    assert path == ONEPASS and rounds == 2


def test_one_chunk_stays_per_chunk_and_three_large_chunks_go_one_pass(models, monkeypatch):
    """Chunk 0 larger than the 4096-row pilot.  Without BOGP_CHUNK_MB 6011 rows are ONE chunk: nothing to save, the per-chunk path.
    At 24 MiB 13 005 rows are three chunks of 5760: one pass, pilot 4096, rounds of at most 5760 survivors."""
    eng, X, y, st = models[True]
    pl = float(y.min())
    acq = [(MGFI, 2.0), (EI, 0.0)]
    Xs = PC.place_winner(st, PC.candidates(seed=9, M=6011), acq, pl, 4100)
    eng.upload_candidates(Xs)
    outs = []
    for mode in (False, "chunks", True):
        eng.set_prune(mode)
        outs.append(eng.sweep(acq, pl, True))
        assert eng.last_prune_path() == ((NONE if mode is False else CHUNKS), 0, 0)
    assert all(o[0].tobytes() == outs[0][0].tobytes() and np.array_equal(o[1], outs[0][1]) for o in outs) and outs[0][1][0] == 4100
    monkeypatch.setenv("BOGP_CHUNK_MB", "24")
    M = 13005
    for where in (4000, 4100, M - 3):
        Xs = PC.place_winner(st, PC.candidates(seed=9, M=M), acq, pl, where)
        v, i, path, surv, rounds = three(eng, st, Xs, acq, pl, pilot=4096, buffer_rows=5760)
        assert i[0] == where and path == ONEPASS and rounds == (1 if surv else 0) and eng.last_contracted_rows() == 4096 + surv


def test_queued_sweep_and_exchange_on_the_one_pass_path(models, small_chunks):
    from bogp import distributed

    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = UCB2
    Xs = PC.place_winner(st, PC.candidates(), acq, pl, 2222)
    v, i, path, surv, rounds = three(eng, st, Xs, acq, pl)
    assert path == ONEPASS
    assert distributed.init_engine_comm(eng) == (0, 1)
    assert eng.sweep(acq, pl, True, local_result=False) is None  # nothing comes back: the winners stay on the device
    assert eng.last_prune_path() == (ONEPASS, surv, rounds)
    gv, gi, gx = eng.exchange_argmax(len(acq), 1_000_000, True)
    assert gv.tobytes() == v.tobytes()
    np.testing.assert_array_equal(gi, i + 1_000_000)
    np.testing.assert_array_equal(gx, Xs[i])
    assert eng.last_contracted_rows() == PILOT + surv
    eng.upload_candidates(Xs, lazy=True)  # a lazy upload keeps the per-chunk path and its copy overlap
    assert eng.sweep(acq, pl, True, local_result=False) is None
    assert eng.last_prune_path() == (CHUNKS, 0, 0)
    gv, gi, gx = eng.exchange_argmax(len(acq), 0, True)
    assert gv.tobytes() == v.tobytes() and np.array_equal(gi, i)


def test_two_runs_give_the_same_bytes_and_the_same_survivors(models, small_chunks):
    eng, X, y, st = models[True]
    pl = float(y.min())
    Xs = PC.candidates()
    eng.upload_candidates(Xs)
    eng.set_prune(True)
    runs = []
    for _ in range(2):
        v, i = eng.sweep(UCB8, pl, True)
        runs.append((v.tobytes(), i.tobytes(), eng.last_prune_path(), eng.last_contracted_rows(), eng.last_timing()["n_chunks"]))
    assert runs[0] == runs[1] and runs[0][2][0] == ONEPASS
    assert runs[0][4] == 1 + runs[0][2][2]  # contraction launches: the pilot's and one a round


def test_set_prune_refuses_an_unknown_mode(models):
    eng = models[False][0]
    with pytest.raises(ValueError):
        eng.set_prune("onepass")
    with pytest.raises(_lib.BogpError):
        eng._check(eng._lib.bogp_set_prune(eng._h, 3))
    eng.set_prune(True)
