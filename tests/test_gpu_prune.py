"""The pruned sweep on the device (csrc/kernels_prune.hip): with the option on and off, the same engine and inputs give the same
winners and bit-identical values, over the cases where pruning could go wrong -- the winner in the pilot, in a middle chunk, in
the last (ragged) chunk and behind the pilot inside chunk 0; nothing prunable; ties; a candidate on a training point; a NaN
row; all values underflowing; every criterion and a q = 8 mix; both kriging flavours.  BOGP_CHUNK_MB=1 at N = 544 gives 192 rows a
chunk: 3001 candidates are 16 chunks, the survivor buffer (192 rows) is flushed every fourth chunk and behind the last.  The peaked cases also hold
the device to contracting fewer than half of the rows (tests/test_prune_bounds_host.py shows with the oracle that fewer than a
quarter can reach the pilot's threshold), the runs without pruning to contracting all of them."""
import numpy as np
import pytest

import prune_cases as PC
from bogp import _lib

pytestmark = pytest.mark.gpu

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
MIX8 = [(EI, 0.0), (PI, 0.05), (UCB, 0.5), (MGFI, 1.0), (MGFI, 2.0), (EI, 0.0), (PI, 0.0), (UCB, 2.0)]


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


def both(eng, Xs, acq, plugin, minimize=True):
    """(values, indices, contracted rows) with the pruning on, after checking them against the run with the pruning off."""
    M = len(Xs)
    eng.upload_candidates(Xs)
    eng.set_prune(False)
    v0, i0 = eng.sweep(acq, plugin, minimize)
    assert eng.last_contracted_rows() == M
    eng.set_prune(True)
    v1, i1 = eng.sweep(acq, plugin, minimize)
    n1 = eng.last_contracted_rows()
    print("M = %d, q = %d: %d rows contracted with pruning (%.1f %%)" % (M, len(acq), n1, 100.0 * n1 / M))
    np.testing.assert_array_equal(i1, i0)
    assert v1.tobytes() == v0.tobytes(), (v0, v1)
    assert 0 < n1 <= M
    return v1, i1, n1


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("acq", [[(EI, 0.0)], [(MGFI, 2.0)], [(MGFI, 2.0), (EI, 0.0)]])
def test_peaked_landscape_winner_in_pilot_middle_and_last_chunk(models, small_chunks, ordinary, acq):
    eng, X, y, st = models[ordinary]
    pl = float(y.min())
    Xs = PC.candidates()
    for where in (5, 1500, 2990):  # chunk 0 = the pilot, chunk 7, chunk 15 (121 rows)
        Xw = PC.place_winner(st, Xs, acq, pl, where)
        v, i, n = both(eng, Xw, acq, pl)
        assert i[0] == where
        assert n < len(Xs) // 2


def test_flat_landscape_contracts_everything_in_place(models, small_chunks):
    eng, X, y, st = models[False]
    v, i, n = both(eng, PC.candidates(), [(UCB, 50.0)], float(y.min()))
    assert n == PC.M_CAND


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("acq", [[(EI, 0.0)], [(PI, 0.05)], [(PI, 0.0)], [(UCB, 0.5)], [(MGFI, 2.0)], [(MGFI, 30.0)], MIX8])
def test_each_criterion_and_a_mix(models, small_chunks, ordinary, acq):
    eng, X, y, st = models[ordinary]
    both(eng, PC.candidates(seed=8, M=2500 + 37), acq, float(y.min()))  # M is no multiple of 64


def test_ucb_with_a_negative_multiplier_is_refused_either_way(models, small_chunks):
    """bogp_sweep validates alpha > 0 (the reference asserts it) before any kernel runs: the option changes nothing about that.
    (The bound's par < 0 branch is held to the oracle on the host, tests/test_prune_bounds_host.py.)"""
    eng, X, y, st = models[False]
    eng.upload_candidates(PC.candidates(M=500))
    msgs = []
    for on in (False, True):
        eng.set_prune(on)
        with pytest.raises(_lib.BogpError) as e:
            eng.sweep([(UCB, -0.5)], float(y.min()), True)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


def test_minimize_false(models, small_chunks):
    eng, X, y, st = models[False]
    both(eng, PC.candidates(), [(EI, 0.0), (MGFI, 2.0)], -1.0 * float(y.max()), minimize=False)


def test_duplicate_rows_lowest_index_wins(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = [(EI, 0.0), (MGFI, 2.0)]
    Xw = PC.place_winner(st, PC.candidates(), acq, pl, 1500)
    Xw[[700, 2500, 2999]] = Xw[1500]
    v, i, n = both(eng, Xw, acq, pl)
    assert i[0] == 700


def test_candidate_on_a_training_point_and_nan_row(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = [(EI, 0.0), (PI, 0.0), (UCB, 0.5), (MGFI, 2.0)]
    Xs = PC.candidates()
    Xs[1000] = X[int(np.argmin(y))]  # sd = 0 there: the guards of EI and MGFI, Phi(+-inf) or 0 / 0 for PI
    Xs[100] = X[3]                   # ... and one inside the pilot
    both(eng, Xs, acq, pl)
    Xs[2000, 1] = np.nan             # a NaN row wins EI, PI and UCB at its index (MGFI maps a non-finite value to 0: its winner stays)
    v, i, n = both(eng, Xs, acq, pl)
    assert np.all(np.isnan(v[:3])) and np.all(i[:3] == 2000) and np.isfinite(v[3]) and i[3] != 2000
    Xs[300, 0] = np.nan              # ... the first of two
    v, i, n = both(eng, Xs, acq, pl)
    assert np.all(i[:3] == 300)


def test_all_underflow_ei_index_zero_wins(models, small_chunks):
    eng, X, y, st = models[False]
    v, i, n = both(eng, PC.candidates(), [(EI, 0.0)], -1.0e3)
    assert v[0] == 0.0 and i[0] == 0
    assert n == PC.M_CAND  # a zero threshold prunes nothing


@pytest.mark.parametrize("chunk_mb,M", [(None, 6000 + 11), (24, 13000 + 5)])
def test_pilot_inside_a_larger_chunk_zero(models, monkeypatch, chunk_mb, M):
    """Chunks larger than the 4096-row pilot: the rest of chunk 0 is bounded against the pilot's thresholds (one chunk of 6011 rows;
    three chunks of 5760 rows at 24 MiB), the winner in the pilot, right behind it, and in the last chunk."""
    eng, X, y, st = models[True]
    if chunk_mb:
        monkeypatch.setenv("BOGP_CHUNK_MB", str(chunk_mb))
    pl = float(y.min())
    acq = [(MGFI, 2.0), (EI, 0.0)]
    Xs = PC.candidates(seed=9, M=M)
    for where in (4000, 4100, M - 3):
        Xw = PC.place_winner(st, Xs, acq, pl, where)
        v, i, n = both(eng, Xw, acq, pl)
        assert i[0] == where and n < M


def test_queued_sweep_and_exchange(models, small_chunks):
    from bogp import distributed

    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = [(MGFI, 2.0), (EI, 0.0)]
    Xs = PC.place_winner(st, PC.candidates(), acq, pl, 2222)
    v, i, n = both(eng, Xs, acq, pl)
    assert distributed.init_engine_comm(eng) == (0, 1)
    assert eng.sweep(acq, pl, True, local_result=False) is None
    gv, gi, gx = eng.exchange_argmax(len(acq), 1_000_000, True)
    assert gv.tobytes() == v.tobytes()
    np.testing.assert_array_equal(gi, i + 1_000_000)
    np.testing.assert_array_equal(gx, Xs[i])
    assert eng.last_contracted_rows() == n
    eng.upload_candidates(Xs, lazy=True)  # the lazy upload feeds the same chunks
    assert eng.sweep(acq, pl, True, local_result=False) is None
    gv, gi, gx = eng.exchange_argmax(len(acq), 0, True)
    assert gv.tobytes() == v.tobytes() and np.array_equal(gi, i)


def test_value_outputs_never_prune(models, small_chunks):
    """sweep_topk, sweep(return_values=True) and predict with the option on: every row is contracted, the outputs are those of the
    option off."""
    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = [(MGFI, 2.0), (EI, 0.0)]
    Xs = PC.candidates()
    eng.upload_candidates(Xs)
    out = {}
    for on in (False, True):
        eng.set_prune(on)
        tv, ti = eng.sweep_topk(acq, pl, True, 5)
        assert eng.last_contracted_rows() == len(Xs)
        bv, bi, vals = eng.sweep(acq, pl, True, return_values=True)
        assert eng.last_contracted_rows() == len(Xs)
        mu, mse = eng.predict()
        assert eng.last_contracted_rows() == len(Xs)
        out[on] = (tv, ti, bv, bi, vals, mu, mse)
    for a, b in zip(out[False], out[True]):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    eng.set_prune(True)
    v, i = eng.sweep(acq, pl, True)  # ... and the pruned winners are the first rank of the top-k
    assert v.tobytes() == out[True][0][:, 0].tobytes() and np.array_equal(i, out[True][1][:, 0])
