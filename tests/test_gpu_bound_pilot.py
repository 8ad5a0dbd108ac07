"""The best-bound pilot of the one-pass pruned sweep (csrc/bogp_api_sweep.hip, csrc/kernels_bound32.hip) on the
device: pruning off, the first-rows pilot (mode 0) and the best-bound pilot (mode 2) give identical value bytes and indices; the pilot
read back is sorted, unique and holds at most one row per block and criterion -- for every block and criterion a row whose FP32 interval
bound, recomputed on the host from the stage's own sums and margins, is the block's largest; the rows that went through the contraction
are the pilot plus exactly the survivors the host counts against the thresholds that pilot sets.

Model and candidates of tests/prune_cases.py: N = 544, d = 3, M = 3001, BOGP_CHUNK_MB=1 -> 192 rows a chunk = the survivor buffer.  Blocks
of 256 and 512 rows: 12 and 6 blocks, the last one ragged.  A second segment (more than 2 Mi rows at this N) cannot be reached at test
sizes and no switch was added to fake one: the segment loop runs once here, and the automatic mode's threshold of 262144 rows is seen
only from below."""
import time

import numpy as np
import pytest

import bound_pilot_cases as BP
import prune_cases as PC
from bogp import _lib

pytestmark = pytest.mark.gpu

UCB = BP.UCB
NONE, CHUNKS, ONEPASS, FALLBACK = (_lib.PRUNE_PATH_NONE, _lib.PRUNE_PATH_CHUNKS, _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK)
FIRST_ROWS, BEST_BOUND = _lib.PRUNE_PILOT_FIRST_ROWS, _lib.PRUNE_PILOT_BEST_BOUND
M = PC.M_CAND


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


def check_pilot(pilot, q, block_rows, n_rows=M):
    blocks = (n_rows + block_rows - 1) // block_rows
    assert np.all(np.diff(pilot) > 0) and pilot[0] >= 0 and pilot[-1] < n_rows  # sorted, unique, in range
    per_block = np.bincount(pilot // block_rows, minlength=blocks)
    assert len(per_block) == blocks and per_block.min() >= 1 and per_block.max() <= q and len(pilot) <= q * blocks


def check_pilot_holds_the_best_fp32_bounds(eng, st, acq, plugin, minimize, pilot, block_rows):
    """Simple kriging (u = 0): the device's interval bound of every row from the sums and margins it reports, through the library's host
    wrapper.  Per block and criterion the pilot holds a row that attains the block's largest bound (to 1e-12: host and device round
    erf and exp differently) and no row in front of the first such row does."""
    lib = _lib.load()
    mu32, e_mu, wd32, e_w, flags = eng.debug_bound32()
    assert len(mu32) == M and not st.estimate_trend
    s2 = float(st.sigma2[0])
    mu = float(np.ravel(st.beta)[0]) + mu32
    y_hat = mu if minimize else -1 * mu
    e_y = e_mu + 1e-15 * np.abs(mu)
    sd_ub = np.sqrt(s2) * (1.0 + 1e-12)
    chosen = set(pilot.tolist())
    for a_id, a_par in acq:
        b = np.array([lib.bogp_acq_upper_bound_interval(int(a_id), float(a_par), float(v), float(e), float(sd_ub), float(plugin), s2) for v, e in zip(y_hat, e_y)])
        for b0 in range(0, M, block_rows):
            blk = b[b0 : b0 + block_rows]
            top = blk.max()
            best = [b0 + int(k) for k in np.flatnonzero(blk >= top - 1e-12 * abs(top))] if np.isfinite(top) else [b0 + int(np.argmax(blk))]
            assert chosen & set(best), (a_id, a_par, b0, best)


def sweep_three(eng, Xs, acq, plugin, minimize, block_rows, upload=True):
    """pruning off, mode 0, mode 2: identical bytes and indices -> (values, indices) and the engine left behind mode 2's sweep"""
    if upload:
        eng.upload_candidates(Xs)
    eng.set_prune(False)
    v0, i0 = eng.sweep(acq, plugin, minimize)
    assert eng.last_prune_pilot()[0] == _lib.PRUNE_PILOT_NONE
    eng.set_prune(True)
    eng.set_prune_pilot(0)
    v1, i1 = eng.sweep(acq, plugin, minimize)
    kind, idx = eng.last_prune_pilot()
    assert kind == FIRST_ROWS and np.array_equal(idx, np.arange(PC.CHUNK_ROWS))
    eng.set_prune_pilot(2, block_rows)
    v2, i2 = eng.sweep(acq, plugin, minimize)
    assert v1.tobytes() == v0.tobytes() and np.array_equal(i1, i0), (v0, v1, i0, i1)
    assert v2.tobytes() == v0.tobytes() and np.array_equal(i2, i0), (v0, v2, i0, i2)
    return v2, i2


def counted(eng, st, Xs, acq, plugin, minimize, block_rows):
    """behind sweep_three: the pilot is what the flow says, and on the one-pass path the contracted rows are the pilot's plus the host's count"""
    kind, pilot = eng.last_prune_pilot()
    path, surv, rounds = eng.last_prune_path()
    n = eng.last_contracted_rows()
    rows32, kept32, wasted = eng.last_bound32()
    assert kind == BEST_BOUND and rows32 == M
    check_pilot(pilot, len(acq), block_rows)
    vals, bounds, nan = BP.rows_view(st, Xs, acq, plugin, minimize)
    host, gap = BP.survivors_behind(vals, bounds, nan, pilot)
    print("q = %d, B = %d: pilot %d rows, |S1| = %d, path %d, %d survivors in %d rounds, %d rows contracted; host: %d survivors, smallest distance %.3g"
          % (len(acq), block_rows, len(pilot), kept32, path, surv, rounds, n, host, gap))  # fmt: skip
    return pilot, path, surv, rounds, n, host, gap, wasted


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("block_rows", BP.BLOCKS)
@pytest.mark.parametrize("name,acq,minimize", BP.CRITERIA)
def test_same_bytes_and_the_survivors_the_host_counts(models, small_chunks, ordinary, block_rows, name, acq, minimize):
    eng, X, y, st = models[ordinary]
    Xs, pl = PC.candidates(), BP.plugin_of(y, minimize)
    sweep_three(eng, Xs, acq, pl, minimize, block_rows)
    pilot, path, surv, rounds, n, host, gap, wasted = counted(eng, st, Xs, acq, pl, minimize, block_rows)
    if name == "MIX8":  # (bounds equal to a threshold: bytes, indices and the pilot's shape alone)
        return
    assert gap > BP.GAP
    assert path == ONEPASS and wasted == 0 and surv == host and n == len(pilot) + host
    assert rounds == (host + PC.CHUNK_ROWS - 1) // PC.CHUNK_ROWS
    assert eng.last_timing()["n_chunks"] == 1 + rounds  # contraction launches: the pilot's and one a round
    if not ordinary:
        check_pilot_holds_the_best_fp32_bounds(eng, st, acq, pl, minimize, pilot, block_rows)


@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("block_rows", BP.BLOCKS)
def test_winner_in_the_first_block_the_middle_and_the_ragged_end(models, small_chunks, ordinary, block_rows):
    eng, X, y, st = models[ordinary]
    pl = float(y.min())
    for acq in (BP.UCB2, [(BP.MGFI, 2.0), (BP.EI, 0.0)]):
        for where in BP.PLACES:
            Xs = PC.place_winner(st, PC.candidates(), acq, pl, where)
            v, i = sweep_three(eng, Xs, acq, pl, True, block_rows)
            pilot, path, surv, rounds, n, host, gap, wasted = counted(eng, st, Xs, acq, pl, True, block_rows)
            assert i[0] == where and gap > BP.GAP and path == ONEPASS and surv == host and n == len(pilot) + host


def test_duplicate_rows_lowest_index_wins(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    Xw = PC.place_winner(st, PC.candidates(), BP.UCB2, pl, 1500)
    Xw[[700, 1400, 2500, 2999]] = Xw[1500]  # (1400 and 1500 share a block of 256 and of 512: the pilot takes the first of equal bounds)
    for block_rows in BP.BLOCKS:
        v, i = sweep_three(eng, Xw, BP.UCB2, pl, True, block_rows)
        pilot, path, surv, rounds, n, host, gap, wasted = counted(eng, st, Xw, BP.UCB2, pl, True, block_rows)
        assert i[0] == 700 and path == ONEPASS and surv == host and n == len(pilot) + host
        assert 1500 not in pilot  # (row 1400 has its bounds, bit for bit, and comes first)


def test_a_nan_row_and_a_candidate_on_a_training_point(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    Xs = PC.candidates()
    Xs[1000] = X[int(np.argmin(y))]  # sd = 0 there: the exact value is far below the bound
    Xs[100] = X[3]
    v, i = sweep_three(eng, Xs, BP.UCB2, pl, True, 256)
    pilot, path, surv, rounds, n, host, gap, wasted = counted(eng, st, Xs, BP.UCB2, pl, True, 256)
    assert path == ONEPASS and surv == host and n == len(pilot) + host
    Xs[2000, 1] = np.nan  # no bound exists: the row leads its block's pilot, wins, and its NaN threshold prunes nothing
    for block_rows in BP.BLOCKS:
        v, i = sweep_three(eng, Xs, BP.UCB2, pl, True, block_rows)
        kind, pilot = eng.last_prune_pilot()
        assert np.all(np.isnan(v)) and np.all(i == 2000) and kind == BEST_BOUND and 2000 in pilot
        check_pilot(pilot, 2, block_rows)
        assert eng.last_prune_path()[0] == FALLBACK and eng.last_bound32()[2] == 1  # everything survives a NaN threshold
    Xs[300, 0] = np.nan  # ... the first of two
    acq = [(BP.EI, 0.0), (BP.PI, 0.0), (UCB, 0.5), (BP.MGFI, 2.0)]  # MGFI maps a NaN to 0: its winner is an ordinary row
    v, i = sweep_three(eng, Xs, acq, pl, True, 512)
    assert np.all(i[:3] == 300) and np.isfinite(v[3]) and i[3] not in (300, 2000)


@pytest.mark.parametrize("ordinary", [False, True])
def test_everything_survives_the_segment_falls_back(models, small_chunks, ordinary):
    """UCB with multiplier 50 is within reach of every row (prune_cases.model): the FP32 pass keeps more than a quarter -- wasted, and
    counted as such --, so does the exact pass, and the segment runs chunk by chunk behind the pilot with the same bytes."""
    eng, X, y, st = models[ordinary]
    acq, pl = [(UCB, 50.0)], float(y.min())
    sweep_three(eng, PC.candidates(), acq, pl, True, 256)
    kind, pilot = eng.last_prune_pilot()
    path, surv, rounds = eng.last_prune_path()
    rows32, kept32, wasted = eng.last_bound32()
    check_pilot(pilot, 1, 256)
    assert kind == BEST_BOUND and path == FALLBACK and (surv, rounds) == (0, 0)
    assert (rows32, wasted) == (M, 1) and 4 * kept32 > M
    assert eng.last_contracted_rows() == M + len(pilot)  # every row in place, the pilot's rows once before


def test_two_runs_give_the_same_bytes_pilot_and_counts(models, small_chunks):
    eng, X, y, st = models[True]
    pl = float(y.min())
    eng.upload_candidates(PC.candidates())
    eng.set_prune(True)
    eng.set_prune_pilot(2, 512)
    runs = []
    for _ in range(2):
        v, i = eng.sweep(BP.MIX8, pl, True)
        kind, pilot = eng.last_prune_pilot()
        runs.append((v.tobytes(), i.tobytes(), kind, pilot.tobytes(), eng.last_prune_path(), eng.last_contracted_rows(), eng.last_bound32(),
                     eng.last_timing()["n_chunks"]))  # fmt: skip
    assert runs[0] == runs[1] and runs[0][2] == BEST_BOUND


def test_queued_sweep_and_exchange(models, small_chunks):
    from bogp import distributed

    eng, X, y, st = models[False]
    pl = float(y.min())
    acq = BP.UCB2
    Xs = PC.place_winner(st, PC.candidates(), acq, pl, 2222)
    v, i = sweep_three(eng, Xs, acq, pl, True, 256)
    kind, pilot = eng.last_prune_pilot()
    path, n = eng.last_prune_path(), eng.last_contracted_rows()
    assert distributed.init_engine_comm(eng) == (0, 1)
    assert eng.sweep(acq, pl, True, local_result=False) is None  # nothing comes back: the winners stay on the device
    gv, gi, gx = eng.exchange_argmax(len(acq), 1_000_000, True)
    assert gv.tobytes() == v.tobytes()
    np.testing.assert_array_equal(gi, i + 1_000_000)
    np.testing.assert_array_equal(gx, Xs[i])
    kind2, pilot2 = eng.last_prune_pilot()
    assert (kind2, pilot2.tobytes()) == (kind, pilot.tobytes()) and eng.last_prune_path() == path and eng.last_contracted_rows() == n


def test_automatic_mode_keeps_the_first_rows_at_this_size(models, small_chunks):
    eng, X, y, st = models[False]
    pl = float(y.min())
    eng.upload_candidates(PC.candidates())
    eng.set_prune(True)
    seen = []
    for mode in (0, 1):
        eng.set_prune_pilot(mode)
        v, i = eng.sweep(BP.UCB2, pl, True)
        kind, pilot = eng.last_prune_pilot()
        seen.append((v.tobytes(), i.tobytes(), kind, pilot.tobytes(), eng.last_prune_path(), eng.last_contracted_rows(), eng.last_bound32()))
    assert seen[0] == seen[1] and seen[1][2] == FIRST_ROWS and seen[1][4][0] == ONEPASS
    assert seen[1][5] == PC.CHUNK_ROWS + seen[1][4][1]  # the first-rows pilot plus the survivors behind it


def test_setter_refuses_an_unknown_mode_and_a_ragged_block(models):
    eng = models[False][0]
    for mode, block_rows in ((3, 0), (-1, 0), (2, 100), (2, 257), (2, -256)):
        with pytest.raises(_lib.BogpError):
            eng.set_prune_pilot(mode, block_rows)
    eng.set_prune_pilot(2, 768)
    eng.set_prune_pilot()  # automatic, the default block


def test_timing_fields_sum_inside_the_call(models, small_chunks):
    """The one-pass row of the table above collect_timing: acquisition_ms is the whole-sweep span less the producer and contraction
    spans, so the three fields sum to that span -- which lies inside the host's interval around the synchronised call."""
    eng, X, y, st = models[False]
    pl = float(y.min())
    eng.upload_candidates(PC.candidates())
    eng.set_prune(True)
    eng.set_prune_pilot(2, 256)
    eng.sweep(BP.UCB2, pl, True)  # (buffers and events exist)
    t0 = time.perf_counter()
    eng.sweep(BP.UCB2, pl, True)
    wall = 1e3 * (time.perf_counter() - t0)
    t = eng.last_timing()
    total = t["corr_ms"] + t["contract_ms"] + t["acquisition_ms"]
    print(t, "sum %.4f ms, wall %.4f ms" % (total, wall))
    assert eng.last_prune_pilot()[0] == BEST_BOUND and eng.last_prune_path()[0] == ONEPASS
    assert t["corr_ms"] > 0 and t["contract_ms"] > 0 and t["acquisition_ms"] > 0 and total <= wall
    assert t["n_chunks"] == 1 + eng.last_prune_path()[2]
    eng.set_prune_pilot()
