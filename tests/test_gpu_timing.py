"""What bogp_last_timing and the four *_last calls report, path by path (the table above collect_timing, csrc/bogp_api_sweep.hip): which
fields are zero, which are positive, how many chunks -- and that no interval is counted twice: the fields of one call are sums of device
intervals that lie inside the host's interval around the synchronised call, so their sum stays below the wall time.  A span on the wrong
pair of events, or a span left over from the call before, breaks one of the two.

Model and candidates of tests/prune_cases.py: N = 544, d = 3, M = 3001; BOGP_CHUNK_MB=1 gives 192 rows a chunk, 16 chunks.

The bound: corr_ms + contract_ms + acquisition_ms <= wall (time.perf_counter() around the call, ms) + EXCESS_MS.  Measured on the commit
before the span ledger over 20 repetitions of each of the 17 paths below (MI355X): the sum never reached the wall; the closest any
repetition came was PARENT_EXCESS_MS = -0.0465 ms (the one launch: 0.026 ms of kernel inside a 0.075 ms call), the chunked paths stayed
0.05 .. 0.22 ms below it.  The parent never exceeds the bound, so EXCESS_MS = 0: the plain inequality.  Every figure is printed
before it is asserted (pytest -s).

predict() without MSE launches nothing between a chunk's contraction marks, and the existing bound for that (tests/test_gpu_parity.py:
contract_ms < 0.05 at one chunk) is for ONE such pair of marks.  An empty pair still measures about 0.005 ms, so at 16 chunks the parent
itself reports 0.082 ms: the bound is asserted as it stands at one chunk and per pair at sixteen."""
import time

import numpy as np
import pytest

import prune_cases as PC
from bogp import _lib, thompson
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

EI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_UCB, _lib.ACQ_MGFI
NONE, CHUNKS, ONEPASS, FALLBACK = (_lib.PRUNE_PATH_NONE, _lib.PRUNE_PATH_CHUNKS, _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK)
N_CHUNKS = (PC.M_CAND + PC.CHUNK_ROWS - 1) // PC.CHUNK_ROWS  # 16
PARENT_EXCESS_MS = -0.0465  # largest (sum - wall) the commit before showed over 20 repetitions per path
EXCESS_MS = 0.0             # twice that excess where it is positive
FIELDS = ("corr_ms", "contract_ms", "acquisition_ms")


def walled(call, read):
    """(what `read` reports after the synchronised `call`, wall ms around the call)"""
    t0 = time.perf_counter()
    call()
    wall = 1e3 * (time.perf_counter() - t0)
    return read(), wall


def bounded(name, t, wall):
    """the *_ms fields of one call sum to no more than the wall time around it"""
    total = sum(v for k, v in t.items() if k.endswith("_ms"))
    print("%-28s %s  sum %.4f ms, wall %.4f ms, excess %.4f" % (name, {k: round(v, 4) if k.endswith("_ms") else v for k, v in t.items()}, total, wall, total - wall))
    assert all(v >= 0 for k, v in t.items() if k.endswith("_ms")), t
    assert total <= wall + EXCESS_MS, (name, t, wall)


def all_positive(t, n_chunks):
    assert t["n_chunks"] == n_chunks and all(t[k] > 0 for k in FIELDS), t


class Paths:
    """The engines of the cases below and one method per path: each runs its call synchronised and returns (timing, wall).
    (`single_stream` lists them: what the measurement in the module docstring repeats.)"""

    def __init__(self):
        self.X, self.y, par, self.st = PC.model(False)
        self.pl = float(self.y.min())
        self.Xs = PC.candidates()
        self.eng = _lib.Engine(0)
        self.eng.set_train(self.X, self.y)
        self.eng.commit(PC.KERNEL, _lib.MODE_NOISY, par, PC.NOISE, False, 0.0)
        self.small = _lib.Engine(0)  # the one-launch model: N = 100, d = 3, M = 1000
        self.one_launch_model(self.small)
        self.multi = None
        self.loaded = None

    def close(self):
        for e in (self.eng, self.small, self.multi):
            if e is not None:
                e.close()

    @staticmethod
    def one_launch_model(eng):
        rng = np.random.default_rng(5)
        X = rng.uniform(-5, 5, size=(100, 3))
        y = np.sum(X**2, axis=1)
        y = ((y - y.mean()) / y.std()).reshape(-1, 1)
        eng.set_train(X, y)
        eng.commit(PC.KERNEL, _lib.MODE_NOISY, np.r_[np.full(3, 0.05), 0.9], PC.NOISE, False, 0.0)
        eng.upload_candidates(rng.uniform(-5, 5, size=(1000, 3)))
        return float(y.min())

    def load(self, what, Xs=None):  # (an upload only where the candidates change)
        if self.loaded != what:
            self.eng.upload_candidates(self.Xs if Xs is None else Xs)
            self.loaded = what

    def sweep(self, acq, prune, **kw):
        self.eng.set_prune(prune)
        return walled(lambda: self.eng.sweep(acq, self.pl, True, **kw), self.eng.last_timing)

    def small_batch(self):
        self.load("20", self.Xs[:20])
        return self.sweep([(EI, 0.0)], True)

    def one_launch(self):
        return walled(lambda: self.small.sweep([(EI, 0.0)], -1.0, True), self.small.last_timing)

    def predict_mse(self):
        self.load("all")
        return walled(self.eng.predict, self.eng.last_timing)

    def predict_mean(self):
        self.load("all")
        return walled(lambda: self.eng.predict(eval_MSE=False), self.eng.last_timing)

    def chunked_q2(self):
        self.load("all")
        return self.sweep([(EI, 0.0), (MGFI, 2.0)], False)

    def pruned_chunks(self):
        self.load("all")
        return self.sweep([(UCB, 0.5)], "chunks")

    def onepass(self, alpha):
        self.load("all")
        return self.sweep([(UCB, alpha)], True)

    def segment_fall_back_rows(self):
        """tests/test_gpu_prune_onepass.py::test_forced_segment_fall_back: the pilot holds the winner and the 191 lowest bounds"""
        mu, mse, sd_ub = PC.oracle_rows(self.st, self.Xs)
        s2 = float(self.st.sigma2[0])
        w = int(np.argmax(O.acquisition(UCB, 30.0, mu, mse, self.pl, s2, True)))
        b = PC.upper_bounds(UCB, 30.0, mu, sd_ub, self.pl, s2)
        head = np.array([w] + [int(r) for r in np.argsort(b, kind="stable") if r != w][: PC.CHUNK_ROWS - 1])
        return self.Xs[np.r_[head, np.setdiff1d(np.arange(len(self.Xs)), head)]]

    def segment_fall_back(self):
        if not hasattr(self, "Xr"):
            self.Xr = self.segment_fall_back_rows()
        self.load("reordered", self.Xr)
        return self.sweep([(UCB, 30.0)], True)

    def multi_model(self):
        """m = 3, N = 700 (Np = 704: 128 rows a chunk at BOGP_CHUNK_MB=1), M = 1000: tests/test_gpu_ehvi.py::test_chunk_invariance_and_topk"""
        from test_gpu_constrained import _bounds
        from test_gpu_ehvi import _model

        if self.multi is None:
            self.multi = _lib.Engine(0)
            X, Y, self.cells_lo, self.cells_hi = _model(self.multi, 3, 700, 5, _lib.KERNEL_MATERN52, True, seed=3)
            self.multi.upload_candidates(np.random.default_rng(2).uniform(-2.5, 2.5, size=(1000, 5)))
            self.box_lo, self.box_hi = _bounds(Y)
            self.multi_pl = float(Y[:, 0].min())
        return self.multi

    def multi_plain(self):
        e = self.multi_model()
        e.set_prune(False)
        return walled(lambda: e.sweep([(EI, 0.0)], self.multi_pl, True), e.last_timing)

    def ehvi(self):
        e = self.multi_model()
        return walled(lambda: e.sweep_ehvi(self.cells_lo, self.cells_hi), e.last_timing)

    def constrained(self):
        e = self.multi_model()
        return walled(lambda: e.sweep_constrained([(EI, 0.0), (MGFI, 2.0)], self.multi_pl, True, self.box_lo, self.box_hi), e.last_timing)

    def believer(self):
        self.load("all")
        self.eng.set_prune(True)
        pend = np.random.default_rng(3).uniform(-5, 5, size=(1, PC.DIM))
        acq = [(EI, 0.0), (UCB, 2.0), (MGFI, 2.0)]
        return walled(lambda: self.eng.sweep_believer(acq, self.pl, True, pending=pend), self.eng.believer_last)

    def believer_ehvi(self):
        e = self.multi_model()
        pend = np.random.default_rng(3).uniform(-2, 2, size=(1, 5))
        ref = np.array([-3.0, -5.0, -7.0])
        return walled(lambda: e.sweep_believer_ehvi(np.zeros((0, 3)), ref, 3, pending=pend), e.believer_ehvi_last)

    def thompson(self):
        """q = 2 paths of a noiseless N = 300, d = 5 model over M = 1000: chunks of 384, 384 and 232 rows at BOGP_CHUNK_MB=1"""
        from test_gpu_thompson import commit, problem

        if not hasattr(self, "th"):
            self.th = _lib.Engine(0)
            X, y, theta, Xs = problem(1000, 5, 300, _lib.KERNEL_MATERN52)
            st = commit(self.th, X, y, theta, _lib.KERNEL_MATERN52, True)
            self.th.upload_candidates(Xs)
            self.th_draw = thompson.draw(st, 2, 48, seed=5)
        return walled(lambda: self.th.sweep_thompson(self.th_draw, k=1), self.th.thompson_last)

    def lift(self):
        """tests/test_gpu_lift.py::test_feasible_rows_get_the_plain_sweeps_bits at N = 1024: r = 3, D = 20, M = 20011"""
        from test_gpu_lift import Q4, _lift, _model, _set

        if not hasattr(self, "lf"):
            self.lf = _lib.Engine(0)
            self.lf_pl = _model(self.lf, 1024, 3, seed=3)
            self.lf.upload_candidates(np.random.default_rng(8).uniform(-1, 1, size=(20011, 3)))
            _set(self.lf, _lift(3, 20))
        return walled(lambda: self.lf.lift_sweep_topk(Q4, self.lf_pl, True, k=16), self.lf.lift_last)

    def single_stream(self):
        """(name, method, arguments) of every single-stream path of the module, in the order the tests run them"""
        return [("small batch", self.small_batch, ()), ("one launch", self.one_launch, ()), ("predict with MSE", self.predict_mse, ()),
                ("predict, mean only", self.predict_mean, ()), ("chunks, q = 2", self.chunked_q2, ()), ("pruned chunks", self.pruned_chunks, ()),
                ("one pass, UCB 0.5", self.onepass, (0.5,)), ("one pass, UCB 15", self.onepass, (15.0,)), ("whole fall-back, UCB 50", self.onepass, (50.0,)),
                ("segment fall-back", self.segment_fall_back, ()), ("multi-target plain", self.multi_plain, ()), ("EHVI", self.ehvi, ()),
                ("constrained", self.constrained, ()), ("believer", self.believer, ()), ("believer EHVI", self.believer_ehvi, ()),
                ("Thompson", self.thompson, ()), ("lift", self.lift, ())]  # fmt: skip


@pytest.fixture(scope="module")
def paths():
    p = Paths()
    yield p
    p.close()
    for e in (getattr(p, "th", None), getattr(p, "lf", None)):
        if e is not None:
            e.close()


@pytest.fixture()
def small_chunks(monkeypatch):
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")


def test_small_batch_reports_nothing(paths, small_chunks):
    t, wall = paths.small_batch()
    bounded("small batch", t, wall)
    assert t == dict(corr_ms=0.0, contract_ms=0.0, acquisition_ms=0.0, n_chunks=0)


def test_one_launch_is_the_contractions_time(paths, small_chunks):
    t, wall = paths.one_launch()
    bounded("one launch", t, wall)
    assert t["corr_ms"] == 0 and t["acquisition_ms"] == 0 and t["contract_ms"] > 0 and t["n_chunks"] == 1


def test_chunks_without_pruning(paths, small_chunks, monkeypatch):
    for name, run in (("predict with MSE", paths.predict_mse), ("chunks, q = 2", paths.chunked_q2)):
        t, wall = run()
        bounded(name, t, wall)
        all_positive(t, N_CHUNKS)
    assert paths.eng.last_prune_path() == (NONE, 0, 0)
    t, wall = paths.predict_mean()
    bounded("predict, mean only", t, wall)
    assert t["n_chunks"] == N_CHUNKS and t["corr_ms"] > 0 and t["acquisition_ms"] > 0
    assert t["contract_ms"] < 0.05 * N_CHUNKS  # nothing was launched between the two marks of any chunk
    monkeypatch.delenv("BOGP_CHUNK_MB")
    t, wall = paths.predict_mean()
    bounded("predict, mean only, 1 chunk", t, wall)
    assert t["n_chunks"] == 1 and t["corr_ms"] > 0 and t["acquisition_ms"] > 0
    assert t["contract_ms"] < 0.05  # (tests/test_gpu_parity.py's bound, at its geometry: one pair of marks)


def test_pruned_chunks(paths, small_chunks):
    t, wall = paths.pruned_chunks()
    bounded("pruned chunks", t, wall)
    assert paths.eng.last_prune_path() == (CHUNKS, 0, 0)
    all_positive(t, N_CHUNKS)


@pytest.mark.parametrize("alpha,rounds", [(0.5, 1), (15.0, 3)])
def test_one_pass_counts_its_contraction_launches(paths, small_chunks, alpha, rounds):
    t, wall = paths.onepass(alpha)
    bounded("one pass, UCB %g" % alpha, t, wall)
    path, surv, n_rounds = paths.eng.last_prune_path()
    assert path == ONEPASS and n_rounds == rounds
    assert t["n_chunks"] == 1 + rounds and t["corr_ms"] > 0 and t["contract_ms"] > 0 and t["acquisition_ms"] >= 0


def test_whole_sweep_fall_back(paths, small_chunks):
    t, wall = paths.onepass(50.0)
    bounded("whole fall-back, UCB 50", t, wall)
    assert paths.eng.last_prune_path() == (CHUNKS, 0, 0)
    all_positive(t, 1 + N_CHUNKS)  # sweep_onepass counts contraction launches: the pilot's, then one per chunk of sweep_chunks(0, 16)


def test_forced_segment_fall_back(paths, small_chunks):
    t, wall = paths.segment_fall_back()
    bounded("segment fall-back", t, wall)
    assert paths.eng.last_prune_path() == (FALLBACK, 0, 0)
    all_positive(t, N_CHUNKS)  # the pilot's contraction, then chunks 1 .. 15: the segment behind the pilot starts in chunk 1


@pytest.mark.parametrize("chunk_mb,n_chunks", [(None, 1), ("1", 8)])
def test_ehvi_and_constrained_have_the_plain_sweeps_chunks(paths, monkeypatch, chunk_mb, n_chunks):
    if chunk_mb:
        monkeypatch.setenv("BOGP_CHUNK_MB", chunk_mb)
    plain, wall = paths.multi_plain()
    bounded("multi-target plain", plain, wall)
    all_positive(plain, n_chunks)
    for name, run in (("EHVI", paths.ehvi), ("constrained", paths.constrained)):
        t, wall = run()
        bounded(name, t, wall)
        all_positive(t, plain["n_chunks"])


def test_believer_thompson_and_lift_sums(paths, small_chunks):
    t, wall = paths.believer()
    bounded("believer", t, wall)
    assert t["n_passes"] == 3 and t["corr_ms"] > 0 and t["solve_ms"] > 0 and t["believer_ms"] > 0  # one pending point + the first two winners
    t, wall = paths.believer_ehvi()
    bounded("believer EHVI", t, wall)
    assert t["n_passes"] == 3 and t["ehvi_ms"] > 0 and t["update_ms"] > 0 and t["solve_ms"] > 0 and t["corr_ms"] > 0
    t, wall = paths.thompson()
    bounded("Thompson", t, wall)
    assert t["n_chunks"] == 3 and t["corr_ms"] > 0 and t["solve_ms"] > 0 and t["paths_ms"] > 0
    t, wall = paths.lift()
    bounded("lift", t, wall)
    assert 100 < t["n_feasible"] < 10000 and t["filter_ms"] > 0 and t["merge_ms"] > 0


def test_no_span_outlives_its_call(paths, monkeypatch):
    """One handle: 16 chunks, then one chunk, then the one-launch model.  Each call's report is that call's alone."""
    e = _lib.Engine(0)
    try:
        e.set_train(paths.X, paths.y)
        e.commit(PC.KERNEL, _lib.MODE_NOISY, np.r_[np.full(PC.DIM, 0.05), 0.01], PC.NOISE, False, 0.0)
        e.upload_candidates(paths.Xs)
        e.set_prune(False)
        acq = [(EI, 0.0), (MGFI, 2.0)]
        monkeypatch.setenv("BOGP_CHUNK_MB", "1")
        t, wall = walled(lambda: e.sweep(acq, paths.pl, True), e.last_timing)
        bounded("16 chunks", t, wall)
        all_positive(t, N_CHUNKS)
        monkeypatch.delenv("BOGP_CHUNK_MB")
        t, wall = walled(lambda: e.sweep(acq, paths.pl, True), e.last_timing)
        bounded("then one chunk", t, wall)
        all_positive(t, 1)
        one_chunk = t
        Paths.one_launch_model(e)
        t, wall = walled(lambda: e.sweep(acq, -1.0, True), e.last_timing)
        bounded("then one launch", t, wall)
        assert t["corr_ms"] == 0 and t["acquisition_ms"] == 0 and 0 < t["contract_ms"] and t["n_chunks"] == 1
        assert one_chunk["contract_ms"] > 0
    finally:
        e.close()


def test_lazy_reading_waits_and_repeats(paths, small_chunks):
    """A queued sweep (local_result=False) followed at once by last_timing(): the read waits for the events; a second read returns the
    same bits."""

    def queued(eng, acq, plugin, prune):
        eng.set_prune(prune)
        t0 = time.perf_counter()
        assert eng.sweep(acq, plugin, True, local_result=False) is None
        t = eng.last_timing()
        wall = 1e3 * (time.perf_counter() - t0)
        assert eng.last_timing() == t
        return t, wall

    paths.load("all")
    t, wall = queued(paths.eng, [(EI, 0.0), (MGFI, 2.0)], paths.pl, False)
    bounded("queued chunks", t, wall)
    all_positive(t, N_CHUNKS)
    t, wall = queued(paths.eng, [(UCB, 15.0)], paths.pl, True)
    bounded("queued one pass", t, wall)
    assert paths.eng.last_prune_path()[0] == ONEPASS and t["n_chunks"] == 1 + 3 and t["corr_ms"] > 0 and t["contract_ms"] > 0 and t["acquisition_ms"] >= 0
    t, wall = queued(paths.small, [(EI, 0.0)], -1.0, True)
    bounded("queued one launch", t, wall)
    assert t["corr_ms"] == 0 and t["acquisition_ms"] == 0 and t["contract_ms"] > 0 and t["n_chunks"] == 1
