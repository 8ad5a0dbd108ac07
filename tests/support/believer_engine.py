"""TEST-ONLY: the oracle-backed stand-in engine (tests/support/oracle_engine.py) extended by `sweep_believer`, served by the
NumPy restatement of tests/support/believer_ref.py, and by a host stand-in for the device generator.  Every call is recorded in
`self.calls` so that a test can tell which entry point a routing decision reached."""
import numpy as np

from support.believer_ref import BelieverRef
from support.oracle_engine import OracleEngine


class BelieverOracleEngine(OracleEngine):
    def __init__(self, device=0):
        super().__init__(device)
        self.calls = []

    def upload_candidates(self, Xs, lazy=False):
        self.calls.append(("upload", len(Xs)))
        return super().upload_candidates(Xs)

    def sweep(self, acq, plugin, minimize=True, return_values=False, local_result=True):
        self.calls.append(("sweep", len(acq)))
        return super().sweep(acq, plugin, minimize, return_values, local_result)

    def sweep_topk(self, acq, plugin, minimize=True, k=1):
        self.calls.append(("sweep_topk", len(acq), int(k)))
        return super().sweep_topk(acq, plugin, minimize, k)

    def sweep_believer(self, acq, plugin, minimize=True, pending=None, believe_plugin=True, return_values=False):
        self.calls.append(("sweep_believer", len(acq), 0 if pending is None else len(pending), bool(believe_plugin)))
        st = self.st
        assert st.trend == 0 and self.n_t == 1
        ref = BelieverRef(self.X, st.theta, st.kernel, self.get_state(), st.estimate_trend)
        out = ref.run(self.Xs, list(acq), plugin, minimize, pending, believe_plugin)
        res = dict(best_val=out["best_val"], best_idx=out["best_idx"], best_x=out["best_x"], pivots=out["pivots"])
        if return_values:
            res.update(acq=out["acq"], mse=out["mse"])
        return res

    def set_candidate_transform(self, scales=None, precisions=None, lo=None, hi=None):
        assert scales is None and precisions is None, "the stand-in draws plain designs"

    def generate_candidates(self, lo, hi, M, seed=0, first_row=0, method="uniform", n_total=None, sobol_sv=None, maximin=5):
        self.calls.append(("generate", int(M), method))
        OracleEngine.upload_candidates(self, np.random.default_rng(int(seed) % 2**32).uniform(lo, hi, size=(int(M), len(lo))))
