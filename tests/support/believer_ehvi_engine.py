"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/believer_engine.py extended by `sweep_ehvi` (the float64
restatement of the reference's EHVI on the oracle's moments) and by `sweep_believer_ehvi`, served by the NumPy restatement of
tests/support/believer_ehvi_ref.py.  Every call is recorded in `self.calls` so that a test can tell which entry point a routing
decision reached."""
import numpy as np

from oracle import gp_oracle as O
from support.believer_ehvi_ref import BelieverEhviRef
from support.believer_engine import BelieverOracleEngine
from support.ehvi_ref64 import ehvi as ehvi_ref


class BelieverEhviOracleEngine(BelieverOracleEngine):
    def sweep_ehvi(self, lower, upper, k=1, return_values=False, return_moments=False):
        self.calls.append(("sweep_ehvi", len(lower), int(k)))
        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals = ehvi_ref(mu, mse, lower, upper)
        order = sorted(range(len(vals)), key=lambda j: (-vals[j], j))[:k]
        idx = np.array(order + [-1] * (k - len(order)), dtype=np.int64)
        best = np.array([vals[j] if j >= 0 else -np.inf for j in idx])
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out

    def sweep_believer_ehvi(self, front, ref_point, q, pending=None, believe_front=True, return_values=False):
        self.calls.append(("sweep_believer_ehvi", int(q), 0 if pending is None else len(pending), bool(believe_front)))
        st = self.st
        assert st.trend == 0 and self.n_t > 1 and not st.estimate_trend
        m = len(np.ravel(ref_point))
        ref = BelieverEhviRef(self.X, st.theta, st.kernel, self.get_state())
        out = ref.run(self.Xs, np.zeros((0, m)) if front is None else front, ref_point, int(q), pending, believe_front)
        res = {k: out[k] for k in ("best_val", "best_idx", "best_x", "best_mu", "pivots", "n_cells")}
        if return_values:
            res.update(ehvi=out["ehvi"], mse=out["mse"])
        return res
