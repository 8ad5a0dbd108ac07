"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/constrained_ehvi_engine.py extended by
`sweep_believer_ehvi_constrained`, served by the NumPy restatement of tests/support/believer_constrained_ehvi_ref.py.  Every call is
recorded in `self.calls` so that a test can tell which entry point a routing decision reached."""
import numpy as np

from support.believer_constrained_ehvi_ref import BelieverConstrainedEhviRef
from support.constrained_ehvi_engine import ConstrainedEhviOracleEngine


class BelieverConstrainedEhviOracleEngine(ConstrainedEhviOracleEngine):
    def sweep_believer_ehvi_constrained(self, front, ref_point, q, lo, hi, pending=None, believe_front=True, feasibility_only=False,
                                        return_values=False):
        m = len(np.ravel(ref_point))
        front = np.zeros((0, m)) if front is None else np.asarray(front, float).reshape(-1, m)
        self.calls.append(("sweep_believer_ehvi_constrained", m, int(q), len(front), 0 if pending is None else len(pending), bool(believe_front),
                           bool(feasibility_only)))  # fmt: skip
        st = self.st
        assert st.trend == 0 and not st.estimate_trend and self.n_t == m + len(np.ravel(lo)) and not (feasibility_only and len(front))
        ref = BelieverConstrainedEhviRef(self.X, st.theta, st.kernel, self.get_state())
        out = ref.run(self.Xs, front, ref_point, int(q), lo, hi, pending, believe_front, feasibility_only)
        res = {k: out[k] for k in ("best_val", "best_idx", "best_x", "best_mu", "pivots", "n_cells")}
        if return_values:
            res.update(val=out["val"], pof=out["pof"], mse=out["mse"])
        return res
