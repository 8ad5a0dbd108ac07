"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/constrained_engine.py extended by `sweep_believer_constrained`,
served by the NumPy restatement of tests/support/believer_constrained_ref.py.  Every call is recorded in `self.calls` so that a test can
tell which entry point a routing decision reached."""
import numpy as np

from support.believer_constrained_ref import BelieverConstrainedRef
from support.constrained_engine import ConstrainedOracleEngine


class BelieverConstrainedOracleEngine(ConstrainedOracleEngine):
    def sweep_believer_constrained(self, acq, plugin, minimize, lo, hi, pending=None, believe_plugin=True, return_values=False):
        acq = list(acq)
        self.calls.append(("sweep_believer_constrained", tuple(int(a) for a, _ in acq), 0 if pending is None else len(pending), bool(believe_plugin)))
        st = self.st
        assert st.trend == 0 and self.n_t >= 2 and not st.estimate_trend and len(np.ravel(lo)) == self.n_t - 1
        ref = BelieverConstrainedRef(self.X, st.theta, st.kernel, self.get_state())
        out = ref.run(self.Xs, acq, plugin, minimize, lo, hi, pending, believe_plugin)
        res = {k: out[k] for k in ("best_val", "best_idx", "best_x", "best_mu", "pivots", "plugins")}
        if return_values:
            res.update(acq=out["acq"], pof=out["pof"], mse=out["mse"])
        return res
