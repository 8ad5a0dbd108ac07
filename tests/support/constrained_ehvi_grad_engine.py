"""TEST-ONLY: the stand-in engine of tests/support/constrained_ehvi_engine.py extended by what `ConstrainedEHVI(input_gradient=True)`
reaches -- `point_eval_ehvi_constrained` through the gradient restatement of tests/support/constrained_ehvi_grad_ref.py.  It has NO
`polish_ehvi_constrained`, so `optim.polish_topk` takes its sequential fall-back on the one-point call.  Calls are recorded in
`self.calls`."""
import numpy as np

from support import constrained_ehvi_grad_ref as R
from support.constrained_ehvi_engine import ConstrainedEhviOracleEngine


class ConstrainedEhviGradOracleEngine(ConstrainedEhviOracleEngine):
    def point_eval_ehvi_constrained(self, X, lower, upper, lo, hi, moments=False):
        X = np.atleast_2d(np.asarray(X, float))
        lower = np.asarray(lower, float)
        m = lower.shape[1]
        self.calls.append(("point_eval_ehvi_constrained", len(X), int(m), len(lower)))
        assert self.n_t == m + len(np.ravel(lo)) and m >= 2
        out = R.batch(self.st, X, m, lower, upper, lo, hi)
        return out if moments else out[:2]
