"""TEST-ONLY: the stand-in engine of tests/support/constrained_engine.py extended by what `Constrained(input_gradient=True)` reaches --
`point_eval_constrained` through the gradient restatement of tests/support/constrained_grad_ref.py.  It has NO `polish_constrained`,
so `optim.polish_topk` takes its sequential fall-back on the one-point call.  Calls are recorded in `self.calls`."""
import numpy as np

from support import constrained_grad_ref as R
from support.constrained_engine import ConstrainedOracleEngine


class ConstrainedGradOracleEngine(ConstrainedOracleEngine):
    def point_eval_constrained(self, X, acq, plugin, minimize, lo, hi, moments=False):
        X = np.atleast_2d(np.asarray(X, float))
        acq = list(acq)
        self.calls.append(("point_eval_constrained", len(X), tuple(int(a) for a, _ in acq)))
        assert self.n_t >= 2 and len(np.ravel(lo)) == self.n_t - 1
        out = R.batch(self.st, X, lo, hi, acq, plugin, minimize)
        return out if moments else out[:2]
