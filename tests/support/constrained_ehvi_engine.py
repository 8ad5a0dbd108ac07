"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/constrained_engine.py extended by `sweep_ehvi_constrained`: the
oracle's chunked posterior of every target plus the NumPy restatement of tests/support/constrained_ehvi_ref.py.  Every call is recorded
in `self.calls` so that a test can tell which entry point a routing decision reached."""
import numpy as np

from oracle import gp_oracle as O
from support import constrained_ehvi_ref as R
from support.constrained_engine import ConstrainedOracleEngine


class ConstrainedEhviOracleEngine(ConstrainedOracleEngine):
    def sweep_ehvi_constrained(self, lower, upper, lo, hi, k=1, return_values=False, return_pof=False, return_moments=False):
        lower, upper = np.atleast_2d(np.asarray(lower, float)), np.atleast_2d(np.asarray(upper, float))
        m = lower.shape[1]
        self.calls.append(("sweep_ehvi_constrained", int(m), len(lower), int(k)))
        assert self.n_t == m + len(np.ravel(lo)) and m >= 2
        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals, pof = R.values(mu, mse, self.st.sigma2, m, lower, upper, lo, hi)
        best, idx = R.topk(vals, int(k))
        self.__dict__.setdefault("winners", []).append(self.Xs[idx[0]].copy())
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_pof:
            out += (pof,)
        if return_moments:
            out += (mu, mse)
        return out

    def sweep_ehvi(self, lower, upper, k=1, return_values=False, return_moments=False):
        self.calls.append(("sweep_ehvi", np.atleast_2d(lower).shape[1], len(lower), int(k)))
        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals = R.ehvi(mu, mse, lower, upper)
        best, idx = R.topk(vals, int(k))
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out
