"""TEST-ONLY: the oracle-backed stand-in engine (tests/support/oracle_engine.py) extended by what `EHVI(input_gradient=True)`
reaches on a Gaussian process -- `sweep_ehvi` through the float64 restatement of the reference's EHVI, `point_eval_ehvi` through the
gradient restatement of tests/support/ehvi_grad_ref.py, and a host stand-in for the device generator.  It has NO `polish_ehvi`, so
`optim.polish_topk` takes its sequential fall-back on the one-point call.  Calls are recorded in `self.calls`."""
import numpy as np

from oracle import gp_oracle as O
from support import ehvi_grad_ref as R
from support.ehvi_ref64 import ehvi as ehvi_ref
from support.oracle_engine import OracleEngine


class EhviGradOracleEngine(OracleEngine):
    def __init__(self, device=0):
        super().__init__(device)
        self.calls = []

    def sweep_ehvi(self, lower, upper, k=1, return_values=False, return_moments=False):
        self.calls.append(("sweep_ehvi", len(self.Xs), int(k)))
        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals = ehvi_ref(mu, mse, lower, upper)
        order = sorted(range(len(vals)), key=lambda j: (-vals[j], j))[:k]
        idx = np.array(order + [-1] * (k - len(order)), dtype=np.int64)
        best = np.array([vals[j] if j >= 0 else -np.inf for j in idx])
        self.last_sweep = (best.copy(), self.Xs[idx[0]].copy())
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_moments:
            out += (mu, mse)
        return out

    def point_eval_ehvi(self, X, lower, upper, moments=False):
        X = np.atleast_2d(np.asarray(X, float))
        self.calls.append(("point_eval_ehvi", len(X)))
        out = R.batch(self.st, X, lower, upper)
        return out if moments else out[:2]

    def set_candidate_transform(self, scale, precision, lo, hi):
        self._prec = None if precision is None else list(precision)

    def generate_candidates(self, lo, hi, M, seed=0, first_row=0, method="uniform", n_total=None, sobol_sv=None, maximin=5):
        X = np.random.default_rng(int(seed) % 2**32).uniform(lo, hi, size=(int(M), len(lo)))
        for j, p in enumerate(getattr(self, "_prec", None) or []):
            if p is not None:
                X[:, j] = np.round(X[:, j], p)
        self.upload_candidates(X)
