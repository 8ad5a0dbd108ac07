"""TEST-ONLY: the oracle-backed stand-in engine (tests/support/oracle_engine.py) extended by `sweep_constrained`: the oracle's
chunked posterior of every target plus the NumPy restatement of tests/support/constrained_ref.py, and a host stand-in for the device
generator.  Every call is recorded in `self.calls` so that a test can tell which entry point a routing decision reached."""
import numpy as np

from oracle import gp_oracle as O
from support import constrained_ref as R
from support.oracle_engine import OracleEngine


class ConstrainedOracleEngine(OracleEngine):
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

    def sweep_constrained(self, acq, plugin, minimize, lo, hi, k=1, return_values=False, return_pof=False, return_moments=False):
        acq = list(acq)
        self.calls.append(("sweep_constrained", tuple(int(a) for a, _ in acq), int(k)))
        assert self.n_t >= 2 and len(np.ravel(lo)) == self.n_t - 1
        mu, mse = O.predict_chunked(self.st, self.Xs, 1024)
        vals, pof = R.constrained(mu, mse, self.st.sigma2, lo, hi, acq, plugin, minimize)
        pairs = [R.topk(v, int(k)) for v in vals]
        best, idx = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs], dtype=np.int64)
        self.__dict__.setdefault("winners", []).append(self.Xs[idx[0, 0]].copy())
        out = (best, idx)
        if return_values:
            out += (vals,)
        if return_pof:
            out += (pof,)
        if return_moments:
            out += (mu, mse)
        return out

    def set_candidate_transform(self, scales=None, precisions=None, lo=None, hi=None):
        assert scales is None and precisions is None, "the stand-in draws plain designs"

    def generate_candidates(self, lo, hi, M, seed=0, first_row=0, method="uniform", n_total=None, sobol_sv=None, maximin=5):
        self.calls.append(("generate", int(M), method))
        OracleEngine.upload_candidates(self, np.random.default_rng(int(seed) % 2**32).uniform(lo, hi, size=(int(M), len(lo))))
