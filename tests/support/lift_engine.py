"""TEST-ONLY: the oracle-backed stand-in engine (tests/support/oracle_engine.py) extended by the lifted sweep of
`bogp_lift_sweep_topk`, restated in NumPy through `bogp.Lift` (section 1 of the contract in include/bogp.h: a row whose
lifted point leaves the original box competes with its penalty, a feasible row with its criterion value; first maximum,
ties -> lower index, a NaN wins, slots beyond M are (-inf, -1)), and by a host stand-in for the device generator that
draws with a seeded NumPy generator.  The posterior runs on the FEASIBLE rows only, as on the device."""
import numpy as np

from bogp import Lift
from oracle import gp_oracle as O

from support.oracle_engine import OracleEngine


def rank_rows(v, k):
    """(values (k,), indices (k,)) of the k best entries of v under bogp_sweep_topk's rules."""
    v = np.asarray(v, dtype=float)
    key = np.where(np.isnan(v), np.inf, v)  # a NaN is maximal
    order = np.lexsort((np.arange(len(v)), -key))[:k]
    best, idx = np.full(k, -np.inf), np.full(k, -1, dtype=np.int64)
    best[: len(order)], idx[: len(order)] = v[order], order
    return best, idx


class LiftOracleEngine(OracleEngine):
    lift = None

    def set_lift(self, A, mean, center, lo, hi):
        lift = Lift(A, mean, center, lo, hi)
        assert lift.r == self.d, "A must have shape (%d, D)" % self.d
        self.lift = lift

    def clear_lift(self):
        self.lift = None

    def lifted_values(self, acq, plugin, minimize=True):
        """(values (q, M), penalty (M,), feasible (M,)) of the current candidates under the engine's lift"""
        assert self.lift is not None, "no lift: call set_lift first"
        pen = self.lift.penalty(self.Xs)
        feas = pen == 0
        vals = np.tile(pen, (len(acq), 1))
        if feas.any():
            mu, mse = O.predict_chunked(self.st, self.Xs[feas], 1024)
            mu, mse = mu[:, self.target], mse[:, self.target]
            for c, (a, p) in enumerate(acq):
                vals[c, feas] = O.acquisition(a, p, mu, mse, plugin, self.st.sigma2[0], minimize)
        return vals, pen, feas

    def lift_sweep_topk(self, acq, plugin, minimize=True, k=1, return_values=False, return_penalty=False):
        vals, pen, feas = self.lifted_values(acq, plugin, minimize)
        ranked = [rank_rows(v, int(k)) for v in vals]
        out = (np.array([r[0] for r in ranked]), np.array([r[1] for r in ranked]), int(feas.sum()))
        self.__dict__.setdefault("lifted_sweeps", []).append((self.Xs.copy(), vals, out[1][:, 0].copy()))
        if return_values:
            out += (vals,)
        if return_penalty:
            out += (pen,)
        return out

    def lift_last(self):
        return dict(n_feasible=0, filter_ms=0.0, merge_ms=0.0)

    # -- host stand-in for the device generator (uniform rows in the drawing box from a seeded NumPy generator) ----
    def set_candidate_transform(self, scales=None, precisions=None, lo=None, hi=None):
        assert scales is None and precisions is None, "the stand-in draws plain designs"

    def generate_candidates(self, lo, hi, M, seed=0, first_row=0, method="uniform", n_total=None, sobol_sv=None, maximin=5):
        self.upload_candidates(np.random.default_rng(int(seed) % 2**32).uniform(lo, hi, size=(int(M), len(lo))))
