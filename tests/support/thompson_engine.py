"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/believer_engine.py extended by `sweep_thompson`, served by the dense
NumPy restatement `bogp.thompson.paths_numpy`.  Every call is recorded in `self.calls`."""
import numpy as np

from bogp import _lib, thompson
from oracle import gp_oracle as O
from support.believer_engine import BelieverOracleEngine


def ranking(crit, k):
    """np.argmax order (first maximum, NaN maximal) of every row of `crit` (q, M), k ranks: (values (q, k), indices (q, k)); slots
    beyond M are (-inf, -1)."""
    q, M = crit.shape
    val, idx = np.full((q, k), -np.inf), np.full((q, k), -1, dtype=np.int64)
    for j in range(q):
        key = np.where(np.isnan(crit[j]), np.inf, crit[j])
        order = np.argsort(-key, kind="stable")[:k]
        val[j, : len(order)], idx[j, : len(order)] = crit[j][order], order
    return val, idx


class ThompsonOracleEngine(BelieverOracleEngine):
    def dense_state(self):
        st = self.st
        if st.mode != O.MODE_NOISELESS:
            raise NotImplementedError("stand-in: %s mode" % ("noisy" if st.mode == O.MODE_NOISY else "noise-estimating"))
        assert st.trend == 0 and self.n_t == 1
        nu = float(st.theta[-1]) if st.kernel == _lib.KERNEL_MATERN_NU else None
        theta = st.theta[:-1] if st.kernel == _lib.KERNEL_MATERN_NU else st.theta
        return thompson.dense_state(self.X, self.y[:, 0], theta, st.kernel, st.estimate_trend, beta=float(st.beta[0, 0]), nu=nu,
                                    sigma2=float(st.sigma2[0]))  # fmt: skip

    def sweep_thompson(self, draw, minimize=True, k=1, conditioned=True, return_values=False):
        q = draw.weights.shape[1]
        self.calls.append(("sweep_thompson", q, int(k), bool(conditioned)))
        paths, coef = thompson.paths_numpy(self.dense_state(), draw, self.Xs, conditioned)
        val, idx = ranking(-paths if minimize else paths, int(k))
        bx = np.where((idx >= 0)[..., None], self.Xs[np.clip(idx, 0, len(self.Xs) - 1)], np.nan)
        out = dict(best_val=val, best_idx=idx, best_x=bx, coef=coef)
        if return_values:
            out["paths"] = paths
        return out
