"""TEST-ONLY: the oracle-backed stand-in engine of tests/support/believer_constrained_engine.py extended by
`sweep_thompson_constrained`, served by the dense NumPy restatement `bogp.thompson.paths_multi_numpy` / `select_numpy`.  Every call is
recorded in `self.calls`."""
import numpy as np

from bogp import _lib, thompson
from oracle import gp_oracle as O
from support.believer_constrained_engine import BelieverConstrainedOracleEngine


class ThompsonConstrainedOracleEngine(BelieverConstrainedOracleEngine):
    def dense_state_multi(self):
        st = self.st
        if st.mode != O.MODE_NOISELESS:
            raise NotImplementedError("stand-in: %s mode" % ("noisy" if st.mode == O.MODE_NOISY else "noise-estimating"))
        assert st.trend == 0 and self.n_t >= 2 and not st.estimate_trend
        nu = float(st.theta[-1]) if st.kernel == _lib.KERNEL_MATERN_NU else None
        theta = st.theta[:-1] if st.kernel == _lib.KERNEL_MATERN_NU else st.theta
        return thompson.dense_state_multi(self.X, self.y, theta, st.kernel, beta=float(np.ravel(st.beta)[0]), nu=nu, sigma2=np.ravel(st.sigma2))

    def sweep_thompson_constrained(self, draw, q, lo, hi, minimize=True, k=1, return_values=False):
        q, k = int(q), int(k)
        self.calls.append(("sweep_thompson_constrained", q, k, bool(minimize)))
        dst = self.dense_state_multi()
        assert draw.weights.shape[1] == q * self.n_t <= 16 and len(np.ravel(lo)) == self.n_t - 1
        paths, gt = thompson.paths_multi_numpy(dst, draw, self.Xs)
        sel = thompson.select_numpy(paths, lo, hi, dst.sigma2, minimize, k)
        idx = sel["best_idx"]
        bx = np.where((idx >= 0)[..., None], self.Xs[np.clip(idx, 0, len(self.Xs) - 1)], np.nan)
        out = dict(best_val=sel["best_val"], best_idx=idx, best_x=bx, coef=gt)
        if return_values:
            out["paths"] = paths
        return out
