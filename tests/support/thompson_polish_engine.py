"""TEST-ONLY: the stand-in engine of tests/support/thompson_engine.py extended by `polish_path`, served by scipy's L-BFGS-B on the dense
restatement `bogp.thompson.path_grad_numpy`.  Every call is recorded in `self.calls`."""
import numpy as np
from scipy.optimize import minimize as scipy_minimize

from bogp import thompson
from support.thompson_engine import ThompsonOracleEngine


class ThompsonPolishOracleEngine(ThompsonOracleEngine):
    def polish_path(self, starts, lo, hi, draw, coef, members, minimize=True, max_evals=50, pgtol=1e-8, factr=1e6):
        starts = np.clip(np.atleast_2d(np.asarray(starts, dtype=float)), lo, hi)
        self.calls.append(("polish_path", len(starts), list(map(int, members)), int(max_evals)))
        st, sign = self.dense_state(), 1.0 if minimize else -1.0

        def fun(x, j):
            v, g = thompson.path_grad_numpy(st, draw, x[None, :], [j])
            return sign * v[0], sign * g[0]

        X, f, n = starts.copy(), np.empty(len(starts)), np.zeros(len(starts), dtype=np.int32)  # (never worse than the clipped start)
        for b, j in enumerate(members):
            res = scipy_minimize(fun, starts[b], args=(int(j),), jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)),
                                 options=dict(maxfun=int(max_evals), gtol=pgtol, ftol=factr * np.finfo(float).eps))
            f0 = fun(starts[b], int(j))[0]
            X[b], f[b], n[b] = (res.x, res.fun, res.nfev) if res.fun <= f0 else (starts[b], f0, res.nfev)
        return X, sign * f, n
