"""TEST-ONLY: a dense NumPy restatement of what `bogp_sweep_believer_ehvi` defines (include/bogp.h), from a committed m-target state
as `Engine.get_state` returns it (fixed constant trend: the only one several targets take, so u = 0).

The recursion in correlation units is `support.believer_ref.BelieverRef`'s, shared by the m targets (the bracket of gpr.py:502-510):
    MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2),     mu_k(x) = beta + r(x) . gamma_k   unchanged
    MSE_k = 0 exactly on the candidate row that is a winner whose pivot passed the guard
The front: F_0 = pareto_front(front, ref_point); with `believe_front` every believed mean mu(p) joins it, F_B = pareto_front(F_{B-1} u
{mu(p_B)}, ref_point).  The cells of step j are `pareto.hypercell_bounds` of the front as it stands, the values `support.ehvi_ref64.ehvi`
(the reference's psi / nu algebra in float64).  Step j takes np.argmax over the rows that are not winners yet."""
import numpy as np

from bogp import pareto
from support.believer_ref import PIVOT_FLOOR, BelieverRef
from support.ehvi_ref64 import ehvi as ehvi_ref


class BelieverEhviRef:
    def __init__(self, X, theta, kernel, state):
        gamma = np.asarray(state["gamma"], float).reshape(len(X), -1)
        self.m = gamma.shape[1]
        self.gamma = gamma
        self.sigma2 = np.asarray(state["sigma2"], float).ravel()
        self.beta = float(state["beta"])
        one = dict(C=state["C"], gamma=gamma[:, 0], beta=self.beta, sigma2=self.sigma2[0])
        self.core = BelieverRef(X, theta, kernel, one, False)  # r, L^-1 r and the correlations

    def mean(self, P):
        return self.beta + self.core.corr(P, self.core.X) @ self.gamma

    def run(self, Xs, front, ref_point, q, pending=None, believe_front=True, evaluate=True):
        """The q steps over the candidates Xs.  Returns a dict: best_val, best_idx (q), best_x (q, d), best_mu (q, m), pivots (n + q),
        n_cells (q), ehvi (q, M), mse (q, M, m), mu (M, m), second (q: the runner-up value of each step among the rows that compete),
        cells (q pairs (lower, upper)), s (n + q + 1, M: the unclamped bracket after B believed points, started from max(0, s_0))."""
        core = self.core
        Xs = np.ascontiguousarray(Xs, dtype=float)
        M, m = len(Xs), self.m
        r = np.asarray(ref_point, float).ravel()
        pend = np.zeros((0, Xs.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, float))
        rx, rt_x, _, _ = core.terms(Xs)
        mu = self.beta + rx @ self.gamma
        s = np.maximum(0.0, 1.0 - (rt_x**2).sum(axis=0))  # pass 0's clamp (it changes nothing that is returned: s only decreases)
        s_hist = [s.copy()]
        F = pareto.pareto_front(np.asarray(front, float).reshape(-1, m), r)
        pts, cols, pivots = [], [], []

        def believe(x, mu_p, row=None):
            nonlocal s, F
            _, rt_p, _, _ = core.terms(x)
            rt_p = rt_p[:, 0]
            cp = []
            for k, pk in enumerate(pts):
                b = float(core.corr(x, pk["x"])[0, 0]) - rt_p @ pk["rt"] - sum(cp[l] * pk["c"][l] for l in range(k))
                cp.append(b / pk["root"] if pk["root"] > 0 else 0.0)
            piv = 1.0 - rt_p @ rt_p - sum(c * c for c in cp)
            pivots.append(piv)
            root = np.sqrt(piv) if piv > PIVOT_FLOOR else 0.0
            if root > 0:
                b = core.corr(Xs, x)[:, 0] - rt_x.T @ rt_p
                for k in range(len(pts)):
                    b = b - cols[k] * cp[k]
                c = b / root
            else:
                c = np.zeros(M)
            cols.append(c)
            pts.append(dict(x=np.asarray(x, float), rt=rt_p, root=root, c=cp))
            s = s - c * c
            if row is not None and root > 0:
                s[row] = 0.0
            s_hist.append(s.copy())
            if believe_front:
                F = pareto.pareto_front(np.vstack([F, np.asarray(mu_p, float).reshape(1, m)]), r)

        for x in pend:
            believe(x, self.mean(x)[0])
        out = dict(best_val=np.empty(q), best_idx=np.empty(q, dtype=np.int64), best_mu=np.empty((q, m)), n_cells=np.empty(q, dtype=np.int64),
                   ehvi=np.empty((q, M)), mse=np.empty((q, M, m)), second=np.empty(q), mu=mu, cells=[])  # fmt: skip
        for j in range(q):
            mse = np.maximum(0.0, s)[:, None] * self.sigma2[None, :]
            lo, hi = pareto.hypercell_bounds(F, r)
            v = ehvi_ref(mu, mse, lo, hi) if evaluate else np.zeros(M)
            free = np.ones(M, bool)
            free[out["best_idx"][:j]] = False
            rows = np.flatnonzero(free)
            i = int(rows[np.argmax(v[free])])
            out["ehvi"][j], out["mse"][j], out["best_idx"][j], out["best_val"][j] = v, mse, i, v[i]
            out["best_mu"][j], out["n_cells"][j] = mu[i], len(lo)
            out["cells"].append((lo, hi))
            free[i] = False
            out["second"][j] = np.max(v[free]) if free.any() else -np.inf
            believe(Xs[i], mu[i], i)
        out["best_x"] = Xs[out["best_idx"]].copy()
        out["pivots"] = np.array(pivots)
        out["s"] = np.array(s_hist)
        return out
