"""TEST-ONLY: a dense NumPy restatement of what `bogp_sweep_believer_ehvi_constrained` defines (include/bogp.h), from a committed
(m + c)-target state as `Engine.get_state` returns it (fixed constant trend: the only one several targets take, so u = 0).

The recursion in correlation units is `support.believer_constrained_ref.BelieverConstrainedRef`'s, shared by the m + c targets:
    MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2),     mu_k(x) = beta + r(x) . gamma_k   unchanged
    MSE_k = 0 exactly on the candidate row that is a winner whose pivot passed the guard
The criterion of step j is `support.constrained_ehvi_ref.values` on these moments over the cells (`bogp.pareto.hypercell_bounds`) of the
feasible front as it stands; no cells at all for a feasibility-only call, in every step.  The front: F_0 = pareto_front(front,
ref_point); with `believe_front` (and not `feasibility_only`) the objective part of a believed mean joins it if and only if every
constraint mean lies in its closed interval [lo_j, hi_j]; an infeasible one conditions the variances only.  Step j takes np.argmax over
the rows that are not winners yet."""
import numpy as np

from bogp import pareto
from support import constrained_ehvi_ref as R
from support.believer_ehvi_ref import BelieverEhviRef
from support.believer_ref import PIVOT_FLOOR


def cells_of(F, r, feasibility_only=False):
    m = len(r)
    if feasibility_only:
        return np.zeros((0, m)), np.zeros((0, m))
    lower, upper = pareto.hypercell_bounds(np.asarray(F, float).reshape(-1, m), r)
    return np.atleast_2d(lower), np.atleast_2d(upper)


class BelieverConstrainedEhviRef(BelieverEhviRef):
    def run(self, Xs, front, ref_point, q, lo, hi, pending=None, believe_front=True, feasibility_only=False):
        """The q steps over the candidates Xs.  Returns a dict: best_val, best_idx (q), best_x (q, d), best_mu (q, m + c), pivots (n + q),
        n_cells (q), val (q, M), pof (q, M), mse (q, M, m + c), mu (M, m + c), second (q: the runner-up value of each step among the rows
        that compete), cells (q pairs (lower, upper)), and about the believed points that stand before a step, in order (n + q - 1):
        believed_mu (B, m + c), feasible (B: every constraint mean inside its interval), nondominated (B: the objective part lies above
        ref_point and no point of the front as it stood dominates or equals it), fronts (B + 1: the front before the first and behind
        each)."""
        core = self.core
        Xs = np.ascontiguousarray(Xs, dtype=float)
        M, mt = len(Xs), self.m
        r = np.asarray(ref_point, float).ravel()
        m = len(r)
        lo, hi = np.asarray(lo, float).ravel(), np.asarray(hi, float).ravel()
        assert mt == m + len(lo) and len(lo) == len(hi)
        pend = np.zeros((0, Xs.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, float))
        rx, rt_x, _, _ = core.terms(Xs)
        mu = self.beta + rx @ self.gamma
        s = np.maximum(0.0, 1.0 - (rt_x**2).sum(axis=0))  # pass 0's clamp (it changes nothing that is returned: s only decreases)
        F = pareto.pareto_front(np.asarray(front, float).reshape(-1, m), r)
        pts, cols, pivots = [], [], []
        believed_mu, feasible, nondominated, fronts = [], [], [], [F.copy()]

        def believe(x, mu_p, row=None, last=False):
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
            if last:  # the last winner: its pivot alone is reported
                return
            mu_p = np.asarray(mu_p, float).ravel()
            ok = bool(np.all((lo <= mu_p[m:]) & (mu_p[m:] <= hi)))
            y = mu_p[:m]
            free = bool(np.all(y > r)) and not np.any(np.all(F >= y, axis=1))
            believed_mu.append(mu_p.copy()), feasible.append(ok), nondominated.append(free)
            if believe_front and not feasibility_only and ok:
                F = pareto.pareto_front(np.vstack([F, y.reshape(1, m)]), r)
            fronts.append(F.copy())

        for x in pend:
            believe(x, self.mean(x)[0])
        out = dict(best_val=np.empty(q), best_idx=np.empty(q, dtype=np.int64), best_mu=np.empty((q, mt)), n_cells=np.empty(q, dtype=np.int64),
                   val=np.empty((q, M)), pof=np.empty((q, M)), mse=np.empty((q, M, mt)), second=np.empty(q), mu=mu, cells=[])  # fmt: skip
        for j in range(q):
            mse = np.maximum(0.0, s)[:, None] * self.sigma2[None, :]
            lower, upper = cells_of(F, r, feasibility_only)
            v, P = R.values(mu, mse, self.sigma2, m, lower, upper, lo, hi)
            free = np.ones(M, bool)
            free[out["best_idx"][:j]] = False
            rows = np.flatnonzero(free)
            i = int(rows[np.argmax(v[free])])
            out["val"][j], out["pof"][j], out["mse"][j], out["best_idx"][j], out["best_val"][j] = v, P, mse, i, v[i]
            out["best_mu"][j], out["n_cells"][j] = mu[i], len(lower)
            out["cells"].append((lower, upper))
            free[i] = False
            out["second"][j] = np.max(v[free]) if free.any() else -np.inf
            believe(Xs[i], mu[i], i, last=j == q - 1)
        out["best_x"] = Xs[out["best_idx"]].copy()
        out["pivots"] = np.array(pivots)
        out["believed_mu"] = np.array(believed_mu).reshape(-1, mt)
        out["feasible"], out["nondominated"], out["fronts"] = np.array(feasible, bool), np.array(nondominated, bool), fronts
        return out
