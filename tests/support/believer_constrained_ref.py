"""TEST-ONLY: a dense NumPy restatement of what `bogp_sweep_believer_constrained` defines (include/bogp.h), from a committed m-target
state as `Engine.get_state` returns it (fixed constant trend: the only one several targets take, so u = 0).

The recursion in correlation units is `support.believer_ehvi_ref.BelieverEhviRef`'s, shared by the m targets:
    MSE_{k,j}(x) = max(0, MSE_{k,0}(x) - sigma2_k sum_i c_i(x)^2),     mu_k(x) = beta + r(x) . gamma_k   unchanged
    MSE_k = 0 exactly on the candidate row that is a winner whose pivot passed the guard
The criterion of step j is `support.constrained_ref.constrained` on these moments with criterion j of the caller's list.  The plugin
(in the criterion's sign): a believed point whose means are feasible by belief -- lo_k <= mu_k(p) <= hi_k for every constraint -- lowers
it, plug = min(plug, +-mu_0(p)); an infeasible one leaves it.  Step j takes np.argmax over the rows that are not winners yet."""
import numpy as np

from support import constrained_ref as R
from support.believer_ehvi_ref import BelieverEhviRef
from support.believer_ref import PIVOT_FLOOR


class BelieverConstrainedRef(BelieverEhviRef):
    def run(self, Xs, acq, plugin, minimize, lo, hi, pending=None, believe_plugin=True):
        """The q = len(acq) steps over the candidates Xs.  Returns a dict: best_val, best_idx (q), best_x (q, d), best_mu (q, m), pivots
        (n + q), plugins (q), acq (q, M), pof (q, M), mse (q, M, m), mu (M, m), second (q: the runner-up value of each step among the
        rows that compete), and about the believed points in order (n + q - 1 of them stand before a step): believed_mu (B, m),
        lowered (B: feasible by belief and below the plugin), blocked (B: infeasible by belief and below the plugin)."""
        core = self.core
        acq = list(acq)
        q = len(acq)
        Xs = np.ascontiguousarray(Xs, dtype=float)
        M, m = len(Xs), self.m
        lo, hi = np.asarray(lo, float).ravel(), np.asarray(hi, float).ravel()
        pend = np.zeros((0, Xs.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, float))
        rx, rt_x, _, _ = core.terms(Xs)
        mu = self.beta + rx @ self.gamma
        s = np.maximum(0.0, 1.0 - (rt_x**2).sum(axis=0))  # pass 0's clamp (it changes nothing that is returned: s only decreases)
        pts, cols, pivots = [], [], []
        plug = float(plugin)
        believed_mu, lowered, blocked = [], [], []

        def believe(x, mu_p, row=None, last=False):
            nonlocal s, plug
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
            feasible = bool(np.all((lo <= mu_p[1:]) & (mu_p[1:] <= hi)))
            y_hat = mu_p[0] if minimize else -mu_p[0]
            believed_mu.append(mu_p.copy())
            lowered.append(feasible and y_hat < plug)
            blocked.append((not feasible) and y_hat < plug)
            if believe_plugin and feasible and y_hat < plug:
                plug = float(y_hat)

        for x in pend:
            believe(x, self.mean(x)[0])
        out = dict(best_val=np.empty(q), best_idx=np.empty(q, dtype=np.int64), best_mu=np.empty((q, m)), plugins=np.empty(q),
                   acq=np.empty((q, M)), pof=np.empty((q, M)), mse=np.empty((q, M, m)), second=np.empty(q), mu=mu)  # fmt: skip
        for j in range(q):
            mse = np.maximum(0.0, s)[:, None] * self.sigma2[None, :]
            vals, pof = R.constrained(mu, mse, self.sigma2, lo, hi, [acq[j]], plug, minimize)
            v = vals[0]
            free = np.ones(M, bool)
            free[out["best_idx"][:j]] = False
            rows = np.flatnonzero(free)
            i = int(rows[np.argmax(v[free])])
            out["acq"][j], out["pof"][j], out["mse"][j], out["best_idx"][j], out["best_val"][j] = v, pof, mse, i, v[i]
            out["best_mu"][j], out["plugins"][j] = mu[i], plug
            free[i] = False
            out["second"][j] = np.max(v[free]) if free.any() else -np.inf
            believe(Xs[i], mu[i], i, last=j == q - 1)
        out["best_x"] = Xs[out["best_idx"]].copy()
        out["pivots"] = np.array(pivots)
        out["believed_mu"] = np.array(believed_mu).reshape(-1, m)
        out["lowered"], out["blocked"] = np.array(lowered, bool), np.array(blocked, bool)
        return out
