"""TEST-ONLY: a dense NumPy restatement of the Kriging-believer recursion that `bogp_sweep_believer` defines (include/bogp.h),
from a committed state as `Engine.get_state` returns it.  Constant trend basis.

    kappa0(x, x') = k(x, x') - r(x)^T R^-1 r(x') + u(x) u(x'),     u = (Ft . L^-1 r - 1) / G under ordinary kriging, else 0
    b_i(x) = kappa0(x, p_i) - sum_{k<i} c_k(x) c_k(p_i),  pivot_i = b_i(p_i),  c_i = b_i / sqrt(pivot_i)  (0 if pivot_i <= 1e-12)
    s_i(x) = s_{i-1}(x) - c_i(x)^2,  s_0(x) = kappa0(x, x),   MSE_j = sigma2 max(0, s_B),   mean mu(x) = beta + r(x) . gamma
    s_i = 0 exactly on the candidate row that is the winner p_i (c_i(p_i)^2 = pivot_i = s_{i-1}(p_i))

A candidate row that is a winner keeps its criterion value but leaves the argmax of the later steps.
`r` is the RAW cross-correlation and L the factor of the committed (normalised, in the noisy modes) R, as gpr.py:486-510 uses
them.  Step j maximises criterion j (the oracle's vectorised functions) with np.argmax's rule; with `believe_plugin` the plugin
is the least of the given one and the believed means in the criterion's sign (y_hat = mu when minimising, -mu otherwise)."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

PIVOT_FLOOR = 1e-12


class BelieverRef:
    def __init__(self, X, theta, kernel, state, estimate_trend):
        """`state`: C, gamma, Ft, G, beta, sigma2 of the committed model (Engine.get_state); `theta` as committed (with the
        kernel's exponent / order behind it where it has one)."""
        self.X = np.ascontiguousarray(X, dtype=float)
        self.theta, self.kernel = np.asarray(theta, dtype=float), int(kernel)
        self.C, self.gamma = np.asarray(state["C"], float), np.asarray(state["gamma"], float).ravel()
        self.est = bool(estimate_trend)
        self.Ft = np.asarray(state["Ft"], float).ravel() if self.est else None
        self.G = float(state["G"]) if self.est else 0.0
        self.beta, self.sigma2 = float(state["beta"]), float(state["sigma2"])

    # -- per-point ingredients -------------------------------------------------------------------------------------------------
    def corr(self, A, B):
        return O.corr(self.kernel, self.theta, O.l1_cross_distances(np.atleast_2d(A), np.atleast_2d(B))).reshape(len(np.atleast_2d(A)), -1)

    def terms(self, P):
        """r (m, N), rt = L^-1 r (N, m), u (m,), mu (m,) of the rows P"""
        r = self.corr(P, self.X)
        rt = solve_triangular(self.C, r.T, lower=True)
        u = (self.Ft @ rt - 1.0) / self.G if self.est else np.zeros(len(r))
        return r, rt, u, self.beta + r @ self.gamma

    def run(self, Xs, acq, plugin, minimize=True, pending=None, believe_plugin=True):
        """The q steps over the candidates Xs.  Returns a dict: best_val, best_idx (q), best_x (q, d), pivots (n + q), acq, mse (q, M),
        mu (M), second (q: the runner-up value of each step among the rows that compete), s (n + q + 1, M: the unclamped s_B after B
        believed points), s_own (q: the recursion's own, unforced s at each winner's row right after it was believed)."""
        Xs = np.ascontiguousarray(Xs, dtype=float)
        M, q = len(Xs), len(acq)
        pend = np.zeros((0, Xs.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, float))
        _, rt_x, u_x, mu = self.terms(Xs)
        s = 1.0 - (rt_x**2).sum(axis=0) + u_x**2
        s_hist = [s.copy()]
        pts = []  # believed so far: dict(x, rt, u, root, c: c_k(p) for k < its index)
        cols = []  # c_k over the candidates
        pivots = []
        s_own = []
        plug = float(plugin)

        def believe(x, mu_p, row=None):
            nonlocal s, plug
            _, rt_p, u_p, mu_own = self.terms(x)
            rt_p, u_p = rt_p[:, 0], float(u_p[0])
            if believe_plugin:
                m = float(mu_own[0]) if mu_p is None else float(mu_p)
                plug = min(plug, m if minimize else -1 * m)
            # c_k(p) for the points before, then the pivot
            cp = []
            for k, pk in enumerate(pts):
                b = float(self.corr(x, pk["x"])[0, 0]) - rt_p @ pk["rt"] + u_p * pk["u"] - sum(cp[l] * pk["c"][l] for l in range(k))
                cp.append(b / pk["root"] if pk["root"] > 0 else 0.0)
            piv = 1.0 - rt_p @ rt_p + u_p * u_p - sum(c * c for c in cp)
            pivots.append(piv)
            root = np.sqrt(piv) if piv > PIVOT_FLOOR else 0.0
            if root > 0:
                b = self.corr(Xs, x)[:, 0] - rt_x.T @ rt_p + u_x * u_p
                for k in range(len(pts)):
                    b = b - cols[k] * cp[k]
                c = b / root
            else:
                c = np.zeros(M)
            cols.append(c)
            pts.append(dict(x=np.asarray(x, float), rt=rt_p, u=u_p, root=root, c=cp))
            s = s - c * c
            if row is not None:
                s_own.append(float(s[row]))
            if row is not None and root > 0:
                s[row] = 0.0  # the believed candidate row is determined: c(p)^2 = pivot = s(p) exactly
            s_hist.append(s.copy())

        for x in pend:
            believe(x, None)
        out = dict(best_val=np.empty(q), best_idx=np.empty(q, dtype=np.int64), acq=np.empty((q, M)), mse=np.empty((q, M)),
                   second=np.empty(q), mu=mu)  # fmt: skip
        for j, (a, par) in enumerate(acq):
            mse = self.sigma2 * np.maximum(0.0, s)
            v = O.acquisition(a, par, mu, mse, plug, self.sigma2, minimize)
            free = np.ones(M, bool)
            free[out["best_idx"][:j]] = False  # the winners before do not compete again
            rows = np.flatnonzero(free)
            i = int(rows[np.argmax(v[free])])
            out["acq"][j], out["mse"][j], out["best_idx"][j], out["best_val"][j] = v, mse, i, v[i]
            free[i] = False
            out["second"][j] = np.max(v[free]) if free.any() else -np.inf
            believe(Xs[i], mu[i], i)  # (the last winner too: its pivot is reported)
        out["best_x"] = Xs[out["best_idx"]].copy()
        out["pivots"] = np.array(pivots)
        out["s"] = np.array(s_hist)
        out["s_own"] = np.array(s_own)
        return out
