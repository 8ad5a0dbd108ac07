"""The cases of Thompson batches under modelled constraints, shared by tests/test_gpu_thompson_constrained.py (the device against the
restatement) and tests/test_thompson_constrained_host.py (which asserts, on the restatement alone, the conditions that keep the device
test from hiding a failure).  No test lives here.

`problem` is tests/test_gpu_thompson.py's generator extended to m sine columns (the same stream: X, then per column its direction and
noise, then the candidates).  The model is committed in the noiseless mode with the FIXED constant trend beta = 0.3, as every
multi-target model is.

Allowance of a path value (ledger T16's form): |dev - ref| <= ptol (|ref| + A), ptol = max(1e-6, 100 cond(R) eps), A the sum of the
absolute terms the device adds up, sqrt(2 sigma2_t / L) sum_l |W_l| + sum_n |r_n (gamma_t - g)_n| + |beta|."""
from types import SimpleNamespace

import numpy as np

from bogp import _lib, thompson

EPS = np.finfo(float).eps
BETA = 0.3
NU = 0.8
KERNELS = [_lib.KERNEL_SE, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP, _lib.KERNEL_MATERN_NU]
HEAVY = (_lib.KERNEL_MATERN12, _lib.KERNEL_ABSEXP, _lib.KERNEL_MATERN_NU)  # spectral draws with Cauchy-like tails

MS, DS, NS, LS = [1, 15, 16, 17, 63, 64, 65, 1000], [1, 3, 4, 5, 20, 33], [5, 64, 67, 300], [16, 48, 1024]
MQ = [(2, 1), (2, 8), (3, 5), (4, 4), (5, 3), (8, 2), (8, 1)]  # 16 columns, 15 columns and fewer
# 28 shapes: every value of every parameter several times, in changing company; all six kernels, both directions
SHAPES = [(MS[i % 8], DS[(i + i // 8) % 6], NS[(i + i // 4) % 4], LS[(i // 2) % 3]) + MQ[(i // 3 + i) % 7] + (KERNELS[(i + i // 6) % 6], bool((i // 4) % 2))
          for i in range(28)]  # fmt: skip

# The selection cases (M = 1000, L = 48, q = 16 // m): name -> (m, N, d, kernel, minimize, bounds, seed of the draw).  "median": lo =
# -inf, hi = the training median of each constraint column (a "mixed" case: feasible and infeasible rows for every member); "none":
# no row can be feasible (lo = hi = 50, far above every path); "open": infinite bounds, every row feasible.  The seeds are chosen so
# that the conditions of tests/test_thompson_constrained_host.py hold; they are asserted there, not assumed.
CASES = {
    "m2-mixed": (2, 67, 3, _lib.KERNEL_MATERN52, True, "median", 1),
    "m3-mixed": (3, 5, 1, _lib.KERNEL_SE, False, "median", 3),
    "m4-mixed": (4, 300, 20, _lib.KERNEL_ABSEXP, True, "median", 0),
    "m5-mixed": (5, 300, 3, _lib.KERNEL_SE, False, "median", 9),
    "m8-mixed": (8, 64, 4, _lib.KERNEL_MATERN12, True, "median", 8),
    "m3-none": (3, 67, 3, _lib.KERNEL_MATERN52, True, "none", 3),
    "m2-open": (2, 67, 3, _lib.KERNEL_MATERN12, False, "open", 1),
}
MIXED = [n for n in CASES if n.endswith("mixed")]
CASE_M, CASE_L = 1000, 48


def problem(M, d, N, kernel, m, seed=0):
    """(X, Y (N, m), theta, candidates): test_gpu_thompson.problem with m sine columns."""
    rng = np.random.default_rng(1000 * N + 10 * d + seed)
    X = rng.uniform(-2, 2, size=(N, d))
    Y = np.column_stack([2 * np.sin(X @ rng.normal(size=d) / np.sqrt(d)) + 0.1 * rng.normal(size=N) for _ in range(m)])
    nn = 4.0 / N ** (1.0 / d)  # spacing of N points in the box, per dimension
    theta = np.full(d, 1.0 / d) if kernel in HEAVY else np.full(d, (3.0 if kernel == _lib.KERNEL_SE else 1.0) / (d * nn * nn))
    Xs = rng.uniform(-2.2, 2.2, size=(M, d))
    n_near = min(M, N, 8)
    Xs[:n_near] = X[:n_near] + 0.01
    return X, Y, theta, Xs


def bounds(kind, Y):
    n_con = Y.shape[1] - 1
    if kind == "median":
        return np.full(n_con, -np.inf), np.median(Y[:, 1:], axis=0)
    if kind == "none":
        return np.full(n_con, 50.0), np.full(n_con, 50.0)
    return np.full(n_con, -np.inf), np.full(n_con, np.inf)


def state(X, Y, theta, kernel, sigma2=None):
    """The dense multi-target state: sigma2 as the engine committed it, or concentrated (the host twin has no engine)."""
    return thompson.dense_state_multi(X, Y, theta, kernel, beta=BETA, nu=NU if kernel == _lib.KERNEL_MATERN_NU else None, sigma2=sigma2)


def restate(st, dr, Xs):
    """The restatement with its allowances: paths (q, m, M), gt (N, q m), tol (q, m, M), tol_g (N, q m), the conditioning term's share
    of the allowance, ptol, cond(R) and the largest phase."""
    finite = np.all(np.isfinite(Xs), axis=1)
    Xf = np.where(finite[:, None], Xs, 0.0)
    m = st.y.shape[1]
    qm = dr.weights.shape[1]
    q, L = qm // m, len(dr.phase)
    R = thompson.correlation(st, st.X, st.X)
    cond = float(np.linalg.cond(R))
    phase = float(np.max(np.abs(Xf) @ np.abs(dr.omega).T + np.abs(dr.phase)))
    ptol = max(1e-6, 100 * cond * EPS)
    paths, gt = thompson.paths_multi_numpy(st, dr, Xs)
    S = np.tile(np.sqrt(2 * st.sigma2 / L), q) * np.abs(dr.weights).sum(axis=0)  # (q m,)
    r = thompson.correlation(st, Xf, st.X)
    gamma = np.tile(np.linalg.solve(R, st.y - st.beta), (1, q))
    cterm = (np.abs(r) @ np.abs(gamma - gt)).T  # (q m, M)
    A = S[:, None] + cterm + abs(st.beta)
    tol = ptol * (np.abs(paths.reshape(qm, -1)) + A)
    tol[:, ~finite] = np.inf
    A_g = np.abs(np.linalg.inv(R)).sum(axis=1)[:, None] * S[None, :]
    return SimpleNamespace(paths=paths, gt=gt, tol=tol.reshape(q, m, -1), tol_g=ptol * (np.abs(gt) + A_g), share=float(np.max(cterm / A)),
                           ptol=ptol, cond=cond, phase=phase)  # fmt: skip


def case(name, sigma2=None):
    """Everything a selection case needs but the engine: (X, Y, theta, Xs, kernel, minimize, lo, hi, q, state, draw)."""
    m, N, d, kernel, minimize, kind, seed = CASES[name]
    X, Y, theta, Xs = problem(CASE_M, d, N, kernel, m)
    lo, hi = bounds(kind, Y)
    st = state(X, Y, theta, kernel, sigma2)
    q = 16 // m
    return SimpleNamespace(X=X, Y=Y, theta=theta, Xs=Xs, kernel=kernel, minimize=minimize, lo=lo, hi=hi, q=q, m=m, st=st,
                           dr=thompson.draw_multi(st, q, CASE_L, seed=seed))  # fmt: skip


def conditions(c, ref, n_rank=17):
    """What must hold on the restatement for the device's winners to be the restatement's: per member (a) consecutive gaps among the
    n_rank best rows of A (and, in a case without a feasible row, of B) exceed the sum of the two rows' allowances, (b) no row whose
    constraint path lies within its allowance of a bound has an objective value above rank n_rank's minus its allowance.  Returns a
    list of violations (empty: the case is decided)."""
    sel = thompson.select_numpy(ref.paths, c.lo, c.hi, c.st.sigma2, c.minimize, n_rank)
    inv_sd = 1.0 / np.sqrt(c.st.sigma2)
    bad = []
    for j in range(c.q):
        crit = -ref.paths[j, 0] if c.minimize else ref.paths[j, 0]
        near = np.zeros(ref.paths.shape[2], dtype=bool)
        for t in range(1, c.m):
            near |= np.abs(ref.paths[j, t] - c.lo[t - 1]) <= ref.tol[j, t]
            near |= np.abs(ref.paths[j, t] - c.hi[t - 1]) <= ref.tol[j, t]
        va, ia = sel["best_val"][j, 0], sel["best_idx"][j, 0]
        n_feas = int(np.sum(va > -np.inf))
        for r in range(min(n_feas, n_rank) - 1):
            if not va[r] - va[r + 1] > ref.tol[j, 0, ia[r]] + ref.tol[j, 0, ia[r + 1]]:
                bad.append("member %d: A ranks %d and %d are a near-tie" % (j, r, r + 1))
        floor = va[n_rank - 1] if n_feas >= n_rank else -np.inf
        hit = near & (crit + ref.tol[j, 0] >= floor)
        if hit.any():
            bad.append("member %d: row %d stands at a bound and could enter the ranking" % (j, int(np.argmax(hit))))
        if n_feas == 0:  # B decides: its gaps against the allowances of the constraint values, scaled as the violation is
            vb, ib = sel["best_val"][j, 1], sel["best_idx"][j, 1]
            allow = np.max(ref.tol[j, 1:] * inv_sd[1:, None], axis=0)
            for r in range(n_rank - 1):
                if not vb[r] - vb[r + 1] > allow[ib[r]] + allow[ib[r + 1]]:
                    bad.append("member %d: B ranks %d and %d are a near-tie" % (j, r, r + 1))
    return bad
