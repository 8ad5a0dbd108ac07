"""Inputs shared by tests/test_gpu_prune.py and tests/test_prune_bounds_host.py (not a test module): the small models and
candidate sets of the pruned sweep's tests, and the oracle's view of them -- exact criterion values, the optimistic standard
deviation sd_ub = sqrt((1 + u^2) sigma2) and, through the library's host wrapper of acq_upper_bound, how many rows the bound
lets through against the threshold the pilot sets."""
import numpy as np
from scipy.linalg import solve_triangular

from bogp import _lib
from oracle import gp_oracle as O

N_TRAIN, DIM, M_CAND = 544, 3, 3001  # Np = 544 > 512: the chunked path; BOGP_CHUNK_MB=1 -> 192 rows a chunk, 16 chunks, the last ragged
CHUNK_ROWS = 192                      # (1 MiB / (544 rows x 8 bytes), rounded down to 64): also the pilot at this chunk size
KERNEL = 3                            # Matern 5/2
NOISE = 1e-6


def model(ordinary=False, seed=0):
    """A quadratic bowl in [-5, 5]^3 at pinned hyper-parameters: process variance 0.01 against standardised targets that span several
    units.  Far from the minimum no variance the prior allows lifts an improvement criterion to what the rows near the minimum reach
    (a peaked landscape), while the posterior deviation stays so far below the prior's that a UCB with multiplier 50 is within
    reach of every row (a flat one: 50 (sd_ub - sd) exceeds the whole range of the mean)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-5, 5, size=(N_TRAIN, DIM))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    par = np.r_[np.full(DIM, 0.05), 0.01]
    st = O.make_state(par, X, y, KERNEL, O.MODE_NOISY, NOISE, estimate_trend=ordinary, beta=None if ordinary else 0.0)
    return X, y, par, st


def candidates(seed=7, M=M_CAND):
    return np.random.default_rng(seed).uniform(-5, 5, size=(M, DIM))


def oracle_rows(st, Xs):
    """mu, MSE and sd_ub of every row: gp_oracle.predict's operations, with |L^-1 r|^2 dropped for sd_ub."""
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    M, N = Xs.shape[0], st.X.shape[0]
    r = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs, st.X)).reshape(M, N)
    mu = (O.trend_F(st.trend, Xs).dot(st.beta) + r.dot(st.gamma)).ravel()
    rt = solve_triangular(st.C, r.T, lower=True)
    if st.estimate_trend:
        u = solve_triangular(st.G.T, np.dot(st.Ft.T, rt) - O.trend_F(st.trend, Xs).T, lower=True)
    else:
        u = np.zeros((1, M))
    u2 = (u**2.0).sum(axis=0)
    s2 = float(st.sigma2[0])
    mse = np.maximum((1.0 - (rt**2.0).sum(axis=0) + u2) * s2, 0.0)
    sd_ub = np.sqrt(np.maximum((1.0 + u2) * s2, 0.0))
    return mu, mse, sd_ub


def upper_bounds(acq_id, par, y_hat, sd_ub, plugin, sigma2):
    lib = _lib.load()
    return np.array([lib.bogp_acq_upper_bound(int(acq_id), float(par), float(a), float(b), float(plugin), float(sigma2))
                     for a, b in zip(np.ravel(y_hat), np.ravel(sd_ub))])  # fmt: skip


def prune_margin(bound, thr):
    return 1e-9 * (np.abs(bound) + np.abs(thr)) + 1e-300


DOMINATION_PARS = {0: (0.0,), 1: (0.0, 0.05, 0.5, 1.5), 2: (0.5, 50.0, -0.5, -3.0), 3: (0.5, 2.0, 10.0, 30.0)}  # by criterion id


def sd_grid(sd_ub, s2):
    """[0, sd_ub] with both ends, the guard edges of EI (sd / sqrt(sigma2) = 1e-6) and MGFI (sd = 1e-8) and their neighbours, and
    the rungs 1 and 2 ulp under sd_ub."""
    edges = [0.0, 1e-8, np.nextafter(1e-8, 0), np.nextafter(1e-8, 1), 1e-6 * np.sqrt(s2), np.nextafter(1e-6 * np.sqrt(s2), 0),
             np.nextafter(1e-6 * np.sqrt(s2), 1), 1e-300, sd_ub, np.nextafter(sd_ub, 0), np.nextafter(np.nextafter(sd_ub, 0), 0)]  # fmt: skip
    g = np.r_[edges, sd_ub * np.linspace(0, 1, 41), sd_ub * np.logspace(-12, 0, 25)]
    return np.unique(g[(g >= 0) & (g <= sd_ub)])


def domination_cases(a_id, trials=120, tail_trials=24):
    """(sigma2, plugin, y_hat, sd_ub) of the domination property (tests/test_prune_bounds_host.py on the host wrappers,
    tests/test_gpu_criteria.py on the device): random values on both sides of plugin - y_hat and exactly on it, ranges that end inside
    the guards; then `tail_trials` rows with z = (plugin - y_hat) / sd_ub in [-37, -20], where Phi and phi amplify a rounding of z by z^2."""
    rng = np.random.default_rng(11 + a_id)
    for trial in range(trials):
        s2 = float(10.0 ** rng.uniform(-4, 1))
        plugin = float(rng.normal(0, 2))
        gap = float(10.0 ** rng.uniform(-6, 1.3) * np.sqrt(s2)) * (1 if trial % 2 else -1)  # y_hat below / above plugin
        y_hat = plugin - gap if trial % 7 else plugin                                     # ... and exactly on it
        sd_ub = float(np.sqrt(s2 * (1.0 + rng.uniform(0, 2) ** 2)))
        if trial % 11 == 0:
            sd_ub = float(10.0 ** rng.uniform(-10, -5))  # ranges that end inside the guards
        yield s2, plugin, y_hat, sd_ub
    rng = np.random.default_rng(311 + a_id)
    for trial in range(tail_trials):
        s2 = float(10.0 ** rng.uniform(-4, 1))
        plugin = float(rng.normal(0, 2))
        sd_ub = float(np.sqrt(s2 * (1.0 + rng.uniform(0, 2) ** 2)))
        yield s2, plugin, float(plugin - rng.uniform(-37.0, -20.0) * sd_ub), sd_ub


def surviving_fraction(st, Xs, acq, plugin, minimize=True, pilot=CHUNK_ROWS):
    """Rows behind the pilot that the prune test lets through when the thresholds are the pilot's best values (the device's thresholds
    only rise from there), as a fraction of all rows."""
    mu, mse, sd_ub = oracle_rows(st, Xs)
    s2 = float(st.sigma2[0])
    y_hat = mu if minimize else -1 * mu
    keep = np.zeros(len(Xs), dtype=bool)
    for a_id, a_par in acq:
        vals = O.acquisition(a_id, a_par, mu, mse, plugin, s2, minimize)
        thr = vals[:pilot][int(np.argmax(vals[:pilot]))]
        b = upper_bounds(a_id, a_par, y_hat, sd_ub, plugin, s2)
        pruned = np.isfinite(thr) & (b + prune_margin(b, thr) < thr)
        keep |= ~pruned
    return float(np.count_nonzero(keep[pilot:])) / len(Xs)


def place_winner(st, Xs, acq, plugin, where, minimize=True):
    """Xs with the oracle's winner of the first criterion moved to row `where` (swapped with the row that was there)."""
    mu, mse, _ = oracle_rows(st, Xs)
    vals = O.acquisition(acq[0][0], acq[0][1], mu, mse, plugin, float(st.sigma2[0]), minimize)
    w = int(np.argmax(vals))
    out = Xs.copy()
    out[[w, where]] = out[[where, w]]
    return out
