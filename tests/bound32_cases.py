"""Shared by tests/test_bound32_host.py and tests/test_gpu_bound32.py (not a test module): a float32 NumPy restatement of the FP32
bounding stage of the one-pass pruned sweep (csrc/kernels_bound32.hip) -- rounding of the inputs, the fma
chain of the cross term, the clamped squared distance, profile, FP32 accumulation in runs of 16 terms with an FP64 tail -- beside the
same sums in FP64, the margins through the library's host wrapper, and the stage's flags against the pilot's thresholds."""
import ctypes as C

import numpy as np
from scipy.linalg import solve_triangular

import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

F32 = np.float32
SLOPE = {O.KERNEL_SE: 1.0, O.KERNEL_MATERN32: 1.5, O.KERNEL_MATERN52: 5.0 / 6.0}


def model(kernel=PC.KERNEL, ordinary=False, d=PC.DIM, nugget=PC.NOISE, seed=0, n=PC.N_TRAIN):
    """PC.model's quadratic bowl for any of the three kernels, any dimension and nugget (d = 3, Matern-5/2, 1e-6: PC.model itself)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-5, 5, size=(n, d))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    par = np.r_[np.full(d, 0.05), 0.01]
    st = O.make_state(par, X, y, kernel, O.MODE_NOISY, nugget, estimate_trend=ordinary, beta=None if ordinary else 0.0)
    return X, y, par, st


def special_rows(X, d):
    """a training point itself, a point 1e-4 from one, the box corners, a row at 1e3"""
    corners = np.array(np.meshgrid(*[[-5.0, 5.0]] * min(d, 3))).reshape(min(d, 3), -1).T
    corners = np.hstack([corners, np.full((len(corners), d - corners.shape[1]), 5.0)])
    return np.vstack([X[17], X[40] + 1e-4 / np.sqrt(d), corners, np.full(d, 1e3)])


def _fma32(a, b, c):
    """float32 fma of float32 arrays: the product of two float32 is exact in float64, the sum is rounded to 53 and then to 24 bits"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def profile32(kernel, s):
    log2e = F32(-1.44269504)
    if kernel == O.KERNEL_SE:
        return np.exp2(s * log2e).astype(F32)
    dist = np.sqrt(s).astype(F32)
    if kernel == O.KERNEL_MATERN32:
        K = (dist * F32(1.73205081)).astype(F32)
        return ((F32(1.0) + K).astype(F32) * np.exp2(K * log2e).astype(F32)).astype(F32)
    K = (dist * F32(2.23606798)).astype(F32)
    p = _fma32(K, _fma32(K, np.full_like(K, F32(0.333333333)), np.ones_like(K)), np.ones_like(K))
    return (p * np.exp2(K * log2e).astype(F32)).astype(F32)


def vectors(st):
    """gamma and w = L^-T Ft (zeros under simple kriging) of the state, as the device holds them"""
    N = st.X.shape[0]
    g = np.asarray(st.gamma, dtype=np.float64)[:, 0]
    w = solve_triangular(st.C.T, st.Ft[:, 0], lower=False) if st.estimate_trend else np.zeros(N)
    return g, w


def restate(st, Xs):
    """-> dict: mu32, wd32 (the stage's sums, float64 arrays), mu64, wd64 (the same sums in FP64), na, gamma_l1, w_l1, nb_max"""
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    M, d = Xs.shape
    N = st.X.shape[0]
    rt = np.sqrt(st.theta) * np.ones(d)
    a, b = Xs * rt, st.X * rt
    na, nb = np.zeros(M), np.zeros(N)
    for k in range(d):  # dimension order, as the device sums them
        na, nb = a[:, k] * a[:, k] + na, b[:, k] * b[:, k] + nb
    g, w = vectors(st)
    # FP64 sums
    with np.errstate(all="ignore"):
        r64 = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs, st.X)).reshape(M, N)
    mu64, wd64 = r64.dot(g), r64.dot(w)
    # the stage in float32
    Npad = (N + 63) // 64 * 64
    a32, b32 = a.astype(F32), np.zeros((Npad, d), dtype=F32)
    b32[:N] = b.astype(F32)
    na32, nb32, g32, w32 = na.astype(F32), np.zeros(Npad, F32), np.zeros(Npad, F32), np.zeros(Npad, F32)
    nb32[:N], g32[:N], w32[:N] = nb.astype(F32), g.astype(F32), w.astype(F32)
    with np.errstate(all="ignore"):
        c = np.zeros((M, Npad), dtype=F32)
        for k in range(d):
            c = _fma32(a32[:, k : k + 1], b32[None, :, k], c)
        nab = (na32[:, None] + nb32[None, :]).astype(F32)
        s = np.maximum(_fma32(np.full_like(c, F32(-2.0)), c, nab), F32(0.0))
        r = profile32(st.kernel, s)
        # lane (g4, lk) of wave g4 chains n = 64 it + 16 g4 + 4 lk + c over c, then it, and empties into FP64 every 4 steps
        r5 = r.reshape(M, Npad // 64, 4, 4, 4)
        out = []
        for v32 in (g32, w32):
            v5 = v32.reshape(Npad // 64, 4, 4, 4)
            tot = np.zeros((M, 4, 4))
            acc = np.zeros((M, 4, 4), dtype=F32)
            for it in range(Npad // 64):
                for cc in range(4):
                    acc = _fma32(r5[:, it, :, :, cc], np.broadcast_to(v5[it, :, :, cc], (M, 4, 4)), acc)
                if it % 4 == 3 or it == Npad // 64 - 1:
                    tot += acc.astype(np.float64)
                    acc = np.zeros((M, 4, 4), dtype=F32)
            out.append(tot.sum(axis=2).sum(axis=1))
    return dict(mu32=out[0], wd32=out[1], mu64=mu64, wd64=wd64, na=na, gamma_l1=float(np.abs(g).sum()), w_l1=float(np.abs(w).sum()),
                nb_max=float(nb.max()))  # fmt: skip


def margins(kernel, d, na, nb_max, gamma_l1, w_l1):
    lib = _lib.load()
    e_mu, e_w = np.empty(len(na)), np.empty(len(na))
    a, b = C.c_double(), C.c_double()
    for i, v in enumerate(na):
        assert lib.bogp_bound32_margin(int(kernel), int(d), float(v), float(nb_max), float(gamma_l1), float(w_l1), C.byref(a), C.byref(b)) == 0
        e_mu[i], e_w[i] = a.value, b.value
    return e_mu, e_w


def interval_bound(a_id, par, y_hat, e, sd_ub, plugin, s2):
    return float(_lib.load().bogp_acq_upper_bound_interval(int(a_id), float(par), float(y_hat), float(e), float(sd_ub), float(plugin), float(s2)))


INTERVAL_PARS = {0: (0.0,), 1: (0.0, 0.05, 0.5, 1.5), 2: (0.5, 8.0, 50.0), 3: (0.5, 2.0, 10.0, 30.0)}  # by criterion id


def interval_cases(a_id, minimize, trials=60, tail_trials=12, ulp_trials=24):
    """(sigma2, plugin, y_hat, e, sd_ub) of the interval bound's domination property (tests/test_bound32_host.py on the host wrappers,
    tests/test_gpu_criteria.py on the device): random intervals, every fifth around the plugin and every fifth around 0; then
    `tail_trials` intervals around z = (plugin - y_hat) / sd_ub in [-37, -20], narrow enough to stay clear of the plugin; then
    `ulp_trials` intervals 1 to 4 ulp of y_hat wide on either side."""
    rng = np.random.default_rng(23 + a_id + 10 * minimize)
    for trial in range(trials):
        s2 = float(10.0 ** rng.uniform(-4, 1))
        plugin = float(rng.normal(0, 2))
        y_hat = float(rng.normal(0, 2)) * (1 if minimize else -1)
        e = float(10.0 ** rng.uniform(-8, 0.5))
        if trial % 5 == 0:
            y_hat = plugin + float(rng.uniform(-1, 1)) * e  # the plugin inside the interval
        if trial % 5 == 1:
            y_hat = float(rng.uniform(-1, 1)) * e           # 0 inside the interval
        sd_ub = float(np.sqrt(s2 * (1.0 + rng.uniform(0, 2) ** 2)))
        yield s2, plugin, y_hat, e, sd_ub
    rng = np.random.default_rng(323 + a_id + 10 * minimize)
    for trial in range(tail_trials):
        s2 = float(10.0 ** rng.uniform(-4, 1))
        plugin = float(rng.normal(0, 2))
        sd_ub = float(np.sqrt(s2 * (1.0 + rng.uniform(0, 2) ** 2)))
        y_hat = float(plugin - rng.uniform(-37.0, -20.0) * sd_ub)
        yield s2, plugin, y_hat, float(10.0 ** rng.uniform(-8, 0) * sd_ub), sd_ub
    for trial in range(ulp_trials):  # intervals of a few ulp of y_hat: what the bound's 1e-12 raise is for, a dip of erf / erfc / exp between the ends
        s2 = float(10.0 ** rng.uniform(-4, 1))
        plugin = float(rng.normal(0, 2))
        sd_ub = float(np.sqrt(s2 * (1.0 + rng.uniform(0, 2) ** 2)))
        y_hat = float(plugin + rng.uniform(0.05, 6.0) * sd_ub * (1 if trial % 3 else -1)) * (1 if minimize else -1)
        yield s2, plugin, y_hat, float((1 + trial % 4) * np.spacing(abs(y_hat))), sd_ub


def interval_points(y_hat, e):
    """201 points of [y_hat - e, y_hat + e], then both ends and the centre as the bound forms them"""
    return np.r_[np.linspace(y_hat - e, y_hat + e, 201), y_hat - e, y_hat + e, y_hat]


def stage1_flags(st, Xs, acq, plugin, minimize=True, pilot=PC.CHUNK_ROWS, rs=None):
    """The stage's flags for every row from the restatement's sums and margins, against the thresholds the pilot sets (k_bound32_flags'
    statements); and the exact test's flags (PC.surviving_fraction's) -> (flags32, flags64), both over all rows."""
    rs = rs or restate(st, Xs)
    d = Xs.shape[1]
    e_mu, e_w = margins(st.kernel, d, rs["na"], rs["nb_max"], rs["gamma_l1"], rs["w_l1"])
    s2 = float(st.sigma2[0])
    beta = float(np.ravel(st.beta)[0])
    mu = beta + rs["mu32"]
    u2 = ((np.abs(rs["wd32"] - 1.0) + e_w) / abs(float(st.G[0, 0]))) ** 2 if st.estimate_trend else 0.0
    sd_ub = np.sqrt((1.0 + u2) * s2) * (1.0 + 1e-12) * np.ones(len(Xs))
    y_hat = mu if minimize else -1 * mu
    e_y = e_mu + 1e-15 * np.abs(mu)
    mu_o, mse_o, sd_o = PC.oracle_rows(st, Xs)
    y_o = mu_o if minimize else -1 * mu_o
    lib = _lib.load()
    below32 = np.ones(len(Xs), dtype=bool)
    keep64 = np.zeros(len(Xs), dtype=bool)
    for a_id, a_par in acq:
        vals = O.acquisition(a_id, a_par, mu_o, mse_o, plugin, s2, minimize)
        thr = float(vals[:pilot][int(np.argmax(vals[:pilot]))])
        b32 = np.array([interval_bound(a_id, a_par, y, e, sd, plugin, s2) for y, e, sd in zip(y_hat, e_y, sd_ub)])
        below32 &= np.array([bool(lib.bogp_prune_below(float(b), thr)) for b in b32])
        b64 = PC.upper_bounds(a_id, a_par, y_o, sd_o, plugin, s2)
        keep64 |= ~(np.isfinite(thr) & (b64 + PC.prune_margin(b64, thr) < thr))
    return ~below32, keep64
