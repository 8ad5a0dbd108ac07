"""Inputs shared by tests/test_gpu_producer_a.py, tests/test_producer_cases_host.py and the cubic rows of
tests/test_gpu_driver.py (not a test module): the models and candidate stacks that hold the VALU correlation producer
(k_corr_chunk<KERNEL, PV>, csrc/kernels_posterior.hip) to the oracle where no other producer runs --
  family 1: PV == 0 with absolute_exponential, cubic, generalized_exponential and the general-nu Matern (no matrix-core producer,
            own dist_accumulate, own host pre-scaling of the coordinates: theta, theta^(1/p), sqrt(theta));
  family 2: PV == 16 / 32, a polynomial trend of 2 .. 32 columns under universal kriging fused into the producer, its boundaries
            p = 16 | 17 and 32 | 33 (from 33 columns on the trend travels as extra rows of the packed factor instead).
Everything is generated from seeds; the oracle's view of a case (state, posterior, criteria, winners) is computed once a process
and shared.  The preconditions that keep the device test from hiding a failure -- finite likelihood, cond(R) <= 1e9, a clear
winner for every criterion -- are asserted on the CPU by test_producer_cases_host.py: a case that misses one is replaced HERE.

Sizes.  Np = N rounded up to 32 rows; the producer cuts them into S = ceil(Np / 256) slices (one workgroup each, partial sums of mu
per slice); with BOGP_CHUNK_MB=1 a chunk holds floor(2^20 / (8 rows) / 64) * 64 candidates, rows = Np, or for the trend-rows path
Np rounded up to 256 plus p rounded up to 32.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import gp_oracle as O

NOISE = 1e-6
SIGMA2_PAR = 0.9
ACQ = ((O.ACQ_EI, 0.0), (O.ACQ_MGFI, 2.0), (O.ACQ_UCB, 0.5))
N_ON, N_NEAR, N_BOX, N_WIDE, N_FAR = 100, 100, 1500, 100, 64
M_STACK = N_ON + N_NEAR + N_BOX + N_WIDE + 1  # 1801 = 28 * 64 + 9: the last 64-candidate workgroup is ragged
# <= 32 candidates and a constant trend: k_batch_corr + k_gemm64 instead of the chunks.  The first 20 rows of the stack (all ON
# training points: the MSE is rounding noise, only mu, the MSE and the UCB winner compare) and 32 rows of the box (everything compares)
SMALL_M = 20
SMALL_BOX = slice(N_ON + N_NEAR, N_ON + N_NEAR + 32)

Case = namedtuple("Case", "family kernel N d theta extra trend")
_NAMES = {O.KERNEL_SE: "se", O.KERNEL_MATERN12: "m12", O.KERNEL_MATERN32: "m32", O.KERNEL_MATERN52: "m52", O.KERNEL_ABSEXP: "absexp",
          O.KERNEL_CUBIC: "cubic", O.KERNEL_GENEXP: "genexp", O.KERNEL_MATERN_NU: "matern_nu"}  # fmt: skip
_TRENDS = {O.TREND_CONSTANT: "", O.TREND_LINEAR: "-lin", O.TREND_QUADRATIC: "-quad"}


def case_id(c):
    return "%s%s%s-N%d-d%d" % (_NAMES[c.kernel], "" if c.extra is None else "(%g)" % c.extra, _TRENDS[c.trend], c.N, c.d)


def _family1():
    out = []
    big = [(600, 20), (530, 50), (1000, 7)]
    for N, d in big:
        out.append(Case(1, O.KERNEL_ABSEXP, N, d, 0.3 / d, None, O.TREND_CONSTANT))
    out.append(Case(1, O.KERNEL_ABSEXP, 777, 1, 50.0, None, O.TREND_CONSTANT))
    for p in (1.5, 0.7):
        for N, d in big:
            out.append(Case(1, O.KERNEL_GENEXP, N, d, 0.3 / d, p, O.TREND_CONSTANT))
    out.append(Case(1, O.KERNEL_GENEXP, 777, 1, 500.0, 1.5, O.TREND_CONSTANT))
    out.append(Case(1, O.KERNEL_CUBIC, 600, 20, 0.12, None, O.TREND_CONSTANT))
    out.append(Case(1, O.KERNEL_CUBIC, 1000, 7, 0.12, None, O.TREND_CONSTANT))
    out.append(Case(1, O.KERNEL_CUBIC, 530, 50, 0.05, None, O.TREND_CONSTANT))
    for nu in (1.7, 0.8):
        for N, d in big:
            out.append(Case(1, O.KERNEL_MATERN_NU, N, d, 0.2 / d, nu, O.TREND_CONSTANT))
    # The low-dimension rows of cubic and the general-nu Matern: on a line (d = 1) 777 points give a singular cubic matrix and
    # cond >= 1e10 for Matern, so these two take the smallest dimension at which the host test's conditions hold (below).
    out.append(Case(1, O.KERNEL_CUBIC, 777, LOW_D, LOW_D_THETA_CUBIC, None, O.TREND_CONSTANT))
    for nu in (1.7, 0.8):
        out.append(Case(1, O.KERNEL_MATERN_NU, 777, LOW_D, LOW_D_THETA_MATERN_NU, nu, O.TREND_CONSTANT))
    return out


# d = 2, the first dimension tried, holds the conditions for both kernels.  Cubic: the likelihood is -inf for theta in {0.3 .. 2} (as on
# the line) and finite from theta = 3 on, a support of 1 / 3 against a point spacing of ~0.36 (cond 3.6e3, gaps >= 2e-2).  Matern:
# theta = 50 gives cond 2.4e3 (nu = 1.7) and 1.5e2 (nu = 0.8) with gaps >= 1e-2; theta = 5 and 20 pass as well, with smaller gaps.
LOW_D = 2
LOW_D_THETA_CUBIC = 3.0
LOW_D_THETA_MATERN_NU = 50.0
# Matern 1/2, N = 1000, linear trend at theta = 0.3 / d: the oracle returns -inf at d = 2 and accepts d = 3 (p = 4)
SMALL_P_D = 3


def _family2():
    L, Q = O.TREND_LINEAR, O.TREND_QUADRATIC
    return [
        Case(2, O.KERNEL_MATERN52, 600, 15, 0.3 / 15, None, L),  # p = 16: the last PV = 16 basis
        Case(2, O.KERNEL_SE, 600, 16, 0.3 / 16, None, L),        # p = 17: the first PV = 32 basis
        Case(2, O.KERNEL_MATERN32, 777, 31, 0.3 / 31, None, L),  # p = 32: the last one
        Case(2, O.KERNEL_ABSEXP, 530, 5, 0.3 / 5, None, Q),      # p = 21
        Case(2, O.KERNEL_CUBIC, 600, 6, 0.12, None, Q),          # p = 28
        Case(2, O.KERNEL_SE, 600, 32, 0.3 / 32, None, L),        # p = 33: handed to the trend-rows path
        Case(2, O.KERNEL_MATERN12, 1000, SMALL_P_D, 0.3 / SMALL_P_D, None, L),  # small p, four slices
        Case(2, O.KERNEL_GENEXP, 600, 7, 0.3 / 7, 1.5, L),
        Case(2, O.KERNEL_MATERN_NU, 600, 7, 0.3 / 7, 1.7, L),
    ]


def _identities():
    """Pairs that are the same function written twice: generalized_exponential with p = 2 is the squared exponential (the matrix-core
    producer), with p = 1 the absolute exponential.  In the oracle each pair agrees to 0.0."""
    N, d = 600, 7
    th = 0.3 / d
    return [
        (Case(0, O.KERNEL_GENEXP, N, d, th, 2.0, O.TREND_CONSTANT), Case(0, O.KERNEL_SE, N, d, th, None, O.TREND_CONSTANT)),
        (Case(0, O.KERNEL_GENEXP, N, d, th, 1.0, O.TREND_CONSTANT), Case(0, O.KERNEL_ABSEXP, N, d, th, None, O.TREND_CONSTANT)),
    ]


FAMILY1 = _family1()
FAMILY2 = _family2()
CASES = FAMILY1 + FAMILY2
IDENTITIES = _identities()


def trend_size(c):
    return {O.TREND_CONSTANT: 1, O.TREND_LINEAR: c.d + 1, O.TREND_QUADRATIC: (c.d + 1) * (c.d + 2) // 2}[c.trend]


def padded_rows(N):
    return (N + 31) // 32 * 32


def slices(N):
    return (padded_rows(N) + 255) // 256


def chunk_rows_1mib(c, trend_rows=None):
    """Candidates a chunk at BOGP_CHUNK_MB=1: by the rows of the correlation chunk, which the trend-rows path (p >= 33) extends."""
    Np, p = padded_rows(c.N), trend_size(c)
    if p >= 33 if trend_rows is None else trend_rows:
        rows = (Np + 255) // 256 * 256 + (p + 31) // 32 * 32
    else:
        rows = Np
    return max(64, (1 << 20) // (8 * rows) // 64 * 64)


def chunks_1mib(c, M=M_STACK, trend_rows=None):
    mc = chunk_rows_1mib(c, trend_rows)
    return (M + mc - 1) // mc


def seed_of(c):
    # identity pairs share data: the seed ignores kernel and exponent there
    key = [c.N, c.d, c.trend] if c.family == 0 else [c.family, c.kernel, c.N, c.d, c.trend, int(round(10 * (c.extra or 0.0)))]
    return np.random.SeedSequence(key)


@lru_cache(maxsize=None)
def build(c):
    """X, y, par and the candidates of a case: `Xs` the stack the sweep runs on, `Xall` = stack + the far block for predict."""
    rng = np.random.default_rng(seed_of(c))
    N, d = c.N, c.d
    X = rng.uniform(-5, 5, size=(N, d))
    y = np.sum(X**2, axis=1)
    if c.trend != O.TREND_CONSTANT:
        y = y + X[:, 0]  # something for the linear columns to pick up
    y = (y - y.mean()) / y.std()
    y = (y + 0.05 * rng.standard_normal(N)).reshape(-1, 1)  # (noise keeps llf <= 0: the reference rejects positive values)
    par = np.r_[np.full(d, c.theta), [] if c.extra is None else [c.extra], SIGMA2_PAR]
    Xs = np.vstack([
        X[:N_ON],                                                                # ON training points
        X[N_ON : N_ON + N_NEAR] * (1.0 + 1e-9 * rng.standard_normal((N_NEAR, d))),  # a hair beside them
        rng.uniform(-5, 5, size=(N_BOX, d)),
        rng.uniform(-12, 12, size=(N_WIDE, d)),                                  # outside the data: the trend extrapolates
        rng.uniform(-5, 5, size=(1, d)),                                         # M = 1801 is no multiple of 64
    ])  # fmt: skip
    # far away: cubic's exact zeros outside its support, exp underflow for the others.  predict only: the oracle's UCB ties exactly there
    Xfar = rng.uniform(-60, 60, size=(N_FAR, d))
    for a in (X, y, par, Xs, Xfar):
        a.setflags(write=False)
    return dict(X=X, y=y, par=par, Xs=Xs, Xall=np.vstack([Xs, Xfar]), plugin=float(y.min()))


def make_state(c):
    b = build(c)
    return O.make_state(b["par"], b["X"], b["y"], c.kernel, O.MODE_NOISY, NOISE, trend=c.trend, estimate_trend=True)


def criteria(st, mu, mse, plugin, acq=ACQ):
    s2 = float(st.sigma2[0])
    return np.array([O.acquisition(a, p, mu, mse, plugin, s2, True) for a, p in acq])


def relative_gaps(vals):
    """(winner - runner-up) / |winner| per criterion: what a device at rtol 1e-6 on the values must stay far below."""
    out = []
    for v in vals:
        top = np.sort(v)[-2:]
        out.append(float((top[1] - top[0]) / abs(top[1])) if top[1] != 0.0 else 0.0)
    return np.array(out)


@lru_cache(maxsize=None)
def oracle(c):
    """The oracle on a case: state, posterior of stack + far block, criteria and winners on the stack.  Arrays are read-only."""
    b = build(c)
    st = make_state(c)
    mu, mse = O.predict_chunked(st, b["Xall"], 512)
    mu, mse = mu[:, 0], mse[:, 0]
    vals = criteria(st, mu[:M_STACK], mse[:M_STACK], b["plugin"])
    idx = np.argmax(vals, axis=1)
    for a in (mu, mse, vals, idx):
        a.setflags(write=False)
    return dict(st=st, sigma2=float(st.sigma2[0]), llf=st.llf, mu=mu, mse=mse, vals=vals, idx=idx, gaps=relative_gaps(vals))


def correlation_cond(st):
    """2-norm condition number of the matrix the fit factorises (nugget included): from its Cholesky factor."""
    sv = np.linalg.svd(st.C, compute_uv=False)
    return float((sv[0] / sv[-1]) ** 2)


# ---- the cubic rows of test_fused_small_sweep_equals_the_chunked_schedule_and_the_oracle (tests/test_gpu_driver.py) ----------------
DRIVER_ACQ = ((O.ACQ_EI, 0.0), (O.ACQ_MGFI, 2.0), (O.ACQ_UCB, 0.5), (O.ACQ_EPSILON_PI, 1e-10))
DRIVER_MS = (33, 63, 64, 65, 1000, 4097, 16384 + 700, 16384 + 5000)  # the last two: bulk launch + 32- / 48-candidate tail launch
# (N, d): Np <= 256 and d <= 32 is the four-wave schedule of k_sweep_small, 256 < N <= 512 the eight-wave one
DRIVER_CUBIC = ((120, 12), (260, 18))


def driver_model(N, d, mode):
    """Training data and parameters of that test, with the generator in the state in which the test goes on to draw candidates."""
    rng = np.random.default_rng(N + d)
    X = rng.uniform(-5, 5, size=(N, d))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std() + 0.05 * rng.standard_normal(N)).reshape(-1, 1)
    theta = np.full(d, 0.4 / d) * rng.uniform(0.7, 1.3, size=d)
    par = np.r_[theta, 0.9 if mode == O.MODE_NOISY else 0.98]
    nv = 1e-6 if mode == O.MODE_NOISY else 0.0
    return rng, X, y, par, nv


def driver_candidates(rng, X, M):
    Xs = rng.uniform(-5, 5, size=(M, X.shape[1]))
    Xs[M // 2] = X[3]  # a candidate on a training point: MSE at nugget level, guards in play
    return Xs
