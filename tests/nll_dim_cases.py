"""Inputs shared by tests/test_gpu_nll_dims.py and tests/test_nll_dim_cases_host.py (not a test module): likelihood problems whose
input dimension sits on every side of the blocks the likelihood kernels walk the dimensions in --
  * 16 dimensions a staged block (KC) in grad_contract_tile, build_R_tile, k_resid_gamma and k_min_pdist2 (csrc/kernels_pairs.hip):
    second and later trips of the kc loops, the partial last block, out[kc + tid];
  * the pitch d | 1 of X in k_nll_small's LDS, its four-dimension gradient reduction inside 64-dimension blocks, its cap d <= 64
    (NllSmallArgs::theta[64], NS_BPAR) and the row limit of its LDS test, which moves with d (csrc/kernels_nllsmall.hip).
Every dimension of a problem has its own weight, phase and length scale, so no two components of the likelihood gradient coincide
and none vanishes: the host test asserts that in the oracle for every case, with the bound the device test uses.  A case that
misses a condition is replaced HERE, through its `seed` field (0: the generator's own seed); none is skipped.

Rows, the smallest at which each path and tile side exists: 100 (one launch up to d = 64, the general path at d = 65: ld = 128),
200 (elimination, 16 x 16 gradient tiles), 300 (32 x 32 tiles), 1025 (64 x 64 tiles; d = 17 and 33, one kernel).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import gp_oracle as O

D_EDGES = (15, 16, 17, 31, 32, 33, 48, 63, 64, 65)
ROWS = (100, 200, 300)
N_TILE64, D_TILE64 = 1025, (17, 33)
# k_nll_small's LDS test: the largest N of one launch is 156 only for d <= 21; these are the pairs at which it gives way
LDS_EDGES = ((156, 21), (156, 22), (144, 35), (144, 36), (128, 57), (128, 58), (100, 64), (100, 65))
GRAD_KERNELS = (O.KERNEL_SE, O.KERNEL_MATERN12, O.KERNEL_MATERN32, O.KERNEL_MATERN52, O.KERNEL_ABSEXP)
MODES = (O.MODE_NOISELESS, O.MODE_NOISE_ESTIM, O.MODE_NOISY)
NOISE_VAR = 1e-4  # noisy mode
FIXED_BETA = 0.17
GENEXP_P = 1.7
BATCH_P = 5
BATCH_SHAPES = ((100, 64), (100, 65), (200, 17), (200, 33), (300, 64))
REML_SHAPES = ((200, 17), (200, 33))
VALUE_ONLY_SHAPES = ((100, 33), (200, 33))
PERMUTED_SHAPES = ((200, 33), (100, 64))
PDIST_SHAPES = tuple((M, d) for d in (16, 17, 33) for M in (63, 129))

EPS = 2.3e-16
# The gradient bound, relative to the oracle's largest component: TOL_G + 200 eps cond(R) per COMPONENT.  TOL_G is ten times the
# worst |g_k - go_k| / max|go| measured over all cases of this module on an MI355X, 6.41e-15 (see test_gpu_nll_dims.py's docstring); the cap is
# the bound up to which the conditions on the inputs were verified when the cases were written, and it is not to be widened.
TOL_G = 7e-14
TOL_G_CAP = 3e-7

# slot: 0 = the problem's own parameters, s >= 1 = the s-th vector of a batch; reml: the restricted likelihood's layout
Case = namedtuple("Case", "N d kernel mode est iso slot reml seed")
_NAMES = {O.KERNEL_SE: "se", O.KERNEL_MATERN12: "m12", O.KERNEL_MATERN32: "m32", O.KERNEL_MATERN52: "m52", O.KERNEL_ABSEXP: "absexp",
          O.KERNEL_CUBIC: "cubic", O.KERNEL_GENEXP: "genexp"}  # fmt: skip
_MODES = {O.MODE_NOISELESS: "noiseless", O.MODE_NOISE_ESTIM: "estim", O.MODE_NOISY: "noisy"}


# Cases whose generator seed 1000 N + d left a gradient component below 100 x, or two components closer than 10 x, the cap of the
# bound (relative to the largest component), with the seed that replaced it: the smallest 1000 N + d + 1e6 j that clears both
# conditions with a factor ten to spare.  (N, d, kernel, mode, est, iso) -> seed
RESEEDED = {
    (300, 48, O.KERNEL_MATERN52, O.MODE_NOISY, True, False): 1300048,      # two components 1.1e-6 apart
    (300, 63, O.KERNEL_MATERN12, O.MODE_NOISY, True, False): 1300063,      # two components 1.9e-6 apart
    (300, 63, O.KERNEL_MATERN32, O.MODE_NOISY, True, False): 1300063,      # a component of 2.5e-7
    (200, 31, O.KERNEL_MATERN52, O.MODE_NOISE_ESTIM, True, False): 2200031,  # two components 9.1e-7 apart
    (200, 65, O.KERNEL_ABSEXP, O.MODE_NOISE_ESTIM, True, False): 1200065,  # a component of 2.0e-5
}


def case(N, d, kernel, mode=O.MODE_NOISY, est=True, iso=False, slot=0, reml=False):
    seed = RESEEDED.get((N, d, kernel, mode, est, iso), 0) if not (slot or reml) else 0
    return Case(N, d, kernel, mode, est, iso, slot, reml, seed)


def case_id(c):
    return "N%d-d%d-%s-%s%s%s%s%s" % (c.N, c.d, _NAMES[c.kernel], _MODES[c.mode], "" if c.est else "-fixed", "-iso" if c.iso else "",
                                      "-slot%d" % c.slot if c.slot else "", "-reml" if c.reml else "")  # fmt: skip


@lru_cache(maxsize=None)
def problem(N, d, seed=0):
    """X, y (standardised), theta: every dimension with its own weight 1 + 0.5 cos(1.7 k), phase 0.3 k and length scale."""
    rng = np.random.default_rng(seed if seed else 1000 * N + d)
    X = rng.uniform(-3, 3, (N, d))
    k = np.arange(d)
    w = 1 + 0.5 * np.cos(1.7 * k)
    y = (w * np.sin(X + 0.3 * k)).sum(axis=1) + 0.3 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    theta = (0.9 / d) * rng.uniform(0.5, 2.0, d)
    for a in (X, y, theta):
        a.setflags(write=False)
    return X, y.reshape(-1, 1), theta


def parameters(c):
    """(par, noise_var) of a case in the layout its likelihood takes (gpr.py:1073-1086; restricted: :826-834)."""
    theta = problem(c.N, c.d, c.seed)[2]
    th = theta[:1] if c.iso else theta
    last = {O.MODE_NOISY: 0.85, O.MODE_NOISE_ESTIM: 0.93}.get(c.mode)
    if c.slot:  # the vectors of a batch: every entry moved by its own factor, like the restarts of an MLE
        f = np.random.default_rng(7919 * c.slot + c.d).uniform(0.6, 1.6, len(th) + 1)
        th = th * f[:-1]
        last = None if last is None else min(0.99, last * f[-1]) if c.mode == O.MODE_NOISE_ESTIM else last * f[-1]
    if c.mode == O.MODE_NOISELESS and not c.reml:
        th = th * 6  # no nugget at all: short length scales keep cond(R) moderate
    if c.kernel == O.KERNEL_GENEXP:
        th = np.r_[th, GENEXP_P]
    if c.reml:  # [theta, sigma2] with the fixed noise variance, or [theta, sigma2, noise variance]
        return (np.r_[th, 0.85], NOISE_VAR) if c.mode == O.MODE_NOISY else (np.r_[th, 0.93, 0.07], 0.0)
    if c.mode == O.MODE_NOISELESS:
        return np.array(th), 0.0
    return np.r_[th, last], (NOISE_VAR if c.mode == O.MODE_NOISY else 0.0)


def beta_of(c):
    return 0.0 if c.est else FIXED_BETA


def has_gradient(c):
    return c.kernel in GRAD_KERNELS


def factorised_matrix(c):
    """The matrix both sides factorise (two correct factorisations differ by ~ eps cond of it)."""
    X = problem(c.N, c.d, c.seed)[0]
    par, nv = parameters(c)
    n_tail = 0 if (c.mode == O.MODE_NOISELESS and not c.reml) else 2 if (c.reml and c.mode == O.MODE_NOISE_ESTIM) else 1
    R0 = O.correlation_matrix(c.kernel, par[: len(par) - n_tail], X)
    eye = np.eye(c.N)
    if c.reml:
        s2, tau2 = (par[-1], nv) if c.mode == O.MODE_NOISY else (par[-2], par[-1])
        return (s2 * R0 + tau2 * eye) / (s2 + tau2)
    if c.mode == O.MODE_NOISE_ESTIM:
        return par[-1] * R0 + (1 - par[-1]) * eye
    if c.mode == O.MODE_NOISY:
        return (par[-1] * R0 + nv * eye) / (par[-1] + nv)
    return R0


@lru_cache(maxsize=None)
def oracle(c):
    """(llf, gradient or None, cond(R)) of a case by oracle/gp_oracle.py, computed once a process and left unchanged."""
    X, y, _ = problem(c.N, c.d, c.seed)
    par, nv = parameters(c)
    fn = O.log_likelihood_restricted if c.reml else O.log_likelihood_concentrated
    out = fn(par, X, y, c.kernel, c.mode, noise_var=nv, estimate_trend=c.est, beta=beta_of(c), eval_grad=has_gradient(c))
    llf, g = (out[0], np.asarray(out[1], dtype=np.float64).ravel()) if has_gradient(c) else (out, None)
    if g is not None:
        g.setflags(write=False)
    return float(llf), g, float(np.linalg.cond(factorised_matrix(c)))


def llf_bound(c):
    llf, _, cond = oracle(c)
    return (1e-10 + 8 * EPS * cond) * max(1.0, abs(llf))


def grad_bound(c):
    """Absolute bound on EVERY component of the gradient."""
    _, g, cond = oracle(c)
    return (TOL_G + 200 * EPS * cond) * np.max(np.abs(g))


def grad_rel_bound(c):
    return TOL_G + 200 * EPS * oracle(c)[2]


def one_launch_fits(N, d):
    """nll_small_fits of csrc/kernels_nllsmall.hip, restated: blocks of 4 rows, at most 39 of them and 1024 threads (the panel waves +
    one owner a block of the lower triangle), 64 theta in the kernel's arguments, X at pitch d | 1 and 16 doubles a block beside
    36 KB of static LDS in the 160 KB of a CU."""
    if N > 156 or d > 64:
        return False
    nb = (N + 3) // 4
    up64 = lambda v: (v + 63) // 64 * 64  # noqa: E731
    threads = up64(4 * (nb + 1)) + up64((nb + 1) * (nb + 2) // 2 - 1)
    lds = (((N * (d | 1) + 1) & ~1) + 16 * (nb * (nb + 1) // 2)) * 8
    return threads <= 1024 and lds + 36 * 1024 <= 160 * 1024


PATH_GENERAL, PATH_ONE_LAUNCH, PATH_ELIM = 0, 1, 2  # BOGP_NLL_PATH_* of include/bogp.h (held to the header by the host test)


def expected_path(N, d):
    """Constant trend, one target, no environment switch: one launch where it fits, the elimination from ld = 192 up to N = 3072."""
    if one_launch_fits(N, d):
        return PATH_ONE_LAUNCH
    ld = (N + 63) // 64 * 64
    return PATH_ELIM if (N <= 3072 and ld >= 192) else PATH_GENERAL


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


def _default_cases():
    out = []
    for N in ROWS:  # all five gradient kernels on every row count and every dimension edge
        for d in D_EDGES:
            out += [case(N, d, k) for k in GRAD_KERNELS]
    for N, d in LDS_EDGES:  # both sides of the one-launch limit where the LDS test moves it
        out += [case(N, d, k) for k in GRAD_KERNELS]
    # N = 200: the three modes, estimated and fixed beta, ARD and isotropic theta; the kernel rotates with the dimension
    for i, d in enumerate(D_EDGES):
        for mode in MODES:
            for est in (True, False):
                for iso in (False, True):
                    out.append(case(200, d, GRAD_KERNELS[i % 5], mode, est, iso))
    out += [case(N_TILE64, d, O.KERNEL_MATERN52) for d in D_TILE64]
    return _unique(out)


DEFAULT_CASES = _default_cases()                                               # the path the library chooses by itself
GENERAL_CASES = [c for c in DEFAULT_CASES if c.N in (200, N_TILE64)]           # again with BOGP_NLL_FUSED=0
BATCH_KERNELS = (O.KERNEL_MATERN52, O.KERNEL_SE, O.KERNEL_ABSEXP, O.KERNEL_MATERN32, O.KERNEL_MATERN12)
BATCH_CASES = [[case(N, d, k, slot=s) for s in range(1, BATCH_P + 1)] for (N, d), k in zip(BATCH_SHAPES, BATCH_KERNELS)]
REML_CASES = [case(N, d, O.KERNEL_MATERN32 if d == 17 else O.KERNEL_SE, mode, reml=True)
              for N, d in REML_SHAPES for mode in (O.MODE_NOISY, O.MODE_NOISE_ESTIM)]  # fmt: skip
VALUE_ONLY_CASES = [case(N, d, k) for N, d in VALUE_ONLY_SHAPES for k in (O.KERNEL_CUBIC, O.KERNEL_GENEXP)]
PERMUTED_CASES = [case(200, 33, O.KERNEL_MATERN52), case(100, 64, O.KERNEL_MATERN32)]
GRADIENT_CASES = _unique(DEFAULT_CASES + [c for b in BATCH_CASES for c in b] + REML_CASES + PERMUTED_CASES)
ALL_CASES = GRADIENT_CASES + VALUE_ONLY_CASES
