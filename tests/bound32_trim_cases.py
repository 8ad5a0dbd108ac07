"""Shared by tests/test_bound32_trim_host.py and tests/test_gpu_bound32_trim.py (not a test module): a float32 NumPy restatement of
k_bound32_sums as it runs up to d = 32 (csrc/kernels_bound32.hip) -- both operands scaled by kappa in FP64
before their one rounding, the fma chain started at fl(kappa^2 na) + fl(kappa^2 nb) so that it ends in kappa^2 s, |.| where a clamp
stood, the profiles without a constant in front of the square root or the exponential, the same FP32 accumulation in runs of 16 terms
with an FP64 tail, w . r left at 0 under simple kriging -- and the criterion each (kernel, kriging, d) of the device test is swept with."""
import numpy as np

import bound32_cases as BC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

F32 = np.float32
LOG2E = 1.4426950408889634
KAPPA = {O.KERNEL_SE: 1.2011224087864498, O.KERNEL_MATERN32: 2.4988211106473432, O.KERNEL_MATERN52: 3.225964182229561}
KERNELS = [O.KERNEL_SE, O.KERNEL_MATERN32, O.KERNEL_MATERN52]
DIMS_REG = [3, 5, 20, 32]  # KS = 1, a padded k-step, KS = 5, KS = 8: the register-fragment kernel
DIM_ANY = 33               # the general kernel
UCB = _lib.ACQ_UCB


def profile32(kernel, sh):
    """the profile on sh = kappa^2 s"""
    if kernel == O.KERNEL_SE:
        return np.exp2(-np.abs(sh)).astype(F32)
    K = np.sqrt(np.abs(sh)).astype(F32)
    e = np.exp2(-K).astype(F32)
    one = np.ones_like(K)
    if kernel == O.KERNEL_MATERN32:
        return (BC._fma32(K, np.full_like(K, F32(0.693147181)), one) * e).astype(F32)
    p = BC._fma32(K, BC._fma32(K, np.full_like(K, F32(0.160151005)), np.full_like(K, F32(0.693147181))), one)
    return (p * e).astype(F32)


def restate(st, Xs):
    """BC.restate's dictionary for the operation sequence of the register-fragment kernel"""
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    M, d = Xs.shape
    assert d <= 32
    N = st.X.shape[0]
    kappa = KAPPA[st.kernel]
    rt = np.sqrt(st.theta) * np.ones(d)
    a, b = Xs * rt, st.X * rt
    na, nb = np.zeros(M), np.zeros(N)
    for k in range(d):  # dimension order, as the device sums them
        na, nb = a[:, k] * a[:, k] + na, b[:, k] * b[:, k] + nb
    g, w = BC.vectors(st)
    with np.errstate(all="ignore"):
        r64 = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs, st.X)).reshape(M, N)
    mu64, wd64 = r64.dot(g), r64.dot(w)
    Npad = (N + 63) // 64 * 64
    a32, b32 = (a * kappa).astype(F32), np.zeros((Npad, d), dtype=F32)
    b32[:N] = ((-2.0 * kappa) * b).astype(F32)
    na32, nb32, g32, w32 = (na * (kappa * kappa)).astype(F32), np.zeros(Npad, F32), np.zeros(Npad, F32), np.zeros(Npad, F32)
    nb32[:N], g32[:N], w32[:N] = ((kappa * kappa) * nb).astype(F32), g.astype(F32), w.astype(F32)
    with np.errstate(all="ignore"):
        sh = (na32[:, None] + nb32[None, :]).astype(F32)
        for k in range(d):  # (the padded k-step adds exact zeros)
            sh = BC._fma32(a32[:, k : k + 1], b32[None, :, k], sh)
        r = profile32(st.kernel, sh)
        r5 = r.reshape(M, Npad // 64, 4, 4, 4)
        out = []
        for v32 in (g32, w32) if st.estimate_trend else (g32,):
            v5 = v32.reshape(Npad // 64, 4, 4, 4)
            tot = np.zeros((M, 4, 4))
            acc = np.zeros((M, 4, 4), dtype=F32)
            for it in range(Npad // 64):
                for cc in range(4):
                    acc = BC._fma32(r5[:, it, :, :, cc], np.broadcast_to(v5[it, :, :, cc], (M, 4, 4)), acc)
                if it % 4 == 3 or it == Npad // 64 - 1:
                    tot += acc.astype(np.float64)
                    acc = np.zeros((M, 4, 4), dtype=F32)
            out.append(tot.sum(axis=2).sum(axis=1))
    if not st.estimate_trend:
        out.append(np.zeros(M))  # WD = false: the sum is not formed
    return dict(mu32=out[0], wd32=out[1], mu64=mu64, wd64=wd64, na=na, gamma_l1=float(np.abs(g).sum()), w_l1=float(np.abs(w).sum()),
                nb_max=float(nb.max()))  # fmt: skip


def candidates(d, seed=7, M=PC.M_CAND):
    """PC.candidates() in d dimensions (d = 3: the same rows)"""
    return np.random.default_rng(seed).uniform(-5, 5, size=(M, d))


def criterion(kernel, ordinary, d):
    """The criterion the device test sweeps (kernel, kriging, d) with: UCB 0.5 as in tests/test_gpu_bound32.py where the pilot estimate
    lets one pass through with it (d = 3, 5), UCB 0.01 -- all but the mean alone; the library wants a multiplier above 0 -- from d = 20
    on, where theta = 0.05 leaves the deviation at the prior's almost everywhere and a larger multiple of it keeps most of the pilot.
    tests/test_bound32_trim_host.py proves each entry with the oracle and bogp_prune_decide."""
    return [(UCB, 0.5 if d <= 5 else 0.01)]


def exact_flags(st, Xs, acq, plugin, minimize=True, pilot=PC.CHUNK_ROWS):
    """PC.surviving_fraction's flags over ALL rows, the pilot's included (what the pilot estimate counts)"""
    mu, mse, sd_ub = PC.oracle_rows(st, Xs)
    s2 = float(st.sigma2[0])
    y_hat = mu if minimize else -1 * mu
    keep = np.zeros(len(Xs), dtype=bool)
    for a_id, a_par in acq:
        vals = O.acquisition(a_id, a_par, mu, mse, plugin, s2, minimize)
        thr = vals[:pilot][int(np.argmax(vals[:pilot]))]
        b = PC.upper_bounds(a_id, a_par, y_hat, sd_ub, plugin, s2)
        keep |= ~(np.isfinite(thr) & (b + PC.prune_margin(b, thr) < thr))
    return keep
