"""TEST-ONLY float64 restatement of the reference's EHVI.forward (bayes_optim/multi_objective/analytic.py:176-274):
the psi / nu factors of [Yang2019] per (cell, objective), the 2^m cross product of {psi(l,l) - psi(l,u), nu(l,u)},
summed over subsets and cells -- in NumPy, written independently of bogp.pareto and of the device's product form."""
import itertools

import numpy as np
from scipy.special import ndtr

_SQRT2PI = np.sqrt(2.0 * np.pi)


def _psi(lower, upper, mu, sigma):
    u = (upper - mu) / sigma
    return sigma * np.exp(-0.5 * u * u) / _SQRT2PI + (mu - lower) * (1.0 - ndtr(u))


def _nu(lower, upper, mu, sigma):
    return (upper - lower) * (1.0 - ndtr((upper - mu) / sigma))


def ehvi(mu, mse, lower, upper, block=512):
    """mu, mse: (M, m) posterior moments of maximised targets; lower, upper: (C, m) cells.  Returns (M,) float64."""
    mu = np.atleast_2d(np.asarray(mu, float))
    sigma = np.sqrt(np.maximum(np.atleast_2d(np.asarray(mse, float)), 1e-9))  # analytic.py:233
    lower = np.asarray(lower, float)
    upper = np.minimum(np.asarray(upper, float), 1e10)  # analytic.py:236-238 (float64 input)
    m = mu.shape[1]
    subsets = np.array(list(itertools.product([0, 1], repeat=m)), dtype=np.int64)  # 2^m x m
    out = np.empty(len(mu))
    for a in range(0, len(mu), block):
        mb, sb = mu[a : a + block, None, :], sigma[a : a + block, None, :]
        psi_diff = _psi(lower, lower, mb, sb) - _psi(lower, upper, mb, sb)  # B x C x m
        nu = _nu(lower, upper, mb, sb)
        stacked = np.stack([psi_diff, nu], axis=-2)  # B x C x 2 x m
        tot = np.zeros(stacked.shape[0])
        for s in subsets:
            tot += np.prod(stacked[:, :, s, np.arange(m)], axis=-1).sum(axis=-1)
        out[a : a + block] = tot
    return out
