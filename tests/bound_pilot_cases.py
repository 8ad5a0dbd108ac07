"""Inputs and host-side expectations shared by tests/test_gpu_bound_pilot.py and tests/test_bound_pilot_host.py (not a test module): the
best-bound pilot of the one-pass pruned sweep on the model and candidates of tests/prune_cases.py -- N = 544,
d = 3, M = 3001; blocks of 256 and 512 rows give 12 and 6 blocks, the last one ragged (185 and 441 rows).

What the host can say with the oracle: given the rows of a pilot, the thresholds are the best exact values over them; a row behind the
pilot survives unless the exact bound puts every criterion below its threshold (the FP32 stage only ever flags a superset); and the
counts of host and device agree wherever no bound lies within GAP relative of its threshold -- the prune test's own margin is 1e-9."""
import numpy as np

import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

EI, PI, UCB, MGFI = _lib.ACQ_EI, _lib.ACQ_EPSILON_PI, _lib.ACQ_UCB, _lib.ACQ_MGFI
UCB2 = [(UCB, 8.0), (UCB, 0.5)]  # tests/test_gpu_prune_onepass.py's
MIX8 = [(EI, 0.0), (PI, 0.05), (UCB, 0.5), (MGFI, 1.0), (MGFI, 2.0), (EI, 0.0), (PI, 0.0), (UCB, 2.0)]
BLOCKS = (256, 512)
GAP = 1e-6
# (name, criteria, minimize): the criteria of the byte-identity cases.  COUNTED: those whose survivors are also counted against the host
# -- not MIX8: its probability of improvement saturates, so bounds EQUAL to the threshold abound (distance 0; bytes and indices only).
CRITERIA = [("EI", [(EI, 0.0)], True), ("MGFI", [(MGFI, 2.0)], True), ("UCB2", UCB2, True), ("MIX8", MIX8, True),
            ("EI+MGFI maximised", [(EI, 0.0), (MGFI, 2.0)], False)]  # fmt: skip
COUNTED = [c for c in CRITERIA if c[0] != "MIX8"]
PLACES = (5, 1500, 2990)  # the first block, the middle, the ragged end


def plugin_of(y, minimize=True):
    return float(y.min()) if minimize else -1.0 * float(y.max())


def rows_view(st, Xs, acq, plugin, minimize=True):
    """(exact values [q][M], exact bounds [q][M], rows with a NaN coordinate) with the oracle; a NaN row is evaluated as row 0 and masked"""
    nan = np.isnan(Xs).any(axis=1)
    if nan.any():
        Xs = Xs.copy()
        Xs[nan] = Xs[0]
    mu, mse, sd_ub = PC.oracle_rows(st, Xs)
    s2 = float(st.sigma2[0])
    y_hat = mu if minimize else -1 * mu
    vals = np.array([O.acquisition(a_id, a_par, mu, mse, plugin, s2, minimize) for a_id, a_par in acq])
    bounds = np.array([PC.upper_bounds(a_id, a_par, y_hat, sd_ub, plugin, s2) for a_id, a_par in acq])
    return vals, bounds, nan


def exact_pilot(bounds, nan, block_rows):
    """The pilot the EXACT bounds would choose: per block and criterion the first row with the largest bound, a NaN row first.  The
    device chooses by FP32 interval bounds, so its pilot may differ where two bounds of a block lie within their margins."""
    M = bounds.shape[1]
    rows = set()
    for b0 in range(0, M, block_rows):
        for b in bounds:
            blk = np.where(nan[b0 : b0 + block_rows], np.inf, b[b0 : b0 + block_rows])
            rows.add(b0 + int(np.argmax(blk)))
    return np.array(sorted(rows), dtype=np.int64)


def survivors_behind(vals, bounds, nan, pilot):
    """(rows that survive the exact bound against the thresholds `pilot` sets, the pilot's rows left out; the smallest relative distance
    of a bound from its threshold over those rows) -- (M, 0.0) less the pilot where a threshold is not finite: nothing is pruned."""
    M = vals.shape[1]
    behind = np.ones(M, dtype=bool)
    behind[pilot] = False
    keep = nan.copy()
    gap = np.inf
    for v, b in zip(vals, bounds):
        pv = np.where(nan[pilot], np.nan, v[pilot])
        thr = pv[int(np.argmax(pv))]  # (np.argmax: a NaN first)
        if not np.isfinite(thr):
            return int(np.count_nonzero(behind)), 0.0
        keep |= ~(b + PC.prune_margin(b, thr) < thr)
        ok = behind & ~nan
        gap = min(gap, float(np.min(np.abs(b[ok] - thr) / np.maximum(np.abs(b[ok]), abs(thr)))))
    return int(np.count_nonzero(keep & behind)), gap
