"""The address form of the FP32 bounding loop (csrc/kernels_bound32.hip).

k_bound32_sums reads its operands through a scalar base per operand row plus one 32-bit lane offset per operand kind.  A wrong base or
offset reads another training block or another fragment row, so the sums are held to the oracle at every k-step count's edge: d = 1, 4
(KS = 1, with and without padding), 5 (KS = 2, padded), 20 (KS = 5), 32 (KS = 8), and d = 33 for the general kernel; the three
kernels; simple and ordinary kriging (the kernel without and with the w . r sum).  N = 544 = 34 sixteen-point blocks: the four waves
take 9, 9, 8, 8 of them, and the last block of a wave is where a base that steps wrongly shows.  M = 3001 with BOGP_CHUNK_MB=1: a
pilot of 192 rows and 2809 rows behind it, the last tile ragged.
The bound on the error: the parent's smallest margin / error ratio over its cases is 525, so the largest error must
stay below a tenth of the smallest margin, a factor 50 inside what the arithmetic itself needs.  Where the correlations are of order one
(every kernel up to d = 5, the Matern kernels beyond) a wrong row or fragment moves a sum by a large part of |gamma|_1, orders of
magnitude more than a margin.  The squared exponential at d = 20, 32, 33 is weaker: with theta = 0.05 its r is 1e-7 and less on nearly
every row, and those cases would pass with almost any address; the address code is shared per KS with the Matern cases at the same d,
which do carry the check.

The criterion is tests/bound32_trim_cases.py's (UCB 0.5 up to d = 5, UCB 0.01 from d = 20 on, where 0.5 keeps most of the pilot).
At d = 1 the shared model (theta = 0.05, process variance 0.01, nugget 1e-6) is refused by the oracle itself: 544 points on a line leave
a positive log-likelihood, which the reference treats as a failed fit.  The bowl is kept and pinned at process variance 1 with nugget 1
there, which the oracle accepts for the three kernels; UCB 0.5 leaves 16 to 18 of the pilot's 192 rows with it (24 would still pass)."""
import numpy as np
import pytest

import bound32_cases as BC
import bound32_trim_cases as TC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

UCB = _lib.ACQ_UCB
ONEPASS, FALLBACK = _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK
PILOT = PC.CHUNK_ROWS
BEHIND = PC.M_CAND - PILOT


@pytest.fixture()
def small_chunks(monkeypatch):
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")


def line_model(kernel, ordinary):
    """BC.model's bowl at d = 1, pinned where the oracle accepts it (module docstring) -> (X, y, par, st, nugget)"""
    rng = np.random.default_rng(0)
    X = rng.uniform(-5, 5, size=(PC.N_TRAIN, 1))
    y = np.sum(X**2, axis=1)
    y = ((y - y.mean()) / y.std()).reshape(-1, 1)
    par = np.r_[0.05, 1.0]
    st = O.make_state(par, X, y, kernel, O.MODE_NOISY, 1.0, estimate_trend=ordinary, beta=None if ordinary else 0.0)
    return X, y, par, st, 1.0


def state(eng, acq, plugin):
    """everything a caller can see of one sweep, as bytes and tuples"""
    v, i = eng.sweep(acq, plugin, True)
    return dict(v=v.tobytes(), i=i.tobytes(), path=eng.last_prune_path(), contracted=eng.last_contracted_rows(), b32=eng.last_bound32(),
                dbg=tuple(a.tobytes() for a in eng.debug_bound32()))  # fmt: skip


@pytest.mark.parametrize("d", [1, 4, 5, 20, 32, 33])
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("kernel", TC.KERNELS)
def test_sums_lie_within_their_margins_at_every_k_step_count(small_chunks, kernel, ordinary, d):
    if d == 1:
        X, y, par, st, nugget = line_model(kernel, ordinary)
        acq = [(UCB, 0.5)]
    else:
        X, y, par, st = BC.model(kernel, ordinary, d)
        nugget, acq = PC.NOISE, TC.criterion(kernel, ordinary, d)
    pl = float(y.min())
    Xs = TC.candidates(d)
    eng = _lib.Engine(0)
    try:
        eng.set_train(X, y)
        eng.commit(kernel, _lib.MODE_NOISY, par, nugget, ordinary, 0.0)
        eng.upload_candidates(Xs)
        eng.set_prune(True)
        eng.set_prune_bound32(True)
        s1 = state(eng, acq, pl)
        mu32, e_mu, wd32, e_w, flags = eng.debug_bound32()
        # the route: the pilot estimate lets one pass through, the stage ran over every row behind the pilot
        keep = TC.exact_flags(st, Xs, acq, pl)
        assert 8 * int(keep[:PILOT].sum()) <= PILOT
        assert s1["path"][0] in (ONEPASS, FALLBACK) and s1["b32"][0] == BEHIND and len(mu32) == BEHIND and int(flags.sum()) == s1["b32"][1]
        # within the exported margins of the oracle's sums on every row, and far inside them
        g, w = BC.vectors(st)
        with np.errstate(all="ignore"):
            r = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs[PILOT:], st.X)).reshape(BEHIND, -1)
        err_mu, err_w = np.abs(mu32 - r.dot(g)), np.abs(wd32 - r.dot(w))
        print("kernel %d ordinary %d d %2d %s: path %s, |S1| = %d; mu: max error %.3g, smallest margin %.3g (ratio %.3g); w: %.3g, %.3g"
              % (kernel, ordinary, d, acq, s1["path"], s1["b32"][1], err_mu.max(), e_mu.min(), e_mu.min() / max(err_mu.max(), 1e-300),
                 err_w.max(), e_w.min()))  # fmt: skip
        assert np.all(err_mu <= e_mu) and np.all(err_w <= e_w)
        assert err_mu.max() < 0.1 * e_mu.min()
        if ordinary:
            assert err_w.max() < 0.1 * e_w.min()
        else:
            assert np.all(wd32 == 0.0)
        # every row the exact bound keeps is flagged
        assert not np.any(keep[PILOT:] & (flags == 0))
        # a second run: the same bytes everywhere
        assert state(eng, acq, pl) == s1
    finally:
        eng.close()
