"""k_bound32_sums on the device at every compile-time shape the trimmed kernel takes (csrc/kernels_bound32.hip, DESIGN.md section
5.22.2): the three kernels, simple and ordinary kriging, d = 3 (one k-step), 5 (a padded k-step), 20 (five), 32 (eight, the last the
register-fragment kernel serves) and 33 (the general kernel).  Per combination, with the criterion tests/bound32_trim_cases.py names
and tests/test_bound32_trim_host.py proves to pass the pilot estimate: the stage runs over every row behind the pilot, its read-back
lies within its margins of the oracle, every exact survivor is flagged, the sweep returns the same bytes with the stage off and on,
and two runs give the same bytes.  N = 544, M = 3001, BOGP_CHUNK_MB=1 -> 192 rows a chunk = the pilot, 2809 rows behind it."""
import numpy as np
import pytest

import bound32_cases as BC
import bound32_trim_cases as TC
import prune_cases as PC
from bogp import _lib
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

ONEPASS, FALLBACK = _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK
PILOT = PC.CHUNK_ROWS
BEHIND = PC.M_CAND - PILOT


@pytest.fixture()
def small_chunks(monkeypatch):
    monkeypatch.setenv("BOGP_CHUNK_MB", "1")


def sweep_state(eng, acq, plugin):
    v, i = eng.sweep(acq, plugin, True)
    return v, i, eng.last_prune_path(), eng.last_contracted_rows(), eng.last_bound32()


@pytest.mark.parametrize("d", TC.DIMS_REG + [TC.DIM_ANY])
@pytest.mark.parametrize("ordinary", [False, True])
@pytest.mark.parametrize("kernel", TC.KERNELS)
def test_stage_runs_within_its_margins_and_changes_nothing(small_chunks, kernel, ordinary, d):
    X, y, par, st = BC.model(kernel, ordinary, d)
    acq, pl = TC.criterion(kernel, ordinary, d), float(y.min())
    Xs = TC.candidates(d)
    Xs[700] = X[17]  # behind the pilot: a training point itself, a point 1e-4 from one, a box corner, a row at 1e3
    Xs[701] = X[40] + 1e-4 / np.sqrt(d)
    Xs[702] = np.where(np.arange(d) % 2 == 0, 5.0, -5.0)
    Xs[703] = 1e3
    eng = _lib.Engine(0)
    try:
        eng.set_train(X, y)
        eng.commit(kernel, _lib.MODE_NOISY, par, PC.NOISE, ordinary, 0.0)
        eng.upload_candidates(Xs)
        eng.set_prune(True)
        eng.set_prune_bound32(False)
        v0, i0, p0, n0, rep0 = sweep_state(eng, acq, pl)
        assert rep0 == (0, 0, 0)
        eng.set_prune_bound32(True)
        v1, i1, p1, n1, rep = sweep_state(eng, acq, pl)
        dbg = eng.debug_bound32()
        mu32, e_mu, wd32, e_w, flags = dbg
        # the stage ran, over every row behind the pilot
        assert p1[0] in (ONEPASS, FALLBACK) and rep[0] == BEHIND and len(mu32) == BEHIND and int(flags.sum()) == rep[1] >= p1[1]
        # off and on: identical bytes, indices, path, survivors, rounds and contracted rows
        assert v1.tobytes() == v0.tobytes() and np.array_equal(i1, i0), (v0, v1, i0, i1)
        assert p1 == p0 and n1 == n0
        # within the margins of the oracle on every row
        g, w = BC.vectors(st)
        with np.errstate(all="ignore"):
            r = O.corr(st.kernel, st.theta, O.l1_cross_distances(Xs[PILOT:], st.X)).reshape(BEHIND, -1)
        err_mu, err_w = np.abs(mu32 - r.dot(g)), np.abs(wd32 - r.dot(w))
        print("kernel %d ordinary %d d %2d %s: path %s, |S1| = %d; E_mu %.3g .. %.3g, max error %.3g, smallest margin / error %.3g"
              % (kernel, ordinary, d, acq, p1, rep[1], e_mu.min(), np.sort(e_mu)[-2], err_mu.max(), (e_mu / np.maximum(err_mu, 1e-300)).min()))  # fmt: skip
        assert np.all(err_mu <= e_mu) and np.all(err_w <= e_w)
        assert ordinary or np.all(wd32 == 0.0)
        na = ((Xs[PILOT:] * np.sqrt(st.theta)) ** 2).sum(axis=1)
        nb_max = float(((X * np.sqrt(st.theta)) ** 2).sum(axis=1).max())
        h_mu, h_w = BC.margins(kernel, d, na, nb_max, float(np.abs(g).sum()), float(np.abs(w).sum()))
        np.testing.assert_allclose(e_mu, h_mu, rtol=1e-8)
        np.testing.assert_allclose(e_w, h_w, rtol=1e-8)
        # every row the exact test keeps is flagged
        keep = TC.exact_flags(st, Xs, acq, pl)
        assert 8 * int(keep[:PILOT].sum()) <= PILOT
        assert not np.any(keep[PILOT:] & (flags == 0))
        # a second run: the same bytes, the same report, the same read-back
        v2, i2, p2, n2, rep2 = sweep_state(eng, acq, pl)
        assert (v2.tobytes(), i2.tobytes(), p2, n2, rep2) == (v1.tobytes(), i1.tobytes(), p1, n1, rep)
        assert tuple(a.tobytes() for a in eng.debug_bound32()) == tuple(a.tobytes() for a in dbg)
    finally:
        eng.close()
