"""The Thompson polish on the host side (no GPU): the restatement `bogp.thompson.path_grad_numpy` against central differences of
`paths_numpy`, and `thompson_batch(polish=True)` with its routing and refusals on the stand-in engine of
tests/support/thompson_polish_engine.py."""
import numpy as np
import pytest

import bogp
from bogp import _lib, optim, thompson
from support.thompson_polish_engine import ThompsonPolishOracleEngine

KERNELS, BOX = [_lib.KERNEL_SE, _lib.KERNEL_MATERN12, _lib.KERNEL_MATERN32, _lib.KERNEL_MATERN52, _lib.KERNEL_ABSEXP], (-2.0, 2.0)


@pytest.mark.parametrize("flavour", ["ordinary", "simple", "prior"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_restatement_against_central_differences(kernel, flavour):
    """Tolerance (ledger T15's rule): the difference quotient's own error, estimated per case as max |FD(h) - FD(h / 2)| with
    h = 1e-5 of the box width, times 10 -- both sides relative to max |grad| of the case.  The value is `paths_numpy`'s to rounding."""
    rng = np.random.default_rng(100 * kernel + len(flavour))
    N, d, q, cond = 30, 3, 4, flavour != "prior"
    X = rng.uniform(*BOX, size=(N, d))
    st = thompson.dense_state(X, np.sin(X @ rng.normal(size=d)) + 0.1 * rng.normal(size=N), [0.7, 0.4, 1.0], kernel, flavour != "simple", beta=0.2)
    dr = thompson.draw(st, q, 64, seed=kernel)
    pts = rng.uniform(BOX[0] + 0.1, BOX[1] - 0.1, size=(6, d))  # away from the training set (a continuous draw)
    members, b = np.array([3, 0, 2, 2, 1, 0]), np.arange(6)
    val, grad = thompson.path_grad_numpy(st, dr, pts, members, conditioned=cond)
    np.testing.assert_allclose(val, thompson.paths_numpy(st, dr, pts, cond)[0][members, b], rtol=1e-9, atol=1e-12)

    def fd(step):
        at = lambda e: thompson.paths_numpy(st, dr, pts + e, cond)[0][members, b]  # noqa: E731
        return np.stack([(at(step * e) - at(-step * e)) / (2 * step) for e in np.eye(d)], axis=1)

    a, a2 = fd(1e-5 * (BOX[1] - BOX[0])), fd(0.5e-5 * (BOX[1] - BOX[0]))
    err, own, scale = np.abs(grad - a).max(), np.abs(a - a2).max(), np.abs(grad).max()
    print("kernel=%d %s: |grad - FD| / max|grad| = %.3g, FD's own error estimate %.3g" % (kernel, flavour, err / scale, own / scale))
    assert err / scale <= 10.0 * own / scale


@pytest.fixture()
def gp():  # on the stand-in engine
    rng = np.random.default_rng(15)
    X = rng.uniform(-2, 2, size=(40, 3))
    model = bogp.GaussianProcess(corr="matern", thetaL=[1e-3] * 3, thetaU=[1e2] * 3, nugget=0)
    model._engine = ThompsonPolishOracleEngine()
    model.set_state(np.r_[0.9, 0.6, 1.2], X, np.sin(X @ rng.normal(size=3)) + 0.1 * rng.normal(size=40))
    return model


def _box():
    return optim.Box([(-2.2, 2.2)] * 3, random_seed=3)


@pytest.mark.parametrize("minimize", [True, False])
def test_polished_batch(gp, minimize):
    eng, Xs = gp.engine, np.random.default_rng(21).uniform(-2.2, 2.2, size=(300, 3))
    kw = dict(q=3, n_features=64, seed=4, Xs=Xs, minimize=minimize)
    pol = dict(polish=True, n_starts=4, max_iter=30)
    plain = bogp.thompson_batch(gp, _box(), 300, **kw)
    eng.calls.clear()
    assert bogp.thompson_batch(gp, _box(), 300, **kw) == plain and eng.calls == [("upload", 300), ("sweep_thompson", 3, 8, True)]  # the default is unchanged
    eng.calls.clear()
    xs, fs = bogp.thompson_batch(gp, _box(), 300, **pol, **kw)
    # one sweep with enough ranks, ONE polish call over paths x n_starts starts
    assert eng.calls == [("upload", 300), ("sweep_thompson", 3, 8, True), ("polish_path", 12, [0] * 4 + [1] * 4 + [2] * 4, 30)]
    assert len({tuple(x) for x in xs}) == 3 and np.all(np.abs(np.array(xs)) <= 2.2)
    sign = -1.0 if minimize else 1.0  # polished: no worse than the sweep's pick, and not all equal to it
    assert all(sign * f >= sign * p for f, p in zip(fs, plain[1])) and any(f != p for f, p in zip(fs, plain[1]))
    np.testing.assert_allclose(fs, thompson.path_grad_numpy(gp, thompson.draw(gp, 3, 64, seed=4), np.array(xs), [0, 1, 2])[0], rtol=1e-12)  # fopt: the path there
    # a proposal np.isclose to an evaluated point gives way to the path's next polished point; the other paths keep theirs
    xs2, fs2 = bogp.thompson_batch(gp, _box(), 300, history=np.array([xs[0]]), **pol, **kw)
    assert not np.allclose(xs2[0], xs[0]) and sign * fs2[0] <= sign * fs[0] and xs2[1:] == xs[1:]
    crits = [bogp.UCB(model=gp, alpha=1.0, minimize=minimize)] * 3  # batch_argmax passes the keywords through
    assert bogp.batch_argmax(crits, _box(), 300, Xs=Xs, seed=4, strategy="thompson", **pol) == \
        bogp.thompson_batch(gp, _box(), 300, **pol, **dict(kw, n_features=1024))


def test_refusals(gp, monkeypatch):
    Xs = np.zeros((10, 3))
    with pytest.raises(ValueError, match="strategy='thompson'"):
        bogp.batch_argmax([bogp.MGFI(model=gp, t=1.0)], _box(), 10, Xs=Xs, polish=True)
    with pytest.raises(ValueError, match="thompson_polish"):
        bogp.integration.install(bayes_optim=object(), thompson_polish=True)
    with pytest.raises(ValueError, match="n_starts"):
        bogp.thompson_batch(gp, _box(), 10, q=2, Xs=Xs, polish=True, n_starts=0)
    monkeypatch.setattr(gp, "kernel_id", _lib.KERNEL_MATERN_NU), monkeypatch.setattr(gp, "_nu", 0.8)
    with pytest.raises(NotImplementedError, match="general-nu Matern"):
        bogp.thompson_batch(gp, _box(), 10, q=2, Xs=Xs, polish=True)
