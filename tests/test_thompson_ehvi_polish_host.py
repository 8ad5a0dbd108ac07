"""The polish of multi-objective Thompson batches on the host side (no GPU): the restatement `bogp.thompson.hvi_grad_numpy` against
central differences of its own value, which is `hvi_select_numpy`'s on `paths_multi_numpy`'s paths, and the refusals of the Python layer."""
import numpy as np
import pytest

import bogp
from bogp import _lib, pareto, thompson

BOX = (-2.0, 2.0)


@pytest.mark.parametrize("m", [2, 3])
@pytest.mark.parametrize("kernel", [_lib.KERNEL_SE, _lib.KERNEL_MATERN52])
def test_restatement_against_central_differences(kernel, m):
    """Tolerance (tests/test_thompson_polish_host.py's rule): the difference quotient's own error, estimated per case as max |FD(h) -
    FD(h / 2)| with h = 1e-5 of the box width, times 10 -- both sides relative to max |grad| of the case.  The front is one point 0.05
    above the lowest drawn vector over a reference point below every drawn vector: that point is dominated (HVI = 0, zero gradient), every
    cell has an infinite upper bound, and the other points lie inside such cells."""
    rng = np.random.default_rng(100 * kernel + m)
    N, d, q = 30, 3, 3
    X = rng.uniform(*BOX, size=(N, d))
    Y = np.column_stack([np.sin(X @ rng.normal(size=d)) + 0.1 * rng.normal(size=N) for _ in range(m)])
    st = thompson.dense_state_multi(X, Y, [0.7, 0.4, 1.0], kernel, beta=0.2)
    dr = thompson.draw_multi(st, q, 64, seed=kernel)
    pts = rng.uniform(BOX[0] + 0.1, BOX[1] - 0.1, size=(6, d))
    members, b = np.array([2, 0, 1, 1, 2, 0]), np.arange(6)
    y = thompson.paths_multi_numpy(st, dr, pts)[0][members, :, b]  # (6, m)
    dom = int(np.argmin(y.sum(axis=1)))
    lower, upper = pareto.hypercell_bounds(y[dom : dom + 1] + 0.05, y.min(axis=0) - 1.0)
    hvi, grad, parts = thompson.hvi_grad_numpy(st, dr, pts, members, lower, upper, parts=True)
    np.testing.assert_allclose(parts["y"], y, rtol=1e-9, atol=1e-12)
    sel = thompson.hvi_select_numpy(np.moveaxis(y, 0, 1)[None], lower, upper, st.sigma2)["A"][0]  # the sweep's own sum, cells in order
    np.testing.assert_allclose(hvi, np.where(sel > 0, sel, 0.0), rtol=1e-12)
    assert hvi[dom] == 0.0 and np.all(grad[dom] == 0.0) and np.all(parts["w"][dom] == 0.0)  # the dominated point
    inside = ((lower[None] < y[:, None]) & (y[:, None] < upper[None])).all(axis=2)  # (6, C): the point's vector lies inside the cell
    assert np.all(np.isinf(upper).any(axis=1)) and inside.any(axis=1).sum() >= 3 and np.count_nonzero(hvi) >= 3

    def fd(step):
        at = lambda e: thompson.hvi_grad_numpy(st, dr, pts + e, members, lower, upper)[0]  # noqa: E731
        return np.stack([(at(step * e) - at(-step * e)) / (2 * step) for e in np.eye(d)], axis=1)

    a, a2 = fd(1e-5 * (BOX[1] - BOX[0])), fd(0.5e-5 * (BOX[1] - BOX[0]))
    err, own, scale = np.abs(grad - a).max(), np.abs(a - a2).max(), np.abs(grad).max()
    print("kernel=%d m=%d: |grad - FD| / max|grad| = %.3g, FD's own error estimate %.3g" % (kernel, m, err / scale, own / scale))
    assert scale > 0 and err / scale <= 10.0 * own / scale
    # from_device: the scalarisation alone, on given y and J -- the same bytes as the full restatement
    again = thompson.hvi_grad_numpy(None, None, None, None, lower, upper, from_device=(parts["y"], parts["jac"]))
    np.testing.assert_array_equal(again[0], hvi), np.testing.assert_array_equal(again[1], grad)


def test_a_nan_value_and_the_refusals():
    hvi, grad, _ = thompson.hvi_scalarise_numpy([[0.5, np.nan]], np.ones((1, 2, 3)), [[0.0, 0.0]], [[1.0, np.inf]])
    assert hvi[0] == -np.inf and np.all(grad == 0.0)
    with pytest.raises(ValueError, match="ehvi_thompson_polish"):
        bogp.integration.install(bayes_optim=object(), ehvi_thompson_polish=True)
