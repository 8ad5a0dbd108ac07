"""The grid form of EHVI's cells, the parts that need no GPU: `pareto.hypercell_grid` expands to `hypercell_bounds`' cells bit for
bit, `pareto.ehvi_grid_numpy` (the factored sum of bogp_sweep_ehvi_grid) agrees with the float64 restatement of the reference's
algebra on those cells at ledger T12, and `EHVI(factored=True)` refuses what has no grid."""
import types

import numpy as np
import pytest

import bogp
from bogp import pareto
from support.ehvi_ref64 import ehvi as ehvi_ref


def _front(kind, m, rng):
    """(Y, ref_point) of a named front in m maximised objectives."""
    ref = -np.ones(m)
    if kind == "empty":
        return np.empty((0, m)), ref
    if kind == "one":
        return np.full((1, m), 0.5), ref
    if kind == "duplicate":  # two rows share their coordinate on axis 0: n_0 = 3 (m > 2: three front points, n_0 < P + 1; m = 2: one of the two is dominated)
        Y = np.zeros((3, m))
        Y[:, 0], Y[:, -1] = [0.7, 0.7, 0.2], [0.5, 0.1, 0.9]
        if m > 2:
            Y[:, 1] = [0.2, 0.6, 0.4]
        return Y, ref
    if kind == "below":  # two points at or below the reference point in one objective: they dominate nothing above it
        Y = rng.uniform(0.0, 1.0, size=(6, m))
        Y[0, 0], Y[1, -1] = -1.0, -1.5
        return Y, ref
    Y = rng.uniform(0.0, 1.0, size=(12, m))
    return Y / np.linalg.norm(Y, axis=1, keepdims=True), ref  # on a sphere: all 12 on the front


@pytest.mark.parametrize("m", [2, 3, 4])
@pytest.mark.parametrize("kind", ["empty", "one", "duplicate", "below", "random"])
def test_grid_expands_to_the_cells_and_the_factored_sum_is_their_ehvi(kind, m):
    rng = np.random.default_rng(10 * m + len(kind))
    Y, ref = _front(kind, m, rng)
    lower, upper = pareto.hypercell_bounds(Y, ref)
    grid = pareto.hypercell_grid(Y, ref)
    glo, ghi = pareto.expand_grid(grid)
    np.testing.assert_array_equal(glo, lower)
    np.testing.assert_array_equal(ghi, upper)
    assert grid.last_idx.dtype == np.int32 and len(grid.last_idx) == len(lower) == int(np.prod(grid.n_cells))
    assert np.all(np.diff(grid.last_val) > 0) and len(grid.last_val) <= len(pareto.pareto_front(Y, ref)) + 1
    if kind == "duplicate":
        assert grid.n_cells[0] == 3
    mu = rng.uniform(-1.5, 1.5, size=(40, m))
    mse = rng.uniform(0.05, 2.0, size=(40, m)) ** 2
    want = ehvi_ref(mu, mse, lower, upper)
    got = pareto.ehvi_grid_numpy(mu, mse, grid)
    assert np.all(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-12 * np.abs(want).max()), np.abs(got - want).max()  # T12


def test_constructor_refusals(monkeypatch):
    Y, ref = _front("random", 3, np.random.default_rng(1))
    model = object()
    crit = bogp.EHVI(model=model, ref_point=ref, Y=Y, factored=True)
    lower, upper = pareto.hypercell_bounds(Y, ref)
    np.testing.assert_array_equal(crit.cell_lower_bounds, lower)  # the cells stay: the point path and the gradient read them
    np.testing.assert_array_equal(pareto.expand_grid(crit.grid)[1], upper)
    assert bogp.EHVI(model=model, ref_point=ref, Y=Y).grid is None
    with pytest.raises(ValueError, match="factored"):
        bogp.EHVI(model=model, ref_point=ref, cells=(lower, upper), factored=True)

    part = types.SimpleNamespace(pareto_Y=pareto.pareto_front(Y, ref), get_hypercell_bounds=lambda: (lower, upper))
    with pytest.raises(ValueError, match="factored"):
        bogp.EHVI(model=model, ref_point=ref, partitioning=part, factored=True)
    monkeypatch.setattr(bogp.acquisition._forest, "is_forest_model", lambda mdl: True)
    with pytest.raises(NotImplementedError, match="factored"):
        bogp.EHVI(model=model, ref_point=ref, Y=Y, factored=True)
