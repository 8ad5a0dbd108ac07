"""`ConstrainedEHVI(factored=True)` and `install(constrained_mobo_factored=True)`, the parts that need no GPU: the grid kept beside the
cells of the feasible front expands to those cells bit for bit, `sweep()` takes the grid entry, no feasible row leaves no grid, and
what has no grid is refused by name."""
import types

import numpy as np
import pytest

import bogp
from bogp import pareto


def _crit(hi, **kw):
    rng = np.random.default_rng(3)
    y = np.c_[rng.normal(size=(40, 3)), rng.normal(size=40)]  # three objectives, one constraint column
    calls = []
    eng = types.SimpleNamespace(sweep_ehvi_constrained_grid=lambda *a, **k: calls.append(("grid", a, k)),
                                sweep_ehvi_constrained=lambda *a, **k: calls.append(("loop", a, k)))  # fmt: skip
    model = types.SimpleNamespace(y=y, engine=eng, _committed_par=1)
    return bogp.ConstrainedEHVI(model=model, ref_point=np.full(3, -3.0), hi=[hi], **kw), y, calls


def test_the_grid_expands_to_the_cells_and_the_sweep_takes_it():
    crit, y, calls = _crit(0.0, factored=True)
    feasible = y[:, 3] <= 0.0
    assert 0 < crit.n_feasible == feasible.sum() < len(y)
    lower, upper = pareto.expand_grid(crit.grid)
    assert lower.tobytes() == crit.cell_lower_bounds.tobytes() and upper.tobytes() == crit.cell_upper_bounds.tobytes()
    assert np.array_equal(lower, pareto.hypercell_bounds(y[feasible, :3], crit.ref_point)[0])
    crit.sweep(k=3, return_values=True)
    assert [c[0] for c in calls] == ["grid"] and calls[0][1][0] is crit.grid and calls[0][2] == dict(k=3, return_values=True)
    plain, _, calls = _crit(0.0)
    plain.sweep()
    assert plain.grid is None and [c[0] for c in calls] == ["loop"]


def test_no_feasible_row_has_no_grid():
    crit, _, calls = _crit(-1e9, factored=True)
    assert crit.n_feasible == 0 and crit.grid is None and crit.feasibility_only
    crit.sweep()
    assert [c[0] for c in calls] == ["loop"] and calls[0][1][0].shape == (0, 3)


def test_what_has_no_grid_is_refused():
    plain, _, _ = _crit(0.0)
    with pytest.raises(ValueError, match="factored"):
        _crit(0.0, cells=(plain.cell_lower_bounds, plain.cell_upper_bounds), factored=True)
    with pytest.raises(ValueError, match="constrained_mobo_factored=True needs constrained_mobo=True"):
        bogp.install(object(), constrained_mobo_factored=True)
    with pytest.raises(ValueError, match="constrained_mobo_factored=True needs constrained_mobo=True"):
        bogp.install(object(), expensive_constraints=True, constrained_mobo_factored=True)
