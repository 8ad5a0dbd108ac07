"""The scalar criterion functions against exact values on the host (no GPU; ledger T20): the committed truth table
tests/golden/G46_criteria_truth.npz (oracle/make_criteria_table.py) belongs to the seeded draws of tests/criteria_cases.py and is
what mpmath gives; the REFERENCE's expressions (numpy + scipy.special.ndtr, as oracle.gp_oracle.acquisition restates
acquisition_fun.py) stay within the recorded multiple of each criterion's allowance, which is where the allowed factor F of the
library comes from; the draw reaches the tails, the centre and both sides of every switch; and the library's host halves
(bogp_feasibility, and bogp_acq_upper_bound with id EI, which is acq_value) meet the same F.  The device half is held to the same
table by tests/test_gpu_criteria.py."""
import numpy as np
import pytest

import criteria_cases as CC
from conftest import load_golden
from bogp import _lib


@pytest.fixture(scope="module")
def table():
    g = load_golden("G46_criteria_truth")
    out = {}
    for name in CC.NAMES:
        c = CC.draw(name)
        assert len(c["z"]) == CC.ROWS[name] == len(g[name + "_true"]) and CC.checksum(c) == float(g[name + "_checksum"]), name
        true, rlo = g[name + "_true"], g[name + "_rlo"]
        out[name] = (c, true, rlo, CC.allowance(name, c, true))
    return out


def test_table_is_smaller_than_the_limit_for_a_committed_file():
    import os

    from conftest import ROOT

    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "G46_criteria_truth.npz")) < 1 << 20


@pytest.mark.parametrize("name", CC.NAMES)
def test_reference_expressions_stay_within_the_recorded_ratio_and_the_draw_reaches_every_region(table, name):
    c, true, rlo, allow = table[name]
    ref = CC.reference(name, c)
    r, cmp = CC.ratios(ref, true, rlo, allow)
    print("T20 %-12s reference: worst |value - exact| / allowance = %.4g over %d of %d rows (recorded %.3g, F = %d)"
          % (name, r.max(), cmp.sum(), len(cmp), CC.REFERENCE_RATIO[name], CC.F[name]))  # fmt: skip
    assert np.all(np.isfinite(allow[cmp])) and np.all(allow[cmp] > 0)
    assert r.max() <= CC.REFERENCE_RATIO[name]          # what F was taken from ...
    assert CC.F[name] == int(np.ceil(4.0 * CC.REFERENCE_RATIO[name])) and r.max() > 0.8 * CC.REFERENCE_RATIO[name]  # ... and not a loose record of it
    assert CC.tiny_rows_ok(ref, cmp)
    for what, got, need in CC.draw_conditions(name, c, cmp):
        assert got >= need, (name, what, got, need)


def test_host_halves_of_the_library_meet_the_same_factor(table):
    lib = _lib.load()
    c, true, rlo, allow = table["EI"]
    v = np.array([lib.bogp_acq_upper_bound(_lib.ACQ_EI, 0.0, float(y), float(s), float(p), 1.0) for y, s, p in zip(c["y_hat"], c["sd"], c["plugin"])])
    r, cmp = CC.ratios(v, true, rlo, allow)
    print("T20 EI          host half:  worst ratio %.4g (F = %d)" % (r.max(), CC.F["EI"]))
    assert r.max() <= CC.F["EI"] and CC.tiny_rows_ok(v, cmp)
    c, true, rlo, allow = table["feasibility"]
    v = np.array([_lib.feasibility(m, s, 1.0, a, b) for m, s, a, b in zip(c["mu"], c["mse"], c["lo"], c["hi"])])
    r, cmp = CC.ratios(v, true, rlo, allow)
    print("T20 feasibility host half:  worst ratio %.4g (F = %d)" % (r.max(), CC.F["feasibility"]))
    assert r.max() <= CC.F["feasibility"] and CC.tiny_rows_ok(v, cmp)


@pytest.mark.parametrize("name", CC.NAMES)
def test_generator_reproduces_the_committed_table(table, name):
    pytest.importorskip("mpmath")
    c, true, rlo, _ = table[name]
    rows = np.random.default_rng(46).choice(len(true), size=min(2000, len(true)), replace=False)
    t2, r2 = CC.exact(name, c, rows)
    np.testing.assert_array_equal(t2, true[rows])
    np.testing.assert_array_equal(r2, rlo[rows])
