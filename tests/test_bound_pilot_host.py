"""The cases of tests/test_gpu_bound_pilot.py, checked on the host with the oracle (no device): for the pilot the exact bounds would
choose, no bound behind it lies within 1e-6 relative of its threshold -- so the device's survivor count, taken with a 1e-9 margin, is
the host's -- and fewer than a quarter of the rows survive, so the segment stays on the one-pass path.  The device's own pilot is
checked the same way in the GPU test, from the indices it reports."""
import numpy as np
import pytest

import bound_pilot_cases as BP
import prune_cases as PC


@pytest.fixture(scope="module")
def models():
    return {ordinary: PC.model(ordinary) for ordinary in (False, True)}


@pytest.mark.parametrize("block_rows", BP.BLOCKS)
@pytest.mark.parametrize("name,acq,minimize", BP.COUNTED)
def test_counted_cases_keep_their_distance_and_stay_one_pass(models, name, acq, minimize, block_rows):
    for ordinary in (False, True):
        X, y, par, st = models[ordinary]
        Xs = PC.candidates()
        vals, bounds, nan = BP.rows_view(st, Xs, acq, BP.plugin_of(y, minimize), minimize)
        pilot = BP.exact_pilot(bounds, nan, block_rows)
        blocks = (len(Xs) + block_rows - 1) // block_rows
        assert len(pilot) <= len(acq) * blocks
        surv, gap = BP.survivors_behind(vals, bounds, nan, pilot)
        print("%s, ordinary %d, B = %d: pilot %d rows, %d survivors, smallest distance %.3g" % (name, ordinary, block_rows, len(pilot), surv, gap))
        assert gap > BP.GAP and 4 * surv <= len(Xs)


def test_exact_pilot_takes_the_first_of_equal_bounds_and_a_nan_row_first():
    b = np.array([[1.0, 3.0, 3.0, 2.0, 5.0, 5.0]])
    nan = np.zeros(6, dtype=bool)
    assert BP.exact_pilot(b, nan, 3).tolist() == [1, 4]
    nan[2] = True
    assert BP.exact_pilot(b, nan, 3).tolist() == [2, 4]
    vals = np.array([[0.5, 2.5, 0.0, 1.0, 4.0, 4.5]])
    nan[2] = False
    surv, gap = BP.survivors_behind(vals, b, nan, np.array([1, 4]))  # threshold 4.0: row 5 (bound 5) survives alone
    assert surv == 1 and gap == pytest.approx(0.2)
