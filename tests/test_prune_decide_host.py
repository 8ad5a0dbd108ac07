"""The two host decisions of the one-pass pruned sweep (bogp_prune_decide, csrc/bogp_internal.h: prune_decide) at their edges -- no
device, no handle.  More than an eighth of the pilot surviving its own thresholds sends the sweep to the per-chunk path; more than a
quarter of a segment surviving makes that segment fall back; shares of exactly 1/8 and 1/4 stay on the one-pass side."""
import pytest

from bogp import _lib

NONE, CHUNKS, ONEPASS, FALLBACK = (_lib.PRUNE_PATH_NONE, _lib.PRUNE_PATH_CHUNKS, _lib.PRUNE_PATH_ONEPASS, _lib.PRUNE_PATH_ONEPASS_FALLBACK)


@pytest.fixture(scope="module")
def decide():
    return _lib.load().bogp_prune_decide


def test_path_ids_match_the_header():
    import os
    import re

    from conftest import ROOT

    consts = dict(re.findall(r"#define\s+(BOGP_PRUNE_PATH_[A-Z_]+)\s+(\d+)", open(os.path.join(ROOT, "include", "bogp.h")).read()))
    assert {k: int(v) for k, v in consts.items()} == {"BOGP_PRUNE_PATH_NONE": NONE, "BOGP_PRUNE_PATH_CHUNKS": CHUNKS,
                                                       "BOGP_PRUNE_PATH_ONEPASS": ONEPASS, "BOGP_PRUNE_PATH_ONEPASS_FALLBACK": FALLBACK}  # fmt: skip


@pytest.mark.parametrize("pilot", [192, 4096, 8])
def test_pilot_share_of_exactly_an_eighth_stays_one_pass(decide, pilot):
    assert decide(pilot, pilot // 8, 1000, 0) == ONEPASS
    assert decide(pilot, pilot // 8 + 1, 1000, 0) == CHUNKS
    assert decide(pilot, pilot, 1000, 0) == CHUNKS  # nothing prunable (a zero or non-finite threshold lets every row through)


def test_pilot_share_is_not_rounded():
    d = _lib.load().bogp_prune_decide
    assert d(100, 12, 1000, 0) == ONEPASS  # 12 / 100 < 1 / 8 < 13 / 100: no integer division on the way
    assert d(100, 13, 1000, 0) == CHUNKS


@pytest.mark.parametrize("rows", [2809, 4, 2**21, 1_000_000 - 4096])
def test_segment_share_of_exactly_a_quarter_is_handled_in_rounds(decide, rows):
    q = rows // 4
    assert decide(4096, 0, rows, q) == ONEPASS
    assert decide(4096, 0, rows, q + 1) == FALLBACK
    assert decide(4096, 0, rows, rows) == FALLBACK


def test_zero_survivors(decide):
    assert decide(4096, 0, 1_000_000, 0) == ONEPASS
    assert decide(192, 0, 1, 0) == ONEPASS  # the pilot estimate itself: no segment bounded yet


def test_pilot_equal_to_the_whole_chunk(decide):
    """BOGP_CHUNK_MB small enough that chunk 0 is the pilot (192 rows at N = 544, 1 MiB): the same rule on those 192 rows."""
    assert decide(192, 24, 2809, 702) == ONEPASS  # both shares exact
    assert decide(192, 25, 2809, 0) == CHUNKS
    assert decide(192, 24, 2809, 703) == FALLBACK


def test_the_pilot_decision_comes_first(decide):
    assert decide(192, 192, 2809, 2809) == CHUNKS


def test_large_counts_do_not_overflow(decide):
    big = 2**40
    assert decide(big, big // 8, 4 * big, big) == ONEPASS
    assert decide(big, big // 8, 4 * big, big + 1) == FALLBACK
