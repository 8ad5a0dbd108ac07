"""The chunk geometry of every candidate pass (bogp_sweep_chunk_rows, csrc/bogp_internal.h: sweep_chunk_rows) -- no device, no handle.
Candidates per chunk = what the chunk bytes hold of columns of `rows` doubles, in whole 64-row tiles, at least 64 and at most M padded
to 64; negative above the largest chunk the kernels' 32-bit lane byte offsets reach, 8 (7 Mc + 30) < 2^32 (k_contract16d's voffA1 and
mm128_tile_direct's voffR1; k_corr_mfma's offR = 8 (3 Mc + 15) is smaller), which the sweeps turn into BOGP_ERR_UNSUPPORTED."""
import os
import re

import pytest

from bogp import _lib

MIB, GIB = 1 << 20, 1 << 30
# the largest whole-tile Mc with 8 * (7 * Mc + 30) < 2**32, from the three kernels' offset expressions -- not from the library
MC_MAX = ((2**32 - 1) // 8 - 30) // 7 // 64 * 64


@pytest.fixture(scope="module")
def rows_of():
    return _lib.load().bogp_sweep_chunk_rows


def test_the_bound_is_the_one_the_offsets_give():
    assert MC_MAX == 76_695_808
    assert 8 * (7 * MC_MAX + 30) < 2**32 <= 8 * (7 * (MC_MAX + 64) + 30)


@pytest.mark.parametrize("rows,M,chunk_bytes,expected", [
    (704, 9000, 8 * MIB, 1472),       # the chunked cases of tests/test_gpu_switches.py: seven chunks, the last one 168 rows
    (2048, 10**6, GIB, 65536),        # the default chunk at N = 2048
    (2048, 1000, GIB, 1024),          # clamped to M padded to 64
    (2048, 10, GIB, 64),              # M = 10: one tile
    (2048, 10**6, 2048 * 8 * 63, 64),  # a chunk too small for 64 rows: still one tile
    (2048, 10**6, 1, 64),
])  # fmt: skip
def test_chunk_rows(rows_of, rows, M, chunk_bytes, expected):
    assert rows_of(rows, M, chunk_bytes) == expected


@pytest.mark.parametrize("rows", [32, 544, 704, 2048, 4128])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 3001, 13005, 10**6])
@pytest.mark.parametrize("mb", [1, 8, 24, 1024])
def test_always_whole_tiles_within_the_candidates(rows_of, rows, M, mb):
    Mc = rows_of(rows, M, mb * MIB)
    assert Mc >= 64 and Mc % 64 == 0 and Mc <= (M + 63) // 64 * 64
    assert Mc == 64 or Mc * rows * 8 <= mb * MIB  # more than one tile only where the bytes hold it


def test_both_sides_of_the_offset_bound(rows_of):
    rows, M = 32, 2**40
    assert rows_of(rows, M, MC_MAX * rows * 8) == MC_MAX  # the last chunk the offsets reach
    assert rows_of(rows, M, (MC_MAX + 64) * rows * 8 - 1) == MC_MAX
    assert rows_of(rows, M, (MC_MAX + 64) * rows * 8) < 0  # the first one past it
    assert rows_of(rows, M, 2**40) < 0
    assert rows_of(rows, MC_MAX, 2**40) == MC_MAX  # (the clamp to the candidates comes first)
    assert rows_of(rows, MC_MAX + 1, 2**40) < 0


def test_large_counts_do_not_overflow(rows_of):
    big = 2**40
    assert rows_of(2048, big, GIB) == 65536
    assert rows_of(big, big, GIB) == 64  # rows * 8 = 2^43 bytes a candidate: one tile
    assert rows_of(2048, big, big * 2048 * 8) < 0  # 2^40 candidates a chunk, 2^54 bytes
    assert rows_of(1, big - 1, 2**62) < 0


@pytest.mark.parametrize("Np,S", [(32, 1), (256, 1), (288, 2), (2048, 8)])
def test_slices_of_the_training_set(Np, S):
    """S = ceil(Np / 32 / SWEEP_NBLK_PER_SPLIT) is a function of Np only; the slice width is the header's one constant."""
    from conftest import ROOT

    src = open(os.path.join(ROOT, "bayesian-optimization_amd", "csrc", "bogp_internal.h")).read()
    (width,) = re.findall(r"constexpr int SWEEP_NBLK_PER_SPLIT = (\d+);", src)
    assert int(width) == 8
    assert -(-(Np // 32) // int(width)) == S
    for f in ("bogp_api_sweep.hip", "bogp_api_believer.hip", "bogp_api_thompson.hip"):  # ... and nobody keeps a literal copy
        text = open(os.path.join(ROOT, "bayesian-optimization_amd", "csrc", f)).read()
        assert "nblk_per_split = 8" not in text and ("BOGP_CHUNK_MB\")" in text) == (f == "bogp_api_sweep.hip")
