"""The automatic candidate tile of the direct contraction (bogp_contract_tile_rows; csrc/bogp_internal.h: contract_tile_rows, DESIGN.md
section 5.2''') at its edges -- no device: 64 rows from CONTRACT_TILE64_MIN_WG_PER_4CU workgroups of the 64-row grid per four CUs, 32
rows from CONTRACT_TILE32_MIN_WG_PER_4CU, else 16; 64 for every gated launch; and the setter's argument check."""
import pytest

from bogp import _lib

Q64, Q32 = _lib.CONTRACT_TILE64_MIN_WG_PER_4CU, _lib.CONTRACT_TILE32_MIN_WG_PER_4CU
CUS = (1, 4, 64, 256, 304, 100000)


@pytest.fixture(scope="module")
def rows():
    fn = _lib.load().bogp_contract_tile_rows
    return lambda tiles, nJ, n_cu, live=0: fn(int(tiles), int(nJ), int(n_cu), int(live))


def restated(tiles, nJ, n_cu):
    wg4 = 4 * tiles * nJ
    return 64 if wg4 >= Q64 * n_cu else 32 if wg4 >= Q32 * n_cu else 16


def test_the_constants_order_the_tiles():
    assert 0 < Q32 < Q64


@pytest.mark.parametrize("n_cu", CUS)
@pytest.mark.parametrize("nJ", [1, 3, 5, 8, 32])
def test_more_rows_never_choose_a_narrower_tile(rows, nJ, n_cu):
    top = (Q64 * n_cu) // (4 * nJ) + 3
    probe = sorted(set(list(range(1, min(top, 400) + 1)) + [top - 2, top - 1, top, top + 1, 10 * top, 1 << 24]))
    got = [rows(t, nJ, n_cu) for t in probe]
    assert set(got) <= {16, 32, 64}
    assert got == sorted(got), list(zip(probe, got))
    assert got[-1] == 64
    assert got == [restated(t, nJ, n_cu) for t in probe]


@pytest.mark.parametrize("n_cu", CUS)
@pytest.mark.parametrize("nJ", [1, 3, 8])
def test_each_crossover_is_exact_one_row_tile_either_side(rows, nJ, n_cu):
    for q, below, at in ((Q64, None, 64), (Q32, 16, None)):
        t = -(-q * n_cu // (4 * nJ))  # the first row-tile count with 4 t nJ >= q n_cu
        assert 4 * t * nJ >= q * n_cu > 4 * (t - 1) * nJ
        hi, lo = rows(t, nJ, n_cu), rows(t - 1, nJ, n_cu) if t > 1 else None
        if at:
            assert hi == at and (lo is None or lo < at)
        else:
            assert hi >= 32 and (lo is None or lo == below)


def test_the_256_cu_device_at_the_sizes_of_the_flagship_sweep(rows):
    """N = 2048: eight column groups.  The survivors' round (13 row tiles: 104 workgroups of the 64-row grid) is below one workgroup a
    CU, the 4096-row pilot (512 workgroups) is two a CU, a whole chunk is far above four."""
    assert rows(13, 8, 256) == restated(13, 8, 256) == 16
    assert rows(64, 8, 256) == restated(64, 8, 256)
    assert rows(15625, 8, 256) == 64


@pytest.mark.parametrize("n_cu", CUS)
def test_a_gated_launch_keeps_64_rows(rows, n_cu):
    for tiles in (1, 2, 13, 64, 5000):
        for nJ in (1, 3, 8):
            assert rows(tiles, nJ, n_cu, live=1) == 64


def test_one_cu_and_a_large_device(rows):
    assert rows(1, 1, 1) == restated(1, 1, 1) and rows(Q64, 1, 1) == 64  # one CU: every launch of four workgroups or more fills it
    assert rows(64, 8, 100000) == 16 and rows(1 << 24, 8, 100000) == 64
    assert rows(1, 1, 0) == rows(1, 1, 1)  # an unknown CU count counts as one


def test_the_setter_refuses_everything_but_0_16_32_64():
    eng = _lib.Engine.__new__(_lib.Engine)  # no device: the binding checks the argument before it calls the library
    for bad in (-1, 1, 8, 24, 48, 63, 65, 128, 6.4):
        with pytest.raises(ValueError):
            eng.set_contract_tile(bad)
    assert _lib.load().bogp_set_contract_tile(None, 7) == _lib.ERR_INVALID  # the library: no handle, no effect
