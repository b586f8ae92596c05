"""The tile walk of the 8-wave dense instance (chromosight_amd/csrc/cs_corr_mfma_dense8.inc, DenseTileWalk) on the CPU.

The kernel carries its tile row, tile column and the row's skew from tile to tile with additions and compares;
cs_dense_tile_walk runs that same helper on the host and returns the (I0, J0) origins of one workgroup's tiles.  Here the
sequence of every workgroup is compared with the division form the kernel used before (and the 4-wave instance still
uses, cs_corr_mfma_body.inc tile_origin), written out below, and every tile must be visited exactly once.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from chromosight_amd import _lib

MF_T = 64
GRIDS_8 = list(range(8, 513, 8))                 # every multiple of 8 up to two workgroups on each of 256 CUs
GRIDS_ODD = [1, 5, 100, 257, 509]                # not multiples of 8: one range for all workgroups, step = grid
TILES_Y = [1, 2, 9, 31, 72]                      # 72 x 70 = 8 x 70 x 9 tiles at the widest


@pytest.fixture(scope="module")
def walk():
    lib = _lib.load_library()
    fn = lib.cs_dense_tile_walk
    cap = 8 * 70 * 9
    i0 = (C.c_int * cap)()
    j0 = (C.c_int * cap)()

    def run(tiles_x, n_tiles, grid, xcd_order, row_begin, block):
        n = fn(tiles_x, n_tiles, grid, xcd_order, row_begin, block, i0, j0, cap)
        assert 0 <= n <= cap
        return np.ctypeslib.as_array(i0)[:n].copy(), np.ctypeslib.as_array(j0)[:n].copy()
    return run


def division_form(tiles_x, n_tiles, grid, xcd_order, row_begin, block):
    """Tiles of workgroup `block` and their origins: one division and one remainder per tile."""
    if (xcd_order & 1) and grid % 8 == 0:
        x, per = block & 7, (n_tiles + 7) // 8
        tiles = np.arange(x * per + (block >> 3), min(n_tiles, (x + 1) * per), grid >> 3)
    else:
        tiles = np.arange(block, n_tiles, grid)
    by = tiles // tiles_x
    bx = tiles - by * tiles_x
    skew = xcd_order >> 1
    if skew:
        bx = bx + (by * skew) % tiles_x
        bx = bx - np.where(bx >= tiles_x, tiles_x, 0)
    return tiles, row_begin + by * MF_T, bx * MF_T


def tiles_of_origins(i0, j0, tiles_x, xcd_order, row_begin):
    """The row-major tile indices that returned origins stand for: the skew of the tile row taken out again."""
    assert np.all((i0 - row_begin) % MF_T == 0) and np.all(j0 % MF_T == 0)
    by, col = (i0 - row_begin) // MF_T, j0 // MF_T
    assert np.all((col >= 0) & (col < tiles_x)) and np.all(by >= 0)
    return by * tiles_x + (col - by * (xcd_order >> 1)) % tiles_x


def check_case(walk, tiles_x, n_tiles, grid, xcd_order, row_begin):
    visited = []
    for block in range(grid):
        tiles, want_i, want_j = division_form(tiles_x, n_tiles, grid, xcd_order, row_begin, block)
        got_i, got_j = walk(tiles_x, n_tiles, grid, xcd_order, row_begin, block)
        where = (tiles_x, n_tiles, grid, xcd_order, row_begin, block)
        assert len(got_i) == len(tiles), where
        assert np.array_equal(got_i, want_i), where
        assert np.array_equal(got_j, want_j), where
        visited.append(tiles_of_origins(got_i, got_j, tiles_x, xcd_order, row_begin))
    # every tile exactly once, counted on what the walk itself returned
    assert np.array_equal(np.sort(np.concatenate(visited)), np.arange(n_tiles)), (tiles_x, n_tiles, grid, xcd_order)


def cases():
    """Every tiles_x in 1 .. 70 with every skew, each with four grids in multiples of 8 (all 64 of them come round 17 times)
    and one that is no multiple; tile rows and row_begin rotate."""
    out, k = [], 0
    for tiles_x in range(1, 71):
        for skew in range(4):
            for _ in range(4):
                out.append((tiles_x, tiles_x * TILES_Y[k % 5], GRIDS_8[(37 * k) % 64], 1 | (skew << 1), (0, 37, 4096)[k % 3]))
                k += 1
            out.append((tiles_x, tiles_x * TILES_Y[(k + 2) % 5], GRIDS_ODD[k % 5], 1 | (skew << 1), 37))
    return out


CASES = cases()


def test_cases_cover_what_they_claim():
    assert {c[0] for c in CASES} == set(range(1, 71))
    assert {c[2] for c in CASES} >= set(GRIDS_8) | set(GRIDS_ODD)
    assert max(c[1] for c in CASES) == 8 * 70 * 9
    assert {(c[0], c[3] >> 1) for c in CASES} == {(t, s) for t in range(1, 71) for s in range(4)}
    assert any(c[4] != 0 for c in CASES)


@pytest.mark.parametrize("part", range(7))
def test_walk_equals_the_division_form(walk, part):
    for tiles_x, n_tiles, grid, xcd_order, row_begin in CASES[part::7]:
        check_case(walk, tiles_x, n_tiles, grid, xcd_order, row_begin)


def test_shapes_of_the_gpu_test(walk):
    """The launches of tests/test_gpu_mfma_dense8_walk.py on a 256-CU part, and the headline 4096 x 4096 map (skew 1)."""
    for tiles_x, tiles_y, skew, row_begin in [(32, 48, 1, 0), (16, 35, 1, 0), (17, 33, 0, 0), (5, 2, 0, 37), (64, 64, 1, 0)]:
        n_tiles = tiles_x * tiles_y
        check_case(walk, tiles_x, n_tiles, min(n_tiles, 512), 1 | (skew << 1), row_begin)


def test_range_ends_that_are_no_multiple_of_the_step(walk):
    """n_tiles that 8 does not divide (the last XCD's range is short or empty), a map smaller than the grid, bit 0 of
    xcd_order clear (one range for all workgroups)."""
    for tiles_x, n_tiles, grid in [(7, 7 * 9 + 0, 64), (13, 13 * 5, 512), (3, 3, 8), (1, 1, 16), (70, 70 * 9, 24), (9, 9 * 11, 40)]:
        for skew in range(4):
            check_case(walk, tiles_x, n_tiles, grid, 1 | (skew << 1), 0)
            check_case(walk, tiles_x, n_tiles, grid, skew << 1, 64)


def test_bad_arguments(walk):
    lib = _lib.load_library()
    buf = (C.c_int * 4)()
    assert lib.cs_dense_tile_walk(0, 10, 8, 1, 0, 0, buf, buf, 4) == -1
    assert lib.cs_dense_tile_walk(4, 10, 8, 1, 0, 8, buf, buf, 4) == -1
    assert lib.cs_dense_tile_walk(4, 10, 0, 1, 0, 0, buf, buf, 4) == -1
    # more tiles than `cap`: the count is returned, the arrays are filled up to cap
    assert lib.cs_dense_tile_walk(4, 400, 8, 1, 0, 0, buf, buf, 4) == 50
