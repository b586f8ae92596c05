"""The tile-invariant lane offsets of the 8-wave dense instance (chromosight_amd/csrc/cs_corr_mfma_dense8.inc, Dense8Offsets)
on the CPU.

An inner tile's transfers and plain stores address memory as a uniform base, which the scalar unit forms per tile, plus a
32-bit byte offset per lane that the kernel forms once.  cs_dense8_offsets runs the kernel's own helper on the host: here its
offsets are compared with the division form (piece p = t + 512 k of a tile's 80 rows x 20 pieces: row p / 20, piece p % 20)
and with the store layout of the epilogue, written out below, and the route condition -- 80 rows of either pitch stay below
2^31 bytes, else the 4-wave instance -- must flip exactly there.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from chromosight_amd import _lib

GUARD_F32 = (1 << 31) // 320              # 80 ld 4 < 2^31  <=>  ld <= 6 710 886
GUARD_F64 = ((1 << 31) - 1) // 640        # 80 ld 8 < 2^31  <=>  ld <= 3 355 443
PITCHES = [80, 4099, 16387, GUARD_F32, GUARD_F32 + 1]


@pytest.fixture(scope="module")
def offsets():
    lib = _lib.load_library()

    def run(ld_in, ld_out, f64):
        fetch = (C.c_uint * (512 * 4))()
        store = (C.c_uint * 512)()
        rc = lib.cs_dense8_offsets(ld_in, ld_out, int(f64), fetch, store)
        return rc, np.ctypeslib.as_array(fetch).reshape(512, 4).astype(np.int64), np.ctypeslib.as_array(store).astype(np.int64)
    return run


def test_guard_values():
    assert 80 * GUARD_F32 * 4 < 2 ** 31 <= 80 * (GUARD_F32 + 1) * 4
    assert 80 * GUARD_F64 * 8 < 2 ** 31 <= 80 * (GUARD_F64 + 1) * 8


@pytest.mark.parametrize("ld_in", PITCHES)
def test_fetch_offsets_equal_the_division_form(offsets, ld_in):
    rc, fetch, _ = offsets(ld_in, 64, False)
    t = np.arange(512, dtype=np.int64)[:, None]
    k = np.arange(4, dtype=np.int64)[None, :]
    p = t + 512 * k
    r, c = p // 20, p % 20
    want = (r * ld_in + 4 * c) * 4
    assert np.array_equal(fetch, want % 2 ** 32)
    issued = p < 1600                     # the pieces a tile has: the fourth of a thread exists in wave 0 only
    assert np.array_equal(issued[:, 3], np.arange(512) < 64) and issued[:, :3].all()
    if rc == 1:
        # below the guard no issued piece wraps, each lies inside the tile's 80 rows, and together they tile it exactly
        assert np.array_equal(fetch[issued], want[issued])
        assert want[issued].max() + 16 == (79 * ld_in + 80) * 4 < 2 ** 31
        assert np.array_equal(np.sort(want[issued]), np.sort(((np.arange(80)[:, None] * ld_in + 4 * np.arange(20)[None, :]) * 4).ravel()))
    assert rc == (1 if ld_in <= GUARD_F32 else 0)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("ld_out", [64, 4100, 16388, GUARD_F64, GUARD_F64 + 1, GUARD_F32, GUARD_F32 + 1])
def test_store_offsets_equal_the_epilogue_layout(offsets, ld_out, f64):
    rc, _, store = offsets(80, ld_out, f64)
    elem = 8 if f64 else 4
    t = np.arange(512, dtype=np.int64)
    lane, wv = t & 63, t >> 6
    n, g = lane & 15, lane >> 4
    row = 16 * (wv & 3) + (n & 7)
    col = 32 * (wv >> 2) + np.where(n < 8, 0, 16) + 4 * g
    want = (row * ld_out + col) * elem
    assert np.array_equal(store, want % 2 ** 32)
    guard = GUARD_F64 if f64 else GUARD_F32
    assert rc == (1 if ld_out <= guard else 0)
    if rc == 1:
        # a thread's two stores (the second 8 rows below) of four values each cover the tile's 64 x 64 exactly once
        assert np.array_equal(store, want)
        first = np.concatenate([want, want + 8 * ld_out * elem]) // elem
        cells = (first[:, None] + np.arange(4)[None, :]).ravel()
        assert np.array_equal(np.sort(cells), np.sort((np.arange(64)[:, None] * ld_out + np.arange(64)[None, :]).ravel()))
        assert cells.max() * elem + elem == (63 * ld_out + 64) * elem < 2 ** 31


def test_route_condition_flips_at_the_guard(offsets):
    for ld_in, ld_out, f64, want in [(GUARD_F32, 64, False, 1), (GUARD_F32 + 1, 64, False, 0),
                                     (80, GUARD_F32, False, 1), (80, GUARD_F32 + 1, False, 0),
                                     (80, GUARD_F64, True, 1), (80, GUARD_F64 + 1, True, 0),
                                     (GUARD_F32, GUARD_F64, True, 1), (GUARD_F32 + 1, GUARD_F64, True, 0),
                                     (2 ** 40, 64, False, 0), (80, 2 ** 40, False, 0)]:
        assert offsets(ld_in, ld_out, f64)[0] == want, (ld_in, ld_out, f64)


def test_bad_arguments(offsets):
    lib = _lib.load_library()
    buf = (C.c_uint * 2048)()
    assert lib.cs_dense8_offsets(0, 64, 0, buf, buf) == -1
    assert lib.cs_dense8_offsets(80, -1, 0, buf, buf) == -1
    assert lib.cs_dense8_offsets(80, 64, 0, None, buf) == -1
