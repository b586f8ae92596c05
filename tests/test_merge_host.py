"""The host side of the merging of pixel tables (chromosight_amd/merge.py) and the tools of its device tests
(tests/merge_util.py): the oracle on a hand-written example, the multinomial split, the refusals of check_compatible and the
shapes the adversarial genome must hold.  No GPU."""
import types

import numpy as np
import pytest

from chromosight_amd import merge as cmg
from tests import merge_util as mu
from tests.merge_util import adversarial_sources, make_cool, oracle_merge, split_counts

TILE_COLUMNS_ASSUMED = 2048         # the column tile the adversarial genome is sized for (tests/test_gpu_merge.py holds the library to it)


def test_oracle_on_a_hand_written_example():
    sizes = [2, 3, 1]                                   # bins 0-1, 2-4, 5
    a = make_cool(sizes, [0, 0, 1, 2, 4], [0, 5, 3, 2, 4], [1, 2, 3, 4, 0])
    b = make_cool(sizes, [0, 1, 3, 4, 5], [5, 3, 4, 4, 5], [10, 20, 30, 0, 7])
    c = make_cool(sizes, [], [], np.zeros(0, dtype=np.int64))
    got = oracle_merge([a, b, c])
    # (4, 4) is a stored zero in both tables that have it: dropped
    assert got["bin1_id"].tolist() == [0, 0, 1, 2, 3, 5]
    assert got["bin2_id"].tolist() == [0, 5, 3, 2, 4, 5]
    assert got["count"].tolist() == [1, 12, 23, 4, 30, 7]
    assert got["count"].dtype == np.int64 and got["val_dtype"] is np.float32
    assert got["chrom_offset"].tolist() == [0, 2, 5, 6] and got["binsize"] == 1000 and got["weight"] is None
    # any order of the tables, and a table merged with nothing, give the same
    again = oracle_merge([c, b, a])
    assert all(np.array_equal(got[k], again[k]) for k in ("bin1_id", "bin2_id", "count"))
    alone = oracle_merge([a])
    assert alone["bin1_id"].tolist() == [0, 0, 1, 2] and alone["count"].tolist() == [1, 2, 3, 4]
    assert oracle_merge([c, c])["count"].size == 0 and oracle_merge([c])["val_dtype"] is np.float32


def test_oracle_dtype_follows_the_largest_sum():
    lo = make_cool([3], [0], [1], [(1 << 23)])
    hi = make_cool([3], [0], [1], [(1 << 23) - 1])
    assert oracle_merge([lo, hi])["count"].tolist() == [(1 << 24) - 1] and oracle_merge([lo, hi])["val_dtype"] is np.float32
    assert oracle_merge([lo, lo])["count"].tolist() == [1 << 24] and oracle_merge([lo, lo])["val_dtype"] is np.float64


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_split_counts_sums_back(k):
    rng = np.random.default_rng(5)
    b1 = rng.integers(0, 50, size=400)
    b2 = rng.integers(0, 50, size=400)
    keys = np.unique(np.minimum(b1, b2) * 50 + np.maximum(b1, b2))
    cool = make_cool([20, 30], keys // 50, keys % 50, rng.integers(0, 12, size=keys.size))
    parts = split_counts(cool, k, seed=3)
    assert len(parts) == k
    total = np.zeros(keys.size, dtype=np.int64)
    for part in parts:
        assert np.array_equal(part["bin1_id"], cool["bin1_id"]) and np.array_equal(part["bin2_id"], cool["bin2_id"])
        assert part["count"].dtype == np.int64 and part["count"].min() >= 0
        total += part["count"]
    assert np.array_equal(total, cool["count"])
    if k > 1:
        assert any((part["count"] == 0).any() for part in parts)          # stored zeros stay in their table
    again = split_counts(cool, k, seed=3)
    assert all(np.array_equal(x["count"], y["count"]) for x, y in zip(parts, again))
    merged, want = oracle_merge(parts), oracle_merge([cool])
    assert all(np.array_equal(merged[key], want[key]) for key in ("bin1_id", "bin2_id", "count"))


# ---- check_compatible on objects that only carry geometry -------------------------------------------------------------------
def _geometry(dev="dev0", names=("a", "b"), offsets=(0, 4, 9), binsize=1000, bin_start=None, bin_end=None):
    return types.SimpleNamespace(dev=dev, names=list(names), offsets=np.asarray(offsets, dtype=np.int64), binsize=binsize,
                                 bin_start=bin_start, bin_end=bin_end)


def test_check_compatible_accepts_equal_geometry():
    dev = object()
    start = np.arange(9) * 1000
    tables = [_geometry(dev=dev), _geometry(dev=dev, bin_start=start, bin_end=start + 1000), _geometry(dev=dev, bin_start=start.copy())]
    assert cmg.check_compatible(tables) == tables
    assert cmg.check_compatible(iter(tables[:1])) == tables[:1]
    assert len(cmg.check_compatible([_geometry(dev=dev)] * cmg.MAX_SOURCES)) == 64


@pytest.mark.parametrize("change, match", [
    (dict(dev="dev1"), "device"),
    (dict(names=("a", "c")), "names"),
    (dict(names=("a", "b", "c")), "names"),
    (dict(offsets=(0, 5, 9)), "offsets"),
    (dict(offsets=(0, 4, 10)), "offsets"),
    (dict(binsize=2000), "2000"),
    (dict(bin_start=np.arange(9) * 1000 + 1), "coordinates"),
    (dict(bin_end=np.arange(9) * 1000 + 999), "coordinates"),
])
def test_check_compatible_refuses(change, match):
    start = np.arange(9) * 1000
    first = _geometry(bin_start=start, bin_end=start + 1000)
    same = _geometry(bin_start=start, bin_end=start + 1000)
    other = _geometry(**{**dict(bin_start=start, bin_end=start + 1000), **change})
    with pytest.raises(ValueError, match=match):
        cmg.check_compatible([first, same, other])
    with pytest.raises(ValueError, match=match):
        cmg.check_compatible([other, first])


def test_check_compatible_refuses_no_source_and_more_than_64():
    with pytest.raises(ValueError, match="at least one"):
        cmg.check_compatible([])
    with pytest.raises(ValueError, match="64"):
        cmg.check_compatible([_geometry()] * 65)


def test_tile_columns_come_from_the_library():
    from chromosight_amd._lib import load_library
    assert cmg.TILE_COLUMNS == load_library().cs_merge_tile_columns() > 0
    assert cmg.TILE_COLUMNS % 64 == 0                   # whole ballot words


# ---- the adversarial genome -------------------------------------------------------------------------------------------------
def _row(cool, row):
    sel = np.asarray(cool["bin1_id"]) == row
    return dict(zip(np.asarray(cool["bin2_id"])[sel].tolist(), np.asarray(cool["count"])[sel].tolist()))


def test_the_genome_is_wider_than_two_tiles_and_stays_small():
    assert mu.ASSUMED_TILE_COLUMNS == TILE_COLUMNS_ASSUMED
    assert len(mu.SIZES) == 3 and mu.SIZES[2] > 2 * TILE_COLUMNS_ASSUMED
    assert sum(mu.SIZES) < 5000
    assert mu.SOURCE_COUNTS == (1, 2, 3, 8, 64)


@pytest.mark.parametrize("k", mu.SOURCE_COUNTS)
def test_the_adversarial_genome_holds_every_listed_shape(k):
    src = adversarial_sources(k)
    n = sum(mu.SIZES)
    assert len(src) == k
    for cool in src:
        b1, b2 = cool["bin1_id"], cool["bin2_id"]
        assert cool["chrom_offset"].tolist() == [0, 5, 75, n]
        assert np.all(b2 >= b1) and b2.max() < n                       # upper triangle, inside the table
        key = b1 * n + b2
        assert np.all(np.diff(key) > 0)                                # sorted, no duplicates
        assert cool["count"].dtype == np.int64 and cool["count"].min() >= 0

    class Rows(dict):                                   # row -> what every source holds there
        def __missing__(self, r):
            self[r] = [_row(cool, r) for cool in src]
            return self[r]
    rows = Rows()
    # empty in every source, present in exactly one, identical in all
    assert all(not r for r in rows[mu.ROW_EMPTY])
    assert sum(bool(r) for r in rows[mu.ROW_ONE_SOURCE]) == 1
    assert rows[mu.ROW_IDENTICAL][0] and all(r == rows[mu.ROW_IDENTICAL][0] for r in rows[mu.ROW_IDENTICAL])
    # first and last column of the table, last row
    assert 0 in rows[mu.ROW_IDENTICAL][0] and n - 1 in rows[mu.ROW_IDENTICAL][0]
    assert all(n - 1 in r for r in rows[n - 1])
    # either side of the first tile boundary
    assert {TILE_COLUMNS_ASSUMED - 1, TILE_COLUMNS_ASSUMED} <= set(rows[mu.ROW_IDENTICAL][0])
    # interleaved: source s holds the columns = s mod k, together all of them
    for s, r in enumerate(rows[mu.ROW_INTERLEAVED]):
        assert sorted(r) == [c for c in range(mu.ROW_INTERLEAVED, n) if c % k == s]
    # one pixel against runs of 63 / 64 / 65 / 257
    assert len(rows[mu.ROW_LONE_PIXEL][0]) == 1
    lengths = [len(r) for r in rows[mu.ROW_LONE_PIXEL][1:]]
    assert lengths == [mu.RUN_LENGTHS[i % 4] for i in range(k - 1)]
    if k >= 8:
        assert set(lengths) == {63, 64, 65, 257}
    # dense in one source, sparse in the rest
    assert sorted(rows[mu.ROW_DENSE][0]) == list(range(mu.ROW_DENSE, n))
    assert all(len(r) == 5 for r in rows[mu.ROW_DENSE][1:])
    # stored zeros that sum to zero, and one that meets a count
    assert all(r[mu.COL_ZERO_IN_ALL] == 0 for r in rows[mu.ROW_ZEROS])
    assert rows[mu.ROW_ZEROS][0][mu.COL_ZERO_ALONE] == 0 and all(mu.COL_ZERO_ALONE not in r for r in rows[mu.ROW_ZEROS][1:])
    assert rows[mu.ROW_ZEROS][0][mu.COL_ZERO_MEETS_COUNT] == 0
    want = oracle_merge(src)
    merged = _row(want, mu.ROW_ZEROS)
    assert mu.COL_ZERO_IN_ALL not in merged and mu.COL_ZERO_ALONE not in merged
    if k > 1:
        assert rows[mu.ROW_ZEROS][k - 1][mu.COL_ZERO_MEETS_COUNT] == 5 and merged[mu.COL_ZERO_MEETS_COUNT] == 5
    else:
        assert mu.COL_ZERO_MEETS_COUNT not in merged
    # trans pixels, of the second chromosome against the third
    assert 5 <= mu.ROW_TRANS < 75 and all(r and min(r) >= 75 for r in rows[mu.ROW_TRANS])
    # rows beyond the second tile boundary
    assert any(np.any((cool["bin1_id"] >= 2 * TILE_COLUMNS_ASSUMED) & (cool["bin1_id"] < n - 1)) for cool in src)
    # the merged table is not any single source
    assert want["count"].size > max(c["count"].size for c in src) or k == 1
    # the same from the same seed
    again = adversarial_sources(k)
    assert all(np.array_equal(x[key], y[key]) for x, y in zip(src, again) for key in ("bin1_id", "bin2_id", "count"))
