"""Coarsening on the host side (no GPU): the numpy oracle of tests/coarsen_util.py against an independent dense formulation, and
chromosight_amd.coarsen.coarse_geometry on hand cases."""
import numpy as np
import pytest

from chromosight_amd.coarsen import coarse_geometry
from tests.coarsen_util import coarse_bins, oracle_coarsen, oracle_geometry


def _random_cool(rng, sizes, density, binsize=1000, upper=True):
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    dense = rng.integers(1, 50, size=(n, n)) * (rng.random((n, n)) < density)
    if upper:
        dense = np.triu(dense)
    b1, b2 = np.nonzero(dense)
    return {"binsize": binsize, "chrom_offset": off, "chrom_names": np.array([f"c{i}" for i in range(sizes.size)]),
            "bin1_id": b1, "bin2_id": b2, "count": dense[b1, b2], "weight": None, "bin_start": None, "bin_end": None}, dense


def _dense_block_sums(dense, off, factor):
    """Every chromosome pair on its own: the sums of the factor x factor blocks of the dense matrix (short last blocks included)."""
    edges = np.concatenate([np.arange(off[c], off[c + 1], factor) for c in range(off.size - 1)] + [[off[-1]]]).astype(np.int64)
    out = np.zeros((edges.size - 1, edges.size - 1), dtype=np.int64)
    for i in range(edges.size - 1):
        for j in range(edges.size - 1):
            out[i, j] = dense[edges[i]:edges[i + 1], edges[j]:edges[j + 1]].sum()
    return out


@pytest.mark.parametrize("upper", [True, False])
@pytest.mark.parametrize("factor", [1, 2, 3, 4, 7, 50])
@pytest.mark.parametrize("sizes", [[7], [1, 5, 4, 1, 9], [6, 6, 6], [2, 11, 3]])
def test_oracle_equals_the_dense_block_sums(sizes, factor, upper):
    rng = np.random.default_rng(len(sizes) * 100 + factor)
    cool, dense = _random_cool(rng, sizes, 0.4, upper=upper)
    got = oracle_coarsen(cool, factor)
    want = _dense_block_sums(dense, cool["chrom_offset"], factor)
    assert int(got["chrom_offset"][-1]) == want.shape[0]
    assert np.array_equal(np.diff(got["chrom_offset"]), -(-np.asarray(sizes) // factor))
    b1, b2, cnt = got["bin1_id"], got["bin2_id"], got["count"]
    assert cnt.dtype == np.int64 and np.all(cnt > 0)
    key = b1 * want.shape[0] + b2
    assert np.all(np.diff(key) > 0), "sorted by (bin1, bin2), no duplicates"
    back = np.zeros_like(want)
    back[b1, b2] = cnt
    assert np.array_equal(back, want)
    if upper:
        assert np.all(b2 >= b1)
    assert got["weight"] is None and got["binsize"] == 1000 * factor


def test_coarse_bins_on_a_hand_case():
    cmap, off = coarse_bins([0, 5, 6, 10], 2)
    assert cmap.tolist() == [0, 0, 1, 1, 2, 3, 4, 4, 5, 5]
    assert off.tolist() == [0, 3, 4, 6]


def _geometry(offsets, binsize, bin_end, factor):
    off, start, end, bs = coarse_geometry(np.asarray(offsets), binsize, bin_end, factor)
    return np.asarray(off).tolist(), np.asarray(start).tolist(), np.asarray(end).tolist(), int(bs)


def test_geometry_of_multiples_and_non_multiples():
    # 6 bins (a multiple of 3) and 7 bins (not), ragged chromosome ends
    bin_end = [1000, 2000, 3000, 4000, 5000, 5500] + [1000, 2000, 3000, 4000, 5000, 6000, 6001]
    off, start, end, bs = _geometry([0, 6, 13], 1000, np.asarray(bin_end), 3)
    assert off == [0, 2, 5]
    assert start == [0, 3000, 0, 3000, 6000]
    assert end == [3000, 5500, 3000, 6000, 6001]
    assert bs == 3000


def test_geometry_of_a_one_bin_chromosome_and_a_factor_larger_than_a_chromosome():
    bin_end = [700] + [2000, 4000, 4100] + [2000, 4000, 6000, 8000, 10000, 12000, 14000, 16000, 17000]
    off, start, end, bs = _geometry([0, 1, 4, 13], 2000, np.asarray(bin_end), 5)
    assert off == [0, 1, 2, 4]
    assert start == [0, 0, 0, 10000]
    assert end == [700, 4100, 10000, 17000]
    assert bs == 10000


def test_geometry_of_factor_one_is_the_parents():
    bin_end = np.asarray([1000, 2000, 2500, 1000, 1800])
    off, start, end, bs = _geometry([0, 3, 5], 1000, bin_end, 1)
    assert off == [0, 3, 5]
    assert start == [0, 1000, 2000, 0, 1000]
    assert end == bin_end.tolist()
    assert bs == 1000


def test_geometry_of_a_parent_without_bin_end():
    off, start, end, bs = _geometry([0, 5, 7], 2000, None, 2)
    assert off == [0, 3, 4]
    assert start == [0, 4000, 8000, 0]
    assert end == [4000, 8000, 10000, 4000]      # the chromosome's length is n_c * binsize
    assert bs == 4000


@pytest.mark.parametrize("factor", [1, 2, 3, 5, 7, 64])
def test_geometry_equals_the_oracles_on_the_yeast_bins(golden, factor):
    cool = golden("yeast_cool")
    got = coarse_geometry(cool["chrom_offset"], int(cool["binsize"]), cool["bin_end"], factor)
    want = oracle_geometry(cool["chrom_offset"], int(cool["binsize"]), cool["bin_end"], factor)
    for g, w in zip(got[:3], want[:3]):
        assert np.array_equal(np.asarray(g), w)
    assert got[3] == want[3]


@pytest.mark.parametrize("factor", [0, -1, 2.5])
def test_geometry_refuses_a_bad_factor(factor):
    with pytest.raises(ValueError):
        coarse_geometry(np.asarray([0, 4]), 1000, None, factor)
