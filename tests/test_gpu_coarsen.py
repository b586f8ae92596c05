"""Coarsening of a resident pixel table on the device (cs_coarsen, chromosight_amd/coarsen.py, DeviceCool.coarsened,
pipeline.open_cool(resolution=)) against the numpy oracle of tests/coarsen_util.py.  The counts are integers and every sum is exact,
so equality is exact throughout: row pointers, column bins, counts and the dtype of the counts."""
import copy
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import coarsen as cco
from chromosight_amd import pipeline
from chromosight_amd._lib import CsCsr, Device, np_dtype_code
from tests.coarsen_util import block_totals, csr_of, oracle_coarsen

pytestmark = pytest.mark.gpu

YEAST_FACTORS = [1, 2, 3, 5, 7, 64]


def _cis_only(cool):
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))
    keep = chrom[cool["bin1_id"]] == chrom[cool["bin2_id"]]
    out = dict(cool)
    for k in ("bin1_id", "bin2_id", "count"):
        out[k] = np.asarray(cool[k])[keep]
    return out


@pytest.fixture(scope="module")
def yeast(golden):
    """{trans: (decoded cool, DeviceCool)} of the yeast fixture, with and without its trans pixels."""
    full = golden("yeast_cool")
    cis = _cis_only(full)
    return {True: (full, pipeline.DeviceCool(full)), False: (cis, pipeline.DeviceCool(cis))}


@pytest.fixture(scope="module")
def yeast_oracle(yeast):
    cache = {}

    def get(trans, factor):
        if (trans, factor) not in cache:
            cache[trans, factor] = oracle_coarsen(yeast[trans][0], factor)
        return cache[trans, factor]

    return get


def _download(res):
    n = res["nnz"]
    return (res["indptr"].download(), res["indices"].download()[:n].copy(),
            res["data"].download().view(res["val_dtype"])[:n].copy())


def _assert_equals_oracle(res, want):
    indptr, indices, cnt, dtype = csr_of(want)
    got_indptr, got_indices, got_data = _download(res)
    assert res["nnz"] == cnt.size
    assert np.dtype(res["val_dtype"]) == np.dtype(dtype)
    assert np.array_equal(got_indptr, indptr)
    assert np.array_equal(got_indices, indices)
    assert got_data.dtype == np.dtype(dtype) and np.array_equal(got_data, cnt.astype(dtype))
    assert np.array_equal(res["offsets"], want["chrom_offset"])
    assert np.array_equal(res["bin_start"], want["bin_start"]) and np.array_equal(res["bin_end"], want["bin_end"])
    assert res["binsize"] == want["binsize"]


def _make_cool(sizes, b1, b2, cnt, binsize=1000):
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    b1, b2, cnt = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64), np.asarray(cnt)
    key, first = np.unique(b1 * int(off[-1]) + b2, return_index=True)      # sorted by (bin1, bin2), duplicates dropped
    return {"binsize": binsize, "chrom_offset": off, "chrom_names": np.array([f"c{i}" for i in range(sizes.size)]),
            "bin1_id": b1[first], "bin2_id": b2[first], "count": cnt[first], "weight": None, "bin_start": None, "bin_end": None}


def _random_upper(rng, n, pixels):
    a, b = rng.integers(0, n, size=pixels), rng.integers(0, n, size=pixels)
    return np.minimum(a, b), np.maximum(a, b)


# ---- the yeast fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("factor", YEAST_FACTORS)
def test_yeast_equals_the_oracle(yeast, yeast_oracle, factor, trans):
    cool, dc = yeast[trans]
    assert dc.n_chrom == 17 and dc.upper
    assert dc.nnz > (2_000_000 if trans else 300_000)
    want = yeast_oracle(trans, factor)
    _assert_equals_oracle(cco.coarsen_csr(dc, factor), want)
    co = dc.coarsened(factor)
    assert co.n_bins == int(want["chrom_offset"][-1]) and co.binsize == int(cool["binsize"]) * factor
    assert co.names == dc.names and co.nnz == want["count"].size
    assert co.upper is True
    host = co.host
    assert np.all(host["bin2_id"] >= host["bin1_id"])
    assert np.array_equal(block_totals(host), block_totals(cool))
    if factor == 1:
        assert co.has_weights and np.array_equal(co.host_weight, dc.host_weight, equal_nan=True)
        assert np.array_equal(host["bin1_id"], cool["bin1_id"]) and np.array_equal(host["bin2_id"], cool["bin2_id"])
        assert np.array_equal(host["count"], cool["count"])
        assert np.array_equal(co.bin_end, cool["bin_end"])
    else:
        assert not co.has_weights and co.host_weight is None


# ---- synthetic edges --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 5])
def test_many_chromosomes_of_one_to_factor_plus_one_bins(factor):
    rng = np.random.default_rng(factor)
    sizes = [1 + i % (factor + 1) for i in range(90)]
    n = sum(sizes)
    b1, b2 = _random_upper(rng, n, 20 * n)
    cool = _make_cool(sizes, b1, b2, rng.integers(1, 100, size=b1.size))
    _assert_equals_oracle(cco.coarsen_csr(pipeline.DeviceCool(cool), factor), oracle_coarsen(cool, factor))


def test_coarse_rows_whose_fine_rows_are_all_empty():
    rng = np.random.default_rng(1)
    sizes = [403, 97, 250]
    n = sum(sizes)
    rows = np.concatenate([np.arange(0, 20), np.arange(300, 310), np.arange(520, 523), [n - 1]])      # every other row is empty
    b1 = rng.choice(rows, size=4000)
    b2 = rng.integers(0, n, size=4000)
    b1, b2 = np.minimum(b1, b2), np.maximum(b1, b2)
    keep = np.isin(b1, rows)
    cool = _make_cool(sizes, b1[keep], b2[keep], rng.integers(1, 9, size=int(keep.sum())))
    for factor in (4, 9):
        want = oracle_coarsen(cool, factor)
        assert np.any(np.diff(csr_of(want)[0]) == 0)
        _assert_equals_oracle(cco.coarsen_csr(pipeline.DeviceCool(cool), factor), want)


def test_empty_table():
    cool = _make_cool([10, 7], [], [], np.zeros(0, dtype=np.int32))
    res = cco.coarsen_csr(pipeline.DeviceCool(cool), 3)
    assert res["nnz"] == 0 and np.dtype(res["val_dtype"]) == np.float32
    assert np.array_equal(res["indptr"].download(), np.zeros(4 + 3 + 1, dtype=np.int64))
    co = pipeline.DeviceCool(cool).coarsened(3)
    assert co.nnz == 0 and co.n_bins == 7 and co.offsets.tolist() == [0, 4, 7]


@pytest.mark.parametrize("factor", [5, 300])
def test_one_heavy_row_among_sparse_ones(factor):
    """One fine row of 200 000 pixels (the workgroup-wide walk of a single range, over a hundred column tiles); factor 300 puts
    more fine rows under a coarse row than a workgroup has threads."""
    rng = np.random.default_rng(7)
    n, heavy = 260_000, 1234
    cols = heavy + rng.choice(n - heavy, size=200_000, replace=False)
    sb1, sb2 = _random_upper(rng, n, 60_000)
    b1 = np.concatenate([np.full(cols.size, heavy), sb1])
    b2 = np.concatenate([cols, sb2])
    cool = _make_cool([n - 10_000, 10_000], b1, b2, rng.integers(1, 1000, size=b1.size))
    assert np.count_nonzero(cool["bin1_id"] == heavy) >= 200_000
    _assert_equals_oracle(cco.coarsen_csr(pipeline.DeviceCool(cool), factor), oracle_coarsen(cool, factor))


def test_sums_that_cross_2_to_24_come_out_as_float64():
    rng = np.random.default_rng(3)
    n = 600
    b1, b2 = _random_upper(rng, n, 30_000)
    cnt = rng.integers(1, 50, size=b1.size)
    cnt[::7] = (1 << 24) - 1                            # exact in float32; two of them in one coarse pixel are not
    cool = _make_cool([350, 250], b1, b2, cnt)
    dc = pipeline.DeviceCool(cool)
    assert dc.val_dtype is np.float32
    want = oracle_coarsen(cool, 4)
    assert want["count"].max() >= 1 << 25
    res = cco.coarsen_csr(dc, 4)
    assert np.dtype(res["val_dtype"]) == np.float64
    _assert_equals_oracle(res, want)


def test_float64_integer_counts_in():
    rng = np.random.default_rng(4)
    n = 500
    b1, b2 = _random_upper(rng, n, 20_000)
    cnt = rng.integers(1, 1 << 36, size=b1.size).astype(np.float64)
    cool = _make_cool([123, 377], b1, b2, cnt)
    dc = pipeline.DeviceCool(cool)
    assert dc.val_dtype is np.float64
    for factor in (3, 600):                             # 600: every chromosome pair becomes one pixel
        _assert_equals_oracle(cco.coarsen_csr(dc, factor), oracle_coarsen(cool, factor))


@pytest.fixture(scope="module")
def wide_cool():
    """40 000 bins, more than 3 M pixels over the whole width: a dense band next to scattered pixels."""
    rng = np.random.default_rng(11)
    sizes = [17_001, 2_999, 20_000]
    n = sum(sizes)
    sb1, sb2 = _random_upper(rng, n, 2_000_000)
    r = rng.integers(0, n, size=1_500_000)
    d = rng.integers(0, 60, size=r.size)
    b1 = np.concatenate([sb1, r])
    b2 = np.concatenate([sb2, np.minimum(r + d, n - 1)])
    cool = _make_cool(sizes, b1, b2, rng.integers(1, 30, size=b1.size).astype(np.int32))
    return cool, pipeline.DeviceCool(cool)


@pytest.mark.parametrize("factor", [2, 5])
def test_a_few_million_pixels_across_tiles_and_grid_strides(wide_cool, factor):
    """More coarse rows than the launch has workgroups (grid stride), rows that span several column tiles."""
    cool, dc = wide_cool
    assert cool["count"].size > 3_000_000
    _assert_equals_oracle(cco.coarsen_csr(dc, factor), oracle_coarsen(cool, factor))


def test_a_table_that_is_not_upper_triangle_stays_as_it_is_stored():
    rng = np.random.default_rng(5)
    n = 900
    b1, b2 = rng.integers(0, n, size=50_000), rng.integers(0, n, size=50_000)
    cool = _make_cool([400, 500], b1, b2, rng.integers(1, 9, size=b1.size))
    dc = pipeline.DeviceCool(cool)
    assert not dc.upper
    _assert_equals_oracle(cco.coarsen_csr(dc, 6), oracle_coarsen(cool, 6))
    assert not dc.coarsened(6).upper


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _small_cool(counts=None):
    rng = np.random.default_rng(2)
    b1, b2 = _random_upper(rng, 300, 5000)
    cool = _make_cool([100, 200], b1, b2, rng.integers(1, 9, size=b1.size).astype(np.float64))
    if counts is not None:
        cool["count"] = counts(cool["count"].copy())
    return cool


@pytest.mark.parametrize("factor", [0, -1])
def test_a_factor_below_one_is_refused(factor):
    dc = pipeline.DeviceCool(_small_cool())
    with pytest.raises(ValueError):
        cco.coarsen_csr(dc, factor)
    with pytest.raises(ValueError):
        dc.coarsened(factor)
    # ... and by the C entry itself (CS_ERR_INVALID)
    dev = dc.dev
    indptr, indices, data = dev.empty(dc.n_bins + 1, np.int64), dev.empty(dc.nnz, np.int32), dev.empty(dc.nnz, np.float64)
    out = CsCsr(0, 0, 0, indptr.ptr, indices.ptr, data.ptr, np_dtype_code(np.float32), 0, None, None, None)
    genome, out_nnz = dc.csr(), C.c_int64(0)
    off = np.ascontiguousarray(dc.offsets, dtype=np.int64)
    with dev.lock:
        rc = dev.lib.cs_coarsen(dev.ctx, None, C.byref(genome), off.ctypes.data_as(C.POINTER(C.c_int64)), dc.n_chrom, factor,
                                C.byref(out), C.byref(out_nnz))
    assert rc == -1
    with pytest.raises(ValueError):
        dev._check(rc)


def _set(at, value):
    def change(cnt):
        cnt[at] = value
        return cnt
    return change


@pytest.mark.parametrize("value", [2.5, np.nan, -1.0, np.inf], ids=["fractional", "nan", "negative", "inf"])
def test_a_count_that_is_not_a_non_negative_integer_is_refused(value):
    dc = pipeline.DeviceCool(_small_cool(_set(1234, value)))
    with pytest.raises(ValueError):
        cco.coarsen_csr(dc, 2)
    with pytest.raises(ValueError):
        dc.coarsened(1)


def test_a_total_of_2_to_53_is_refused():
    def big(cnt):
        cnt[:] = 1.0
        cnt[:1024] = float(1 << 43)
        return cnt
    with pytest.raises(ValueError):
        cco.coarsen_csr(pipeline.DeviceCool(_small_cool(big)), 2)

    def below(cnt):
        cnt[:] = 0.0
        cnt[:1023] = float(1 << 43)
        return cnt
    cool = _small_cool(below)
    _assert_equals_oracle(cco.coarsen_csr(pipeline.DeviceCool(cool), 2), oracle_coarsen(cool, 2))


@pytest.mark.parametrize("resolution", [3000, 1000, 0, -2000])
def test_open_cool_refuses_a_resolution_that_is_no_multiple_of_the_bin_size(golden, resolution):
    with pytest.raises(ValueError, match="2000"):
        pipeline.open_cool(golden("yeast_cool"), resolution=resolution)


# ---- reproducibility --------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_second_context_give_the_same_bits(yeast):
    cool, dc = yeast[True]
    first = _download(cco.coarsen_csr(dc, 5))
    again = _download(cco.coarsen_csr(dc, 5))
    other = _download(cco.coarsen_csr(pipeline.DeviceCool(cool, Device(0)), 5))
    for a, b, c in zip(first, again, other):
        assert a.dtype == b.dtype == c.dtype
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _same_tables(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for col in a.columns:
        x, y = a[col].to_numpy(), b[col].to_numpy()
        if col in ("score", "pvalue", "qvalue"):
            assert np.allclose(x.astype(float), y.astype(float), rtol=1e-9, atol=1e-12, equal_nan=True), col
        else:
            assert np.array_equal(x, y), col


@pytest.mark.parametrize("norm", ["auto", "raw"])
def test_open_cool_at_10_kb_equals_an_upload_of_the_coarse_table(golden, yeast_oracle, norm):
    cool = golden("yeast_cool")
    got = pipeline.open_cool(cool, resolution=10000, norm=norm)
    want = pipeline.open_cool(yeast_oracle(True, 5), norm=norm)
    assert got.binsize == want.binsize == 10000 and got.n_bins == want.n_bins and got.nnz == want.nnz
    assert np.array_equal(got.offsets, want.offsets)
    assert np.array_equal(got.bin_start, want.bin_start) and np.array_equal(got.bin_end, want.bin_end)
    w_got, w_want = got.host_weight, want.host_weight
    assert w_got.dtype == np.float64 and w_got.tobytes() == w_want.tobytes()
    assert np.isfinite(w_got).sum() > w_got.size // 2
    if norm == "raw":
        assert set(np.unique(w_got[np.isfinite(w_got)])) == {1.0}
    # the file's own bin size: the stored weights, as without the argument
    same = pipeline.open_cool(cool, resolution=2000, norm=norm)
    plain = pipeline.open_cool(cool, norm=norm)
    assert same.binsize == 2000 and same.host_weight.tobytes() == plain.host_weight.tobytes()
    # hairpins are defined at 10 kb
    hairpins = dict(copy.deepcopy(ck.hairpins), max_perc_zero=100.0)
    assert hairpins["resolution"] == got.binsize
    tab_got = pipeline.detect(got, hairpins)
    tab_want = pipeline.detect(want, hairpins)
    _same_tables(tab_got, tab_want)
    assert len(tab_got) > 0
    names, sizes = got.names, np.diff(got.offsets)
    rows = []
    for ci in (0, 3, 10):
        for i in range(10, int(sizes[ci]) - 10, 7):
            rows.append((names[ci], i * 10000, (i + 1) * 10000, names[ci], (i + 2) * 10000, (i + 3) * 10000))
    positions = pd.DataFrame(rows, columns=["chrom1", "start1", "end1", "chrom2", "start2", "end2"])
    q_got, w_q_got = pipeline.quantify(got, positions, hairpins)
    q_want, w_q_want = pipeline.quantify(want, positions, hairpins)
    _same_tables(q_got, q_want)
    assert np.isfinite(q_got.score.to_numpy(dtype=float)).sum() > 0
    assert np.allclose(w_q_got, w_q_want, rtol=0, atol=1e-12, equal_nan=True)
