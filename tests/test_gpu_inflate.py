"""The pixel columns of a .cool decoded on the device: cs_inflate_chunks (engine.run_inflate_chunks) on the stream list of
tests/inflate_util.py, the finish pass (engine.run_table_from_columns) against numpy, and open_cool(decode="device") against
decode="host".  The judge is zlib.decompress plus numpy's transpose; every comparison is exact, byte for byte."""
import copy

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import engine, hdf5_lite, pipeline
from chromosight_amd._lib import get_device
from tests import inflate_util as iu
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

EXAMPLE = GOLDEN / "example.cool"
GUARD = 4096                        # elements behind a column that no store may reach
CASES = iu.stream_cases()


@pytest.fixture(scope="module")
def dev():
    return get_device()


def _dataset(cases, length=None):
    """One dataset made of the chunks of `cases` (all of one geometry): (file bytes, ChunkIndex, expected column)."""
    first = cases[0]
    assert all((c.elem_bytes, c.chunk_elems, c.filters) == (first.elem_bytes, first.chunk_elems, first.filters) for c in cases)
    pad = b"\x5a" * 13                                   # chunks do not touch in a file, nor are they aligned
    blob, offsets = bytearray(b"head"), []
    for c in cases:
        blob += pad
        offsets.append(len(blob))
        blob += c.stored
    blob += pad
    n = len(cases)
    length = n * first.chunk_elems if length is None else length
    index = hdf5_lite.ChunkIndex(first.values.dtype, length, first.chunk_elems, tuple((fid, ()) for fid in first.filters),
                                 np.asarray(offsets, dtype=np.int64), np.asarray([len(c.stored) for c in cases], dtype=np.int64),
                                 np.arange(n, dtype=np.int64) * first.chunk_elems, np.asarray([c.mask for c in cases], dtype=np.uint32))
    return bytes(blob), index, np.concatenate([c.values for c in cases])[:length]


def _guarded(dev, index, fill=0x5A):
    out = dev.empty(index.length + GUARD, index.dtype)
    out.upload(np.frombuffer(bytes([fill]) * out.nbytes, dtype=index.dtype))
    return out


def _decode(dev, cases, length=None):
    blob, index, want = _dataset(cases, length)
    out = _guarded(dev, index)
    _, status = engine.run_inflate_chunks(dev, blob, index, out=out)
    got = out.download()
    assert not status.any()
    assert got[:index.length].tobytes() == want.tobytes()
    assert got[index.length:].tobytes() == b"\x5a" * (GUARD * index.dtype.itemsize)       # nothing behind the column's end
    return got


def test_limit_is_reported():
    assert engine.inflate_max_chunk_bytes() >= 64 * 1024


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_each_stream_as_its_own_chunk(dev, case):
    _decode(dev, [case])


def test_all_streams_together(dev):
    """Every case of the list in one call per dataset geometry (a call decodes one dataset: one element size, chunk length and
    filter list), the cases of a geometry as its consecutive chunks."""
    groups = {}
    for c in CASES:
        groups.setdefault((c.elem_bytes, c.chunk_elems, c.filters), []).append(c)
    assert max(len(g) for g in groups.values()) >= 9
    for cases in groups.values():
        _decode(dev, cases)
    # ... and one dataset of more chunks than the device holds at once: a wave decodes several, one after the other
    ids = [c for c in CASES if c.chunk_elems == iu.N_IDS and c.elem_bytes == 8 and c.filters == (2, 1)]
    assert len(ids) * 250 > 8 * dev.cu_count
    _decode(dev, ids * 250)


def test_last_chunk_is_clipped_to_the_column(dev):
    """A dataset of 2 * 1899 + 700 elements: its last chunk is stored whole, and only 700 of its elements belong to the column."""
    ids = [c for c in CASES if c.name.startswith("ids level")][:3]
    length = 2 * iu.N_IDS + 700
    got = _decode(dev, ids, length=length)
    assert got.size == length + GUARD


def test_corrupt_chunks_among_valid_neighbours(dev):
    """One stream per failure the decoder names (each went through the sanitizer build first: tests/test_inflate_host.py), every one
    between valid chunks, in one call: the failed chunks carry their status and leave their elements alone, the valid ones are exact,
    and the call reports the failure."""
    good = [c for c in CASES if c.name.startswith("ids level")][:3]
    bad = iu.failure_streams()
    template = good[0]
    cases, want_status = [], []
    for k, (status, label, stream, cap) in enumerate(bad):
        assert cap == len(template.raw)
        cases += [good[k % 3], template._replace(name=label, stored=stream)]
        want_status += [0, status]
    # a chunk whose mask skips gzip and whose stored size is not a chunk's
    cases += [good[0], template._replace(name="unfiltered, short", stored=template.raw[:-8], mask=2), good[1]]
    want_status += [0, 10, 0]
    assert set(want_status) == set(range(11))
    blob, index, values = _dataset(cases)
    out = _guarded(dev, index)
    with pytest.raises(engine.CorruptChunks, match=f"{len(bad) + 1} of {len(cases)} chunks failed; the first is chunk 1 ") as err:
        engine.run_inflate_chunks(dev, blob, index, out=out)
    assert err.value.status.tolist() == want_status
    got = out.download()
    n = iu.N_IDS
    for k, status in enumerate(want_status):
        chunk = got[k * n:(k + 1) * n]
        if status == 0:
            assert chunk.tobytes() == values[k * n:(k + 1) * n].tobytes(), k
        else:
            assert chunk.tobytes() == b"\x5a" * (8 * n), cases[k].name
    assert got[index.length:].tobytes() == b"\x5a" * (8 * GUARD)


def test_bad_chunk_indexes_are_refused_before_any_launch(dev):
    blob, index, _ = _dataset([CASES[0], CASES[1]])
    out = _guarded(dev, index)
    with pytest.raises(ValueError, match="leaves the file"):
        engine.run_inflate_chunks(dev, blob, index._replace(nbytes=index.nbytes + len(blob)), out=out)
    with pytest.raises(ValueError, match="starts at element"):
        engine.run_inflate_chunks(dev, blob, index._replace(starts=index.starts + index.length), out=out)
    with pytest.raises(NotImplementedError, match="filter 32015"):
        engine.run_inflate_chunks(dev, blob, index._replace(filters=((2, ()), (32015, ()))), out=out)
    with pytest.raises(NotImplementedError, match="cs_inflate_max_chunk_bytes"):
        engine.run_inflate_chunks(dev, blob, index._replace(chunk=engine.inflate_max_chunk_bytes() // 8 + 1), out=out)
    assert out.download().tobytes() == b"\x5a" * out.nbytes


def test_scattered_chunks_are_gathered(dev):
    """Chunks far apart in the file (their span many times their sum) reach the device gathered; the column is the same."""
    a, b = CASES[0], CASES[1]
    blob = b"\0" * 7 + a.stored + b"\0" * 300_000 + b.stored
    index = hdf5_lite.ChunkIndex(a.values.dtype, 2 * iu.N_IDS, iu.N_IDS, ((2, ()), (1, ())), np.asarray([7, 7 + len(a.stored) + 300_000]),
                                 np.asarray([len(a.stored), len(b.stored)]), np.asarray([0, iu.N_IDS]), np.zeros(2, dtype=np.uint32))
    column, status = engine.run_inflate_chunks(dev, blob, index)
    assert not status.any() and column.download().tobytes() == a.values.tobytes() + b.values.tobytes()


# ---- the finish pass ----------------------------------------------------------------------------------------------------------------
def _finish(dev, b1, b2, cnt, n_bins):
    res = engine.run_table_from_columns(dev, dev.to_device(b1), dev.to_device(b2), dev.to_device(cnt), b1.size, n_bins)
    assert res["nnz"] == b1.size
    return res


def _assert_finish_is_the_constructor(dev, b1, b2, cnt, n_bins):
    res = _finish(dev, b1, b2, cnt, n_bins)
    assert res["ids_ok"] and res["sorted"]
    assert res["upper"] == bool(np.all(b2 >= b1))
    assert (res["count_min"], res["count_max"]) == (int(cnt.min()), int(cnt.max()))
    want_dtype = np.float32 if cnt.max() < (1 << 24) else np.float64
    assert res["val_dtype"] is want_dtype
    n = b1.size
    assert res["indptr"].download().tobytes() == np.searchsorted(b1, np.arange(n_bins + 1)).astype(np.int64).tobytes()
    assert res["indices"].download()[:n].tobytes() == b2.astype(np.int32).tobytes()
    data = res["data"].download()
    assert data.dtype == want_dtype and data[:n].tobytes() == cnt.astype(want_dtype).tobytes()
    return res


def _sorted_table(rng, n, n_bins, id_dtype, count_dtype, upper=True, rows=None):
    lo, hi = rows or (0, n_bins)
    r = rng.integers(lo, hi, 3 * n)
    c = rng.integers(0, n_bins, 3 * n)
    if upper:
        r, c = np.minimum(r, c), np.maximum(r, c)
        keep = (r >= lo) & (r < hi)
        r, c = r[keep], c[keep]
    key = np.unique(r.astype(np.int64) * n_bins + c)
    if key.size > n:
        key = np.sort(rng.choice(key, n, replace=False))
    return (key // n_bins).astype(id_dtype), (key % n_bins).astype(id_dtype), rng.integers(1, 500, key.size).astype(count_dtype)


@pytest.mark.parametrize("id_dtype, count_dtype", [(np.int64, np.int32), (np.int32, np.int32), (np.int64, np.int64), (np.int32, np.int64)])
def test_finish_pass_is_what_the_constructor_uploads(dev, id_dtype, count_dtype):
    rng = np.random.default_rng(11)
    # more than one workgroup's share per thread (8 workgroups a CU), rows without pixels at either end and in the middle
    b1, b2, cnt = _sorted_table(rng, 700_001, 5000, id_dtype, count_dtype, rows=(37, 4800))
    keep = (b1 < 2000) | (b1 >= 2010)
    b1, b2, cnt = b1[keep], b2[keep], cnt[keep]
    assert b1.size > 8 * 256 * dev.cu_count and b1[0] >= 37 and b1[-1] < 4800
    _assert_finish_is_the_constructor(dev, b1, b2, cnt, 5000)


def test_finish_pass_reports_dtype_sign_triangle_and_order(dev):
    rng = np.random.default_rng(12)
    b1, b2, cnt = _sorted_table(rng, 3001, 300, np.int64, np.int64)
    big = cnt.copy()
    big[1234] = 1 << 24
    assert _assert_finish_is_the_constructor(dev, b1, b2, big, 300)["val_dtype"] is np.float64
    big[1234] = (1 << 24) - 1
    assert _assert_finish_is_the_constructor(dev, b1, b2, big, 300)["val_dtype"] is np.float32
    big[77] = -5
    assert _assert_finish_is_the_constructor(dev, b1, b2, big, 300)["count_min"] == -5
    huge = cnt.copy()
    huge[5] = (1 << 53) + 1                              # not a float64: rounds as numpy rounds it
    _assert_finish_is_the_constructor(dev, b1, b2, huge, 300)
    lo1, lo2, lo_cnt = _sorted_table(rng, 3001, 300, np.int32, np.int32, upper=False)
    assert not _assert_finish_is_the_constructor(dev, lo1, lo2, lo_cnt, 300)["upper"]
    # two pixels in each other's place, one pixel twice, ids outside the bins
    swap1, swap2 = b1.copy(), b2.copy()
    swap1[[100, 101]], swap2[[100, 101]] = b1[[101, 100]], b2[[101, 100]]
    res = _finish(dev, swap1, swap2, cnt, 300)
    assert res["ids_ok"] and not res["sorted"] and res["data"] is None
    twice1, twice2 = b1.copy(), b2.copy()
    twice1[501], twice2[501] = twice1[500], twice2[500]
    assert not _finish(dev, twice1, twice2, cnt, 300)["sorted"]
    for column, value in ((0, -1), (0, 300), (1, 300), (1, -7)):
        ids = [b1.copy(), b2.copy()]
        ids[column][2000] = value
        assert not _finish(dev, ids[0], ids[1], cnt, 300)["ids_ok"]
    empty = np.zeros(0, dtype=np.int64)
    res = _finish(dev, empty, empty, empty, 300)
    assert res["ids_ok"] and res["sorted"] and res["upper"] and res["val_dtype"] is np.float32
    assert not res["indptr"].download().any()


# ---- open_cool ----------------------------------------------------------------------------------------------------------------------
def _table(dcool):
    n = dcool.nnz
    return (dcool.indptr.download(), dcool.indices.download()[:n].copy(), dcool.data.download().view(dcool.val_dtype)[:n].copy())


def _assert_same_cool(got, want):
    assert got.nnz == want.nnz and got.n_bins == want.n_bins and got.binsize == want.binsize and got.names == want.names
    assert np.dtype(got.val_dtype) == np.dtype(want.val_dtype) and got.upper == want.upper and got.counts_ok == want.counts_ok
    assert got._counts_exact == want._counts_exact
    for a, b in zip(_table(got), _table(want)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.array_equal(got.offsets, want.offsets)
    assert got.weight.download().tobytes() == want.weight.download().tobytes()
    assert got.miss.download().tobytes() == want.miss.download().tobytes()
    hg, hw = got.host, want.host
    assert set(hg) == set(hw)
    for key in hw:
        a, b = np.asarray(hg[key]), np.asarray(hw[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def _assert_same_detect(got, want, config):
    """detect is not bitwise repeatable in score / pvalue / qvalue even on one table (tests/test_gpu_cload.py: up to 3.9e-15 between
    calls), so those three are held to the 2e-10 of tests/test_gpu_pipeline.py and every other column to equality."""
    a = pipeline.detect(got, copy.deepcopy(config))
    b = pipeline.detect(want, copy.deepcopy(config))
    assert len(b) > 0 and list(a.columns) == list(b.columns)
    floats = ["score", "pvalue", "qvalue"]
    pd.testing.assert_frame_equal(a.drop(columns=floats), b.drop(columns=floats), check_exact=True)
    for col in floats:
        diff = float(np.abs(a[col].to_numpy() - b[col].to_numpy()).max())
        print(f"{col}: largest difference {diff:.3g}")
        assert diff <= 2e-10, col


@pytest.mark.parametrize("options", [{}, {"resolution": "twice"}, {"norm": "force"}], ids=["as stored", "coarsened", "norm=force"])
def test_open_cool_on_the_device_is_open_cool_on_the_host(dev, options):
    options = dict(options)
    if options.get("resolution") == "twice":
        with hdf5_lite.File(EXAMPLE) as f:
            options["resolution"] = 2 * int(f.attrs("/")["bin-size"])
    got = pipeline.open_cool(str(EXAMPLE), decode="device", **options)
    want = pipeline.open_cool(str(EXAMPLE), decode="host", **options)
    if not options:
        assert got._host is None                          # the device route downloads nothing until .host is read
    _assert_same_cool(got, want)
    _assert_same_detect(got, want, ck.loops)
    _assert_same_detect(got, want, ck.borders)


def test_from_cool_file_and_auto(dev, monkeypatch):
    want = pipeline.DeviceCool(str(EXAMPLE))
    got = pipeline.DeviceCool.from_cool_file(str(EXAMPLE))
    assert got._host is None
    _assert_same_cool(got, want)
    auto = pipeline.open_cool(str(EXAMPLE))
    assert (auto._host is None) == pipeline.AUTO_DECODE_ON_DEVICE
    _assert_same_cool(auto, want)
    monkeypatch.setenv("CHROMOSIGHT_HIP_HOST_DECODE", "1")
    assert pipeline.open_cool(str(EXAMPLE))._host is not None
    monkeypatch.delenv("CHROMOSIGHT_HIP_HOST_DECODE")
    merged = pipeline.open_cool([str(EXAMPLE), str(EXAMPLE)], decode="device")
    _assert_same_cool(merged, pipeline.open_cool([str(EXAMPLE), str(EXAMPLE)], decode="host"))


def test_device_route_refuses_what_does_not_qualify(dev, golden, monkeypatch):
    cool = dict(golden("example_cool"))
    order = np.random.default_rng(3).permutation(cool["bin1_id"].size)
    unsorted = dict(cool, bin1_id=cool["bin1_id"][order], bin2_id=cool["bin2_id"][order], count=cool["count"][order])
    with pytest.raises(ValueError, match="dictionary"):
        pipeline.open_cool(unsorted, decode="device")
    assert pipeline.open_cool(unsorted).nnz == cool["bin1_id"].size           # "auto": the host route sorts it, as before
    # an oversized chunk: the file's own chunks against a limit below them
    monkeypatch.setattr(engine, "inflate_max_chunk_bytes", lambda: 4096)
    with pytest.raises(pipeline.DeviceDecodeRefused, match="chunks of"):
        pipeline.open_cool(str(EXAMPLE), decode="device")
    assert pipeline.open_cool(str(EXAMPLE), decode="auto")._host is not None   # ... and "auto" goes to the host
