"""The host side of the binning of read pairs (chromosight_amd/cload.py, io.read_pairs) and the tools of its device tests
(tests/cload_util.py): the geometry's edge cases, the oracle against a dense per-pair loop, the round trip table -> pairs -> table,
the .pairs reader and the refusals of check_chunk.  No GPU."""
import gzip

import numpy as np
import pytest

from chromosight_amd import cload
from chromosight_amd import io as cio
from tests import cload_util as cu
from tests.cload_util import oracle_cload, pairs_of_table


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def test_geometry_edge_cases():
    sizes = [("one", 1000), ("multiple", 3000), ("over", 3001), ("short", 7)]
    geo = cload.bin_geometry(sizes, 1000)
    assert geo.offsets.tolist() == [0, 1, 4, 8, 9] and geo.names == ["one", "multiple", "over", "short"] and geo.binsize == 1000
    assert geo.bin_start.tolist() == [0, 0, 1000, 2000, 0, 1000, 2000, 3000, 0]
    assert geo.bin_end.tolist() == [1000, 1000, 2000, 3000, 1000, 2000, 3000, 3001, 7]
    assert geo.lengths.tolist() == [1000, 3000, 3001, 7]
    names, lengths, offsets, start, end = cu.geometry(sizes, 1000)
    assert np.array_equal(offsets, geo.offsets) and np.array_equal(start, geo.bin_start) and np.array_equal(end, geo.bin_end)
    assert cload.bin_geometry(dict(sizes), 1000).offsets.tolist() == [0, 1, 4, 8, 9]
    assert cload.bin_geometry(sizes, 1).offsets[-1] == 1000 + 3000 + 3001 + 7
    toy = cload.bin_geometry(cu.TOY, cu.BINSIZE)
    assert int(toy.offsets[-1]) == cu.TOY_BINS and np.diff(toy.offsets).tolist() == [101, 1, 155]


@pytest.mark.parametrize("sizes,binsize", [([("a", 0)], 10), ([("a", 5)], 0), ([("a", 5)], 2.5), ([("a", 5), ("a", 6)], 2),
                                           ([("a", 2 ** 40)], 1), ([("a", 5)], True)])
def test_geometry_refusals(sizes, binsize):
    with pytest.raises(ValueError):
        cload.bin_geometry(sizes, binsize)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_oracle_equals_a_dense_per_pair_loop():
    sizes, binsize = [("x", 130), ("y", 7), ("z", 250)], 10                      # 13 + 1 + 25 = 39 bins ... and one more
    sizes.append(("w", 10))                                                      # 40 bins
    names, lengths, offsets, _, _ = cu.geometry(sizes, binsize)
    n = int(offsets[-1])
    assert n == 40
    rng = np.random.default_rng(3)
    m = 5000
    c1, c2 = rng.integers(-1, 4, size=m), rng.integers(-1, 4, size=m)
    p1 = np.array([rng.integers(1, lengths[max(c, 0)] + 1) for c in c1])
    p2 = np.array([rng.integers(1, lengths[max(c, 0)] + 1) for c in c2])
    dense = np.zeros((n, n), dtype=np.int64)
    dropped = 0
    for a, x, b, y in zip(c1.tolist(), p1.tolist(), c2.tolist(), p2.tolist()):
        if a == -1 or b == -1:
            dropped += 1
            continue
        i, j = offsets[a] + (x - 1) // binsize, offsets[b] + (y - 1) // binsize
        dense[min(i, j), max(i, j)] += 1
    got = oracle_cload(sizes, binsize, c1, p1, c2, p2)
    assert got["dropped"] == dropped > 0
    rows, cols = np.nonzero(dense)
    assert np.array_equal(got["bin1_id"], rows) and np.array_equal(got["bin2_id"], cols) and np.array_equal(got["count"], dense[rows, cols])
    assert got["val_dtype"] is np.float32 and got["weight"] is None and np.all(got["bin2_id"] >= got["bin1_id"])
    zero = oracle_cload(sizes, binsize, c1, p1 - 1, c2, p2 - 1, zero_based=True)
    assert all(np.array_equal(got[k], zero[k]) for k in ("bin1_id", "bin2_id", "count"))


@pytest.mark.parametrize("c,p,zero_based", [(0, 0, False), (0, 131, False), (0, 130, True), (0, -4, True), (4, 1, False), (-2, 1, False),
                                            (1, 8, False), (0, np.iinfo(np.int64).min, False)])
def test_oracle_refusals(c, p, zero_based):
    sizes = [("x", 130), ("y", 7), ("z", 250), ("w", 10)]
    c1, p1 = np.array([0, 0, c, 0, c]), np.array([5, 5, p, 5, p])
    for cols in ((c1, p1, np.zeros(5, dtype=np.int64), np.full(5, 5)), (np.zeros(5, dtype=np.int64), np.full(5, 5), c1, p1)):
        with pytest.raises(ValueError, match="2 of 5 pairs refused; the first is pair 2 "):
            oracle_cload(sizes, 10, *cols, zero_based=zero_based)
    # refusing comes before dropping
    with pytest.raises(ValueError, match="1 of 1 pairs refused"):
        oracle_cload(sizes, 10, [-1], [1], [c], [p], zero_based=zero_based)


def _same_table(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("bin1_id", "bin2_id", "count", "chrom_offset"))


def test_round_trip_on_the_example_fixture(golden):
    cool = golden("example_cool")
    assert int(cool["chrom_offset"][-1]) == 720 and int(cool["count"].sum()) == 3_299_038
    pairs = pairs_of_table(cool, seed=1)
    assert pairs[0].size == 3_299_038 and pairs[0].dtype == np.int32 and pairs[1].dtype == np.int64
    below = (pairs[0] > pairs[2]) | ((pairs[0] == pairs[2]) & (pairs[1] > pairs[3]))
    assert 0.3 < below.mean() < 0.6                                  # about half of them come lower-triangle
    got = oracle_cload(cu.chromsizes_of(cool), int(cool["binsize"]), *pairs)
    assert _same_table(got, cool) and got["dropped"] == 0
    assert np.array_equal(got["bin_start"], cool["bin_start"]) and np.array_equal(got["bin_end"], cool["bin_end"])
    assert [str(x) for x in got["chrom_names"]] == [str(x) for x in cool["chrom_names"]]


def test_round_trip_on_the_toy():
    toy = cu.toy_table(seed=0)
    assert int(toy["chrom_offset"][-1]) == cu.TOY_BINS and toy["count"].sum() == 6000 and toy["count"].max() > 1
    assert np.any(toy["bin1_id"] < 101) and np.any(toy["bin2_id"] >= 102) and np.any(toy["bin1_id"] == toy["bin2_id"])
    got = oracle_cload(cu.TOY, cu.BINSIZE, *pairs_of_table(toy, seed=5))
    assert _same_table(got, toy)


@pytest.mark.parametrize("family", cu.FAMILIES)
def test_adversarial_chunks_hold_what_they_promise(family):
    block = 2048
    for n in (0, 1, 65, block - 1, block, block + 1, 2 * block + 1):
        cols = cu.adversarial_chunk(family, n, block)
        assert all(c.size == n for c in cols)
        want = oracle_cload(cu.TOY, cu.BINSIZE, *cols)
        assert want["count"].sum() == n
        if n == 0:
            continue
        if family == "distinct":
            assert want["count"].size == n
        elif family == "one_pixel":
            assert want["count"].tolist() == [n]
        elif family == "block_runs":
            assert np.all(want["count"][:-1] == block) and want["count"].size == -(-n // block)
        else:
            assert want["count"][-1] == 1 and (want["bin1_id"][-1], want["bin2_id"][-1]) == (cu.TOY_BINS - 1, cu.TOY_BINS - 1)
            assert np.all(want["count"][:-2] == 3)
            if n % block == 1 and n > 1:
                assert int(np.cumsum(want["count"])[-2]) == n - 1          # the last block holds that one pixel and nothing else


# ---- read_pairs ---------------------------------------------------------------------------------------------------------------
ROWS = [("r0", "chr1", 5, "chr2", 17, "+", "-"), ("r1", "chr2", 1, "chr1", 250, "-", "-"), ("r2", "chrM", 9, "chr1", 3, "+", "+"),
        ("r3", "chr1", 250, "chr1", 1, "+", "-"), ("r4", "chr2", 40, "chrM", 2, "-", "+"), ("r5", "NA", 4, "chr2", 4, "+", "+")]
SIZES = {"chr1": 250, "chr2": 40}
WANT = ([0, 1, -1, 0, 1, -1], [5, 1, 9, 250, 40, 4], [1, 0, 0, 0, -1, 1], [17, 250, 3, 1, 2, 4])


def _write(path, rows, chromsize=True, columns=None, order=None):
    lines = ["## pairs format v1.0"]
    if chromsize:
        lines += [f"#chromsize: {name} {size}" for name, size in SIZES.items()]
    if columns:
        lines.append("#columns: " + " ".join(columns))
    for row in rows:
        lines.append("\t".join(str(row[k]) for k in (order or range(len(row)))))
    text = "\n".join(lines) + "\n"
    if str(path).endswith(".gz"):
        with gzip.open(path, "wt") as handle:
            handle.write(text)
    else:
        path.write_text(text)
    return path


def _collect(reader):
    chunks = list(reader)
    return chunks, [np.concatenate([c[k] for c in chunks]).tolist() if chunks else [] for k in range(4)]


@pytest.mark.parametrize("suffix", [".pairs", ".pairs.gz"])
def test_read_pairs_plain_and_gz(tmp_path, suffix):
    reader = cio.read_pairs(_write(tmp_path / f"x{suffix}", ROWS))
    assert reader.chromsizes == SIZES and list(reader.chromsizes) == ["chr1", "chr2"] and reader.columns == (1, 2, 3, 4)
    chunks, cols = _collect(reader)
    assert len(chunks) == 1 and tuple(cols) == tuple(WANT)
    assert [c.dtype for c in chunks[0]] == [np.int32, np.int64, np.int32, np.int64]
    _, again = _collect(reader)                                  # the reader can be walked again
    assert again == cols


def test_read_pairs_header_variants(tmp_path):
    # no #chromsize: lines: the caller's are needed, and their order decides the ids
    bare = _write(tmp_path / "bare.pairs", ROWS, chromsize=False)
    with pytest.raises(ValueError, match="chromsize"):
        cio.read_pairs(bare)
    reader = cio.read_pairs(bare, chromsizes=[("chr2", 40), ("chr1", 250)])
    _, cols = _collect(reader)
    assert cols[0] == [1, 0, -1, 1, 0, -1] and cols[2] == [0, 1, 1, 1, -1, 0] and cols[1] == WANT[1]
    # the caller's chromsizes win over the header's: chr2 becomes a chromosome that is not part of the genome
    _, cols = _collect(cio.read_pairs(_write(tmp_path / "h.pairs", ROWS), chromsizes={"chr1": 250}))
    assert cols[0] == [0, -1, -1, 0, -1, -1]
    # a #columns: line that moves the four fields
    names = ["readID", "strand1", "pos1", "chr1", "strand2", "chr2", "pos2"]
    moved = _write(tmp_path / "moved.pairs", ROWS, columns=names, order=[0, 5, 2, 1, 6, 3, 4])
    reader = cio.read_pairs(moved)
    assert reader.columns == (3, 2, 5, 6)
    assert tuple(_collect(reader)[1]) == tuple(WANT)
    with pytest.raises(ValueError, match="pos2"):
        cio.read_pairs(_write(tmp_path / "nopos.pairs", ROWS, columns=["readID", "chr1", "pos1", "chr2"]))
    # a header and no body
    assert list(cio.read_pairs(_write(tmp_path / "empty.pairs", []))) == []


def test_read_pairs_short_line_names_its_line(tmp_path):
    rows = list(ROWS)
    rows[3] = ("r3", "chr1", 250)
    path = _write(tmp_path / "short.pairs", rows)
    for chunk_rows in (1, 2, 100):
        with pytest.raises(ValueError, match=r"line 7:"):               # 3 header lines, then the 4th row
            list(cio.read_pairs(path, chunk_rows=chunk_rows))
    first = _write(tmp_path / "first.pairs", [("r0", "chr1", 5)] + list(ROWS))
    with pytest.raises(ValueError, match=r"line 4:"):
        list(cio.read_pairs(first))
    with pytest.raises(ValueError, match="not an integer"):
        list(cio.read_pairs(_write(tmp_path / "text.pairs", [("r0", "chr1", "x", "chr2", 17)])))


def test_read_pairs_chunk_boundaries(tmp_path):
    path = _write(tmp_path / "c.pairs.gz", ROWS)
    n = len(ROWS)
    for chunk_rows, sizes in ((1, [1] * n), (n - 1, [n - 1, 1]), (n, [n]), (n + 1, [n])):
        chunks, cols = _collect(cio.read_pairs(path, chunk_rows=chunk_rows))
        assert [c[0].size for c in chunks] == sizes and tuple(cols) == tuple(WANT)
    with pytest.raises(ValueError):
        cio.read_pairs(path, chunk_rows=0)


def test_read_pairs_feeds_the_oracle(tmp_path):
    reader = cio.read_pairs(_write(tmp_path / "o.pairs", ROWS), chunk_rows=4)
    _, cols = _collect(reader)
    got = oracle_cload(reader.chromsizes, 100, *cols)
    # bins: chr1 0-2, chr2 3; r0 (0, 3), r1 (3, 2) reflected, r3 (2, 0) reflected; r2, r4, r5 dropped
    assert got["dropped"] == 3
    assert list(zip(got["bin1_id"].tolist(), got["bin2_id"].tolist(), got["count"].tolist())) == [(0, 2, 1), (0, 3, 1), (2, 3, 1)]


# ---- check_chunk ------------------------------------------------------------------------------------------------------------
def test_check_chunk():
    c, p = np.array([0, 1], dtype=np.int32), np.array([5, 6], dtype=np.int64)
    out = cload.check_chunk(c, p, c, p)
    assert out[0] is c and out[1] is p                                   # no copy where the kinds already fit
    out = cload.check_chunk([0, 1], np.array([5, 6], dtype=np.uint16), np.array([0, -1], dtype=np.int8), [5, 6])
    assert [x.dtype for x in out] == [np.int32, np.int64, np.int32, np.int64] and out[2].tolist() == [0, -1]
    assert all(x.size == 0 for x in cload.check_chunk(np.zeros(0, dtype=np.int8), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)))
    with pytest.raises(ValueError, match="differ in length"):
        cload.check_chunk(c, p, c, p[:1])
    with pytest.raises(ValueError, match="integers"):
        cload.check_chunk(c.astype(np.float64), p, c, p)
    with pytest.raises(ValueError, match="integers"):
        cload.check_chunk(c, p, c, p.astype(np.float32))
    with pytest.raises(ValueError, match="integers"):
        cload.check_chunk(c, p, c.astype(bool), p)
    with pytest.raises(ValueError, match="one-dimensional"):
        cload.check_chunk(c.reshape(1, 2), p, c, p)
    with pytest.raises(ValueError, match="outside int32"):
        cload.check_chunk(np.array([0, 2 ** 31]), p, c, p)
    with pytest.raises(ValueError, match="outside int64"):
        cload.check_chunk(c, np.array([1, 2 ** 63], dtype=np.uint64), c, p)


def test_check_chunk_refuses_more_than_the_kernel_takes():
    # (nobody allocates 2^31 pairs for this: one element, seen 2^31 - 1 times)
    cols = [np.lib.stride_tricks.as_strided(np.zeros(1, dtype=d), shape=(cload.MAX_CHUNK_PAIRS + 1,), strides=(0,))
            for d in (np.int32, np.int64, np.int32, np.int64)]
    with pytest.raises(ValueError, match="2\\^31 - 2"):
        cload.check_chunk(*cols)
    assert cload.MAX_CHUNK_PAIRS == 2 ** 31 - 2
