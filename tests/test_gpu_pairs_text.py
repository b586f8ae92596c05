"""The text of a .pairs file parsed on the device (cs_pairs_text_count / cs_pairs_text_parse, cload.parse_pairs_text,
DeviceCool.from_pairs_file, open_pairs(parse=)) against the host route: the columns of io.read_pairs, the tables of
open_pairs(parse="host") and of tests/cload_util.oracle_cload.  Everything is an integer, so equality is exact throughout."""
import ctypes as C
import gzip

import numpy as np
import pytest

from chromosight_amd import cload, io as cio, pipeline
from chromosight_amd._lib import CsPairsTextFormat, CsPairsTextReport, get_device
from tests import cload_util as cu
from tests import pairs_text_util as pt
from tests.cload_util import BINSIZE, TOY

pytestmark = pytest.mark.gpu

SIZES = (("chr1", 10 ** 18), ("chr10", 10 ** 18), ("chr1_random", 10 ** 18), ("c", 10 ** 18))
NAMES = [n for n, _ in SIZES]
COLUMN_DTYPES = (np.int32, np.int64, np.int32, np.int64)


@pytest.fixture(scope="module")
def dev():
    return get_device()


@pytest.fixture(scope="module")
def tile(dev):
    assert pt.MAX_LINE == cload.MAX_LINE_BYTES >= 4096
    return cload.TEXT_TILE_BYTES


def _device_columns(dev, path):
    """The columns of the body of the file at `path`, parsed on the device in one call with what the host's header pass found."""
    pf = cio.read_pairs(str(path))
    data = path.read_bytes()
    at = 0
    for _ in range(pf.header_lines):
        at = data.index(b"\n", at) + 1
    cols, n, report = cload.parse_pairs_text(dev, data[at:], pf.columns, max(pf.width, max(pf.columns) + 1), list(pf.chromsizes))
    assert report.n_lines == n
    return tuple(c.download()[:n] for c in cols), n, report


def _assert_as_host(dev, tmp_path, text, layout="default", sizes=SIZES, lines=None):
    want, path = pt.host_columns(tmp_path, sizes, text, layout)
    got, n, report = _device_columns(dev, path)
    assert report.first_flagged == -1 and report.reason == 0
    assert n == want[0].size and (lines is None or n == lines)
    for g, w, dt in zip(got, want, COLUMN_DTYPES):
        assert g.dtype == w.dtype == dt and np.array_equal(g, w)
    return got


def _columns(seed, n, n_names=len(NAMES) + 1):
    return pt.random_columns(np.random.default_rng([31, seed]), n, n_names)


ALL_NAMES = NAMES + ["unlisted"]


# ---- tile edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [-1, 0, 1])
@pytest.mark.parametrize("eol", ["\n", "\r\n"])
def test_a_line_end_at_the_edge_of_a_tile(dev, tile, tmp_path, where, eol):
    cols = _columns(1, 300)
    plain = pt.body(ALL_NAMES, *cols, eol=eol)
    k = 40                                          # the line whose '\n' is moved to byte tile + where
    ends = np.flatnonzero(np.frombuffer(plain, dtype=np.uint8) == 10)
    assert ends[k] < tile - 1 and ends.size == 300
    fills = [None] * k + [("r" * (1 + tile + where - int(ends[k])), ".")]
    text = pt.body(ALL_NAMES, *cols, eol=eol, fills=fills)
    assert text[tile + where] == 10 and len(text) > 2 * tile
    _assert_as_host(dev, tmp_path, text, lines=300)


@pytest.mark.parametrize("final", [True, False])
def test_tiles_without_a_line_end(dev, tile, tmp_path, final):
    cols = _columns(2, 200)
    long_id = min(5 * tile // 2, cload.MAX_LINE_BYTES - 1 - 64)
    text = pt.body(ALL_NAMES, *cols, final=final, fills=[None] * 90 + [("r" * long_id, ".")])
    starts = np.concatenate([[0], np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10) + 1])
    assert np.setdiff1d(np.arange(len(text) // tile), starts // tile).size >= 1           # a tile in which no line starts
    _assert_as_host(dev, tmp_path, text, lines=200)


@pytest.mark.parametrize("per_tile", [64, 65])
def test_64_and_65_lines_start_in_one_tile(dev, tile, tmp_path, per_tile):
    length = tile // 64 if per_tile == 64 else tile // 64 - 1
    cols = _columns(3, 3 * per_tile + 10)
    text = pt.fixed_length_body(ALL_NAMES, cols[0], cols[1] % 1000, cols[2], cols[3] % 1000, length)
    starts = np.arange(cols[0].size) * length
    assert per_tile in np.bincount(starts // tile).tolist()
    _assert_as_host(dev, tmp_path, text, lines=cols[0].size)


def test_minimal_lines_fill_two_tiles(dev, tile, tmp_path):
    n = 2 * tile // 8
    text = b"a\t1\ta\t1\n" * n
    assert len(text) == 2 * tile
    got = _assert_as_host(dev, tmp_path, text, layout="bare", sizes=(("a", 10),), lines=n)
    assert not got[0].any() and np.all(got[1] == 1)


@pytest.mark.parametrize("eol", ["\n", "\r\n", ""])
def test_a_single_line_and_an_empty_body(dev, tmp_path, eol):
    got = _assert_as_host(dev, tmp_path, ("r\tchr10\t12\tc\t34\t+\t-" + eol).encode(), lines=1)
    assert [int(g[0]) for g in got] == [1, 12, 3, 34]
    _assert_as_host(dev, tmp_path, b"", lines=0)


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["default", "late", "last"])
@pytest.mark.parametrize("eol, final", [("\n", True), ("\r\n", True), ("\r\n", False)])
def test_layouts(dev, tmp_path, layout, eol, final):
    cols = _columns(4, 500)
    rng = np.random.default_rng(5)
    fills = ["r" * int(rng.integers(1, 40)) for _ in range(500)]
    _assert_as_host(dev, tmp_path, pt.body(ALL_NAMES, *cols, layout=layout, eol=eol, final=final, fills=fills), layout=layout, lines=500)


def test_lines_with_fewer_fields_than_the_first(dev, tmp_path, layout="default"):
    cols = _columns(6, 300)
    columns, width, _ = pt.LAYOUTS[layout]
    rng = np.random.default_rng(7)
    short = {i: int(rng.integers(max(columns) + 1, width + 1)) for i in range(1, 300)}
    assert min(short.values()) == max(columns) + 1 < width
    _assert_as_host(dev, tmp_path, pt.body(ALL_NAMES, *cols, layout=layout, short=short), layout=layout, lines=300)


# ---- positions and names ------------------------------------------------------------------------------------------------------------------
def test_positions(dev, tmp_path):
    values = ["7", "007", str(2 ** 32 + 5), "999999999999999999", "0", "000000000000000000"]
    text = "".join(f".\tc\t{a}\tchr1\t{b}\t+\t-\n" for a in values for b in values).encode()
    got = _assert_as_host(dev, tmp_path, text, lines=36)
    assert got[1].tolist() == [int(a) for a in values for _ in values] and got[3].tolist() == [int(b) for b in values] * 6


def _name_case(dev, tmp_path, names, used):
    """Lines that use the names `used` (strings; unknown ones among them) on either side, against the host reader."""
    sizes = tuple((n, 1000) for n in names)
    text = "".join(f".\t{a}\t5\t{b}\t6\t+\t-\n" for a in used for b in (used[0], used[-1], a)).encode()
    got = _assert_as_host(dev, tmp_path, text, sizes=sizes, lines=3 * len(used))
    index = {n: k for k, n in enumerate(names)}
    assert got[0].tolist() == [index.get(a, -1) for a in used for _ in range(3)]


def test_names_that_are_prefixes_of_each_other_and_unknown_ones(dev, tmp_path):
    _name_case(dev, tmp_path, NAMES, ["chr1", "chr10", "chr1_random", "c", "chr", "chr11", "chr1_rando", "C", "chr1_random_"])


def test_a_255_byte_name_and_a_single_name(dev, tmp_path):
    long_name = "L" * 255
    _name_case(dev, tmp_path, ["chr1", long_name], [long_name, "chr1", long_name[:-1], long_name + "L"])
    _name_case(dev, tmp_path, ["only"], ["only", "onl", "only1"])


def test_4096_names(dev, tmp_path):
    names = [f"scaffold_{k}" for k in range(4096)]
    _name_case(dev, tmp_path, names, names[::37] + ["scaffold_4096", names[-1]])


def test_two_names_on_one_slot_of_the_table(dev, tmp_path):
    lib = dev.lib
    n_names = 8
    slot = lambda name: lib.cs_pairs_text_name_slot(name.encode(), len(name), n_names)         # noqa: E731
    by_slot = {}
    for k in range(400):
        by_slot.setdefault(slot(f"k{k}"), []).append(f"k{k}")
    crowd = max(by_slot.values(), key=len)
    assert len(crowd) >= 3 and slot(crowd[0]) == slot(crowd[1]) == slot(crowd[2]) >= 0
    others = [n for n in (f"k{k}" for k in range(400)) if n not in crowd][:n_names - 3]
    names = [others[0], crowd[0], crowd[1]] + others[1:] + [crowd[2]]
    assert len(names) == n_names
    unknown_same_slot = crowd[3:4] or ["k0x"]
    _name_case(dev, tmp_path, names, crowd[:3] + unknown_same_slot + others[:2])


# ---- flagged lines ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_pairs():
    """6 000 pairs over TOY and, at 7 places, a pair on a chromosome the header does not list."""
    cols = [c.copy() for c in cu.pairs_of_table(cu.toy_table(seed=5), seed=6)]
    other = np.arange(7) * 801 + 3
    cols[0][other[:4]] = len(TOY)
    cols[2][other[4:]] = len(TOY)
    keep = np.ones(cols[0].size, dtype=bool)
    keep[other] = False
    return tuple(cols), keep, [n for n, _ in TOY] + ["other"]


def _table_of(dcool):
    n = dcool.nnz
    return (dcool.indptr.download(), dcool.indices.download()[:n].copy(), dcool.data.download().view(dcool.val_dtype)[:n].copy(),
            np.dtype(dcool.val_dtype))


def _same_tables(a, b):
    ta, tb = _table_of(a), _table_of(b)
    return a.nnz == b.nnz and ta[3] == tb[3] and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(ta[:3], tb[:3]))


def _outcome(call):
    try:
        return call()
    except Exception as exc:                        # noqa: BLE001 (the point is to compare whatever is raised)
        return exc


@pytest.mark.parametrize("family", pt.FAMILIES)
def test_flagged_lines_refuse_the_device_route_and_send_auto_to_the_host(dev, tile, tmp_path, toy_pairs, monkeypatch, family):
    cols, _, names = toy_pairs
    part = [c[:600] for c in cols]
    good = pt.body(names, *part).split(b"\n")[:-1]
    raw, reason = pt.flagged_line(family, "default", pt.fields_of("default", "a", 17, "c", 1500))
    first, second = 5, 450
    lines = good[:first] + [raw] + good[first:second] + [raw] + good[second:]
    text = b"\n".join(lines) + b"\n"
    starts = np.concatenate([[0], np.cumsum([len(x) + 1 for x in lines])])
    assert starts[first] // tile == 0 < starts[second + 1] // tile          # the two bad lines start in different tiles
    head = pt.header(TOY)
    path = tmp_path / f"{family}.pairs"
    path.write_bytes(head.encode() + text)
    n_head = head.count("\n")
    for piece_bytes in (None, 3000):
        with pytest.raises(pipeline.DevicePairsRefused) as info:
            pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="device", piece_bytes=piece_bytes)
        assert str(info.value) == f"{path}, line {n_head + first + 1}: {cload.FLAG_REASONS[reason]}"
    monkeypatch.setattr(pipeline, "AUTO_PARSE_ON_DEVICE", True)
    host = _outcome(lambda: pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="host"))
    auto = _outcome(lambda: pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="auto"))
    if isinstance(host, Exception):
        assert type(auto) is type(host) and str(auto) == str(host)
    else:
        assert _same_tables(auto, host) and auto.dropped == host.dropped


def test_a_bad_line_in_a_later_piece_is_numbered_through_the_file(dev, tmp_path, toy_pairs):
    cols, _, names = toy_pairs
    lines = pt.body(names, *[c[:2000] for c in cols], eol="\r\n").split(b"\n")[:-1]
    lines[1234] = lines[1234].replace(b"\t", b"\t ", 2)             # " <pos1>"
    head = pt.header(TOY)
    path = tmp_path / "late.pairs.gz"
    path.write_bytes(gzip.compress(head.encode() + b"\n".join(lines) + b"\n"))
    with pytest.raises(pipeline.DevicePairsRefused, match=rf"line {head.count(chr(10)) + 1235}: a position that is not 1 to 18 digits"):
        pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="device", piece_bytes=5000)


# ---- streaming ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_files(tmp_path_factory, toy_pairs):
    cols, keep, names = toy_pairs
    text = pt.header(TOY).encode() + pt.body(names, *cols)
    root = tmp_path_factory.mktemp("toy")
    plain, packed = root / "toy.pairs", root / "toy.pairs.gz"
    plain.write_bytes(text)
    packed.write_bytes(gzip.compress(text[:len(text) // 3]) + gzip.compress(text[len(text) // 3:]))
    want = cu.oracle_cload(TOY, BINSIZE, *[c[keep] for c in cols])
    host = pipeline.DeviceCool.from_pairs_file(plain, BINSIZE, parse="host")
    return plain, packed, want, host


@pytest.mark.parametrize("piece", [64, 1000, "T+1", None])
@pytest.mark.parametrize("gz", [False, True])
def test_pieces_of_every_size_give_the_host_routes_table(dev, tile, toy_files, piece, gz):
    plain, packed, want, host = toy_files
    got = pipeline.DeviceCool.from_pairs_file(packed if gz else plain, BINSIZE, parse="device",
                                              piece_bytes=tile + 1 if piece == "T+1" else piece)
    indptr, indices, counts = cu.csr_of(want)
    table = _table_of(got)
    assert got.dropped == host.dropped == 7 and got.nnz == counts.size
    assert np.array_equal(table[0], indptr) and np.array_equal(table[1], indices)
    assert table[2].dtype == counts.dtype and np.array_equal(table[2], counts)
    assert _same_tables(got, host)
    assert got.names == host.names and got.upper and not got.has_weights and got.binsize == BINSIZE


def test_open_pairs_on_either_route(dev, toy_files):
    plain, packed, _, _ = toy_files
    tables = [pipeline.open_pairs(source, BINSIZE, norm="force", resolution=2 * BINSIZE, parse=parse)
              for source, parse in ((plain, "host"), (plain, "device"), (packed, "device"))]
    for other in tables[1:]:
        assert _same_tables(other, tables[0]) and other.dropped == tables[0].dropped == 7 and other.binsize == 2 * BINSIZE
        assert other.has_weights and np.array_equal(other.host_weight, tables[0].host_weight, equal_nan=True)
    with pytest.raises(ValueError, match="chunks"):
        pipeline.open_pairs([tuple(np.zeros(1, dtype=dt) for dt in COLUMN_DTYPES)], BINSIZE, TOY, parse="device")


# ---- the entries ----------------------------------------------------------------------------------------------------------------------------
def test_the_text_is_never_written_and_a_second_parse_gives_the_same(dev, tile):
    cols = _columns(8, 400)
    text = pt.body(ALL_NAMES, *cols, eol="\r\n", final=False)
    resident = dev.to_device(np.frombuffer(text, dtype=np.uint8))
    runs = []
    for _ in range(2):
        got, n, report = cload.parse_pairs_text(dev, resident, (1, 2, 3, 4), 7, NAMES)
        assert (n, report.first_flagged) == (400, -1)
        runs.append([c.download()[:n] for c in got])
    assert all(np.array_equal(a, b) for a, b in zip(*runs))
    assert np.array_equal(runs[0][1], cols[1]) and np.array_equal(runs[0][0], np.where(cols[0] == len(NAMES), -1, cols[0]))
    assert resident.download().tobytes() == text


def test_bad_arguments_are_invalid(dev):
    lib, text = dev.lib, dev.to_device(np.frombuffer(b"a\t1\ta\t1\n" * 4, dtype=np.uint8))
    n = C.c_int64(-1)
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr, 0, C.byref(n)) == 0 and n.value == 0           # empty: no launch
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr, 32, C.byref(n)) == 0 and n.value == 4
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr, 31, C.byref(n)) == 0 and n.value == 4          # no final '\n'
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr, -1, C.byref(n)) == -1
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr + 8, 24, C.byref(n)) == -1                      # not at a multiple of 16
    assert lib.cs_pairs_text_count(dev.ctx, None, None, 8, C.byref(n)) == -1
    assert lib.cs_pairs_text_count(dev.ctx, None, text.ptr, 8, None) == -1
    offsets = np.asarray([0, 1], dtype=np.int64)
    out = [dev.zeros(4, dt) for dt in COLUMN_DTYPES]
    report = CsPairsTextReport()

    def parse(cols=(0, 1, 2, 3), width=4, lines=4, off=offsets, n_names=1):
        fmt = CsPairsTextFormat(*cols, width, n_names, C.cast(C.c_char_p(b"aa"), C.c_void_p), off.ctypes.data_as(C.c_void_p))
        return lib.cs_pairs_text_parse(dev.ctx, None, text.ptr, 32, C.byref(fmt), *[o.ptr for o in out], lines, C.byref(report))
    assert parse() == 0 and (report.n_lines, report.first_flagged, report.reason) == (4, -1, 0)
    assert out[1].download().tolist() == [1, 1, 1, 1] and out[0].download().tolist() == [0, 0, 0, 0]
    assert parse(cols=(0, 1, 2, 2)) == -1 and parse(cols=(0, 1, 2, 4)) == -1 and parse(cols=(-1, 1, 2, 3)) == -1
    assert parse(lines=3) == -1 and parse(lines=5) == -1 and parse(lines=-1) == -1
    assert parse(off=np.asarray([0, 1, 2], dtype=np.int64), n_names=2) == -1                               # "a" twice
    assert parse(off=np.asarray([1, 2], dtype=np.int64)) == -1
    assert parse(width=5) == 0 and report.first_flagged == -1
    assert parse(width=3) == -1
    assert cload.TEXT_TILE_BYTES == lib.cs_pairs_text_tile_bytes() and cload.MAX_LINE_BYTES == lib.cs_pairs_text_max_line_bytes() >= 4096
