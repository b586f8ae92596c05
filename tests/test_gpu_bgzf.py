"""The members of a bgzip-compressed file inflated on the device (cs_bgzf_inflate, engine.run_bgzf_inflate) against Python's zlib, byte
for byte, and a .pairs.gz read with inflate="device" (DeviceCool.from_pairs_file) against the table of the host route, bit for bit.
tests/test_bgzf_host.py has sent the same bodies, valid and corrupt, through the sanitizer build of the decoder first."""
import gzip
import struct
import zlib

import numpy as np
import pytest

from chromosight_amd import cload, engine, io as cio, pipeline
from chromosight_amd._lib import get_device
from tests import bgzf_util as bu
from tests import cload_util as cu
from tests import pairs_text_util as pt
from tests.cload_util import BINSIZE, TOY

pytestmark = pytest.mark.gpu

CANARY = 0xC5
CS_ERR_CORRUPT = -6


@pytest.fixture(scope="module")
def dev():
    return get_device()


class Packed:
    """Bodies put into one buffer of file bytes, each followed by its CRC-32 and ISIZE as in a member, `gap` bytes of filler between
    (an odd gap puts the bodies at unaligned offsets)."""

    def __init__(self, members, gap=3):
        parts, self.offsets, self.nbytes, self.isizes = [], [], [], []
        at = 0
        for body, isize, crc in members:
            parts.append(b"\xEE" * gap + body + struct.pack("<II", crc, isize))
            self.offsets.append(at + gap)
            self.nbytes.append(len(body))
            self.isizes.append(isize)
            at += len(parts[-1])
        self.data = np.frombuffer(b"".join(parts), dtype=np.uint8)


def _inflate(dev, packed, out_offsets, text_bytes, expect_corrupt=False):
    """One call: (status, last newline, the text buffer afterwards, the return code)."""
    d_file = dev.to_device(packed.data)
    d_text = dev.to_device(np.full(max(text_bytes, 1), CANARY, dtype=np.uint8))
    try:
        status, last = engine.run_bgzf_inflate(dev, d_file, packed.data.size, packed.offsets, packed.nbytes, out_offsets, packed.isizes, d_text,
                                               text_bytes)
        rc = 0
    except engine.CorruptChunks as exc:
        assert expect_corrupt, str(exc)
        status, last, rc = exc.status, None, CS_ERR_CORRUPT
    assert np.array_equal(d_file.download(), packed.data)             # the input is never written
    return status, last, d_text.download()[:text_bytes], rc


def _member(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    return bu.deflate_raw(raw, level, strategy), len(raw), zlib.crc32(raw)


# ---- valid bodies -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(16))
def test_each_body_as_its_own_block(dev, k):
    name, body, raw = bu.bodies()[k]
    assert len(bu.bodies()) == 16
    for out_offset in (0, 5):
        text_bytes = out_offset + len(raw) + 9
        status, last, text, _ = _inflate(dev, Packed([(body, len(raw), zlib.crc32(raw))]), [out_offset], text_bytes)
        assert status.tolist() == [0], name
        assert text[out_offset:out_offset + len(raw)].tobytes() == raw, name
        assert np.all(text[:out_offset] == CANARY) and np.all(text[out_offset + len(raw):] == CANARY), name
        assert last == (out_offset + raw.rfind(b"\n") if b"\n" in raw else -1), name


def test_all_bodies_in_one_call_packed_at_unaligned_offsets_in_shuffled_order(dev):
    rng = np.random.default_rng(17)
    small = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in (1, 7, 15, 17)] + [b"\n", b"ab\ncd\n\n"]
    raws = [b""] + [raw for _, _, raw in bu.bodies()[:8]] + [b""] + small + [raw for _, _, raw in bu.bodies()[8:]] + [b""]
    bodies = {raw: body for _, body, raw in bu.bodies()}
    members = [(bodies[raw], len(raw), zlib.crc32(raw)) if raw in bodies else _member(raw) for raw in raws]
    # the texts stand against each other from byte 3 on, but for three gaps of 1, 16 and 37 bytes; 50 bytes are left behind the last
    out_offsets, at = [], 3
    gaps = {4: 1, 11: 16, 15: 37}
    for i, raw in enumerate(raws):
        at += gaps.get(i, 0)
        out_offsets.append(at)
        at += len(raw)
    text_bytes = at + 50
    assert len({o % 16 for o, r in zip(out_offsets, raws) if r}) >= 8            # heads of many alignments
    order = rng.permutation(len(raws))
    packed = Packed([members[i] for i in order], gap=5)
    status, last, text, _ = _inflate(dev, packed, [out_offsets[i] for i in order], text_bytes)
    assert not status.any()
    want = np.full(text_bytes, CANARY, dtype=np.uint8)
    for o, raw in zip(out_offsets, raws):
        want[o:o + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    assert np.array_equal(text, want)               # every byte: the texts, the gaps between them and the bytes beyond the last
    newlines = [o + raw.rfind(b"\n") for o, raw in zip(out_offsets, raws) if b"\n" in raw]
    assert last == max(newlines)


def test_full_blocks(dev):
    text = bu.pairs_text_block()
    members = [_member(text, lv) for lv in (1, 6, 9)] + [_member(text, 6, zlib.Z_FIXED), _member(text[:65280], 0)]
    assert [m[1] for m in members] == [65536] * 4 + [65280] and engine.bgzf_max_block_bytes() == 65536
    out_offsets = np.concatenate([[7], 7 + np.cumsum([m[1] for m in members])[:-1]])
    total = 7 + sum(m[1] for m in members)
    status, last, got, _ = _inflate(dev, Packed(members, gap=1), out_offsets, total + 1)
    assert not status.any()
    assert got[7:total].tobytes() == text * 4 + text[:65280] and got[total] == CANARY and np.all(got[:7] == CANARY)
    assert last == out_offsets[-1] + text[:65280].rfind(b"\n")


def test_blocks_without_text_only(dev):
    status, last, text, _ = _inflate(dev, Packed([_member(b"")] * 3), [0, 4, 8], 8)
    assert not status.any() and last == -1 and np.all(text == CANARY)
    assert engine.run_bgzf_inflate(dev, None, 0, [], [], [], [], None, 0)[1] == -1


# ---- corrupt bodies -----------------------------------------------------------------------------------------------------------------------
def test_corrupt_blocks_among_valid_neighbours(dev):
    valid = [(body, len(raw), zlib.crc32(raw), raw) for _, body, raw in bu.bodies()]
    cases = list(bu.corruptions(300))
    members, wants = [], []
    for i, (label, body, isize, crc) in enumerate(cases):
        members.append((body, isize, crc))
        wants.append(bu.body_verdict(body, isize, crc))
        if i % 3 == 0:
            body, isize, crc, raw = valid[(i // 3) % len(valid)]
            members.append((body, isize, crc))
            wants.append(raw)
    out_offsets = np.concatenate([[1], 1 + np.cumsum([m[1] for m in members])[:-1]])
    total = 1 + sum(m[1] for m in members)
    status, _, text, rc = _inflate(dev, Packed(members), out_offsets, total, expect_corrupt=True)
    assert rc == CS_ERR_CORRUPT and sum(w is None for w in wants) > 150
    for k, (o, (_, isize, _), want) in enumerate(zip(out_offsets, members, wants)):
        assert (status[k] == 0) == (want is not None), k
        if want is None:
            assert 2 <= status[k] <= 11 and np.all(text[o:o + isize] == CANARY), k          # a failed block leaves its canary
        else:
            assert text[o:o + isize].tobytes() == want, k                                   # its neighbours decode
    assert text[0] == CANARY


def test_one_body_per_status(dev):
    cases = bu.failure_bodies()
    good = _member(b"a neighbour\n")
    members = [good] + [(body, isize, crc) for _, _, body, isize, crc in cases] + [good]
    out_offsets = np.concatenate([[0], np.cumsum([m[1] for m in members])[:-1]])
    packed, total = Packed(members), sum(m[1] for m in members)
    status, _, text, rc = _inflate(dev, packed, out_offsets, total, expect_corrupt=True)
    assert rc == CS_ERR_CORRUPT and status.tolist() == [0] + [s for s, *_ in cases] + [0]
    assert text[:12].tobytes() == text[-12:].tobytes() == b"a neighbour\n" and np.all(text[12:-12] == CANARY)
    with pytest.raises(engine.CorruptChunks, match=rf"{len(cases)} of {len(members)} blocks failed; the first is block 1 \("):
        engine.run_bgzf_inflate(dev, dev.to_device(packed.data), packed.data.size, packed.offsets, packed.nbytes, out_offsets, packed.isizes,
                                dev.empty(total, np.uint8), total)


# ---- descriptors --------------------------------------------------------------------------------------------------------------------------
def test_bad_descriptors_are_refused_before_any_launch(dev):
    raw = b"some text\n" * 20
    packed = Packed([_member(raw), _member(raw)], gap=0)
    n, size = len(raw), packed.data.size
    d_file = dev.to_device(packed.data)
    d_text = dev.to_device(np.full(2 * n, CANARY, dtype=np.uint8))

    def call(offsets=packed.offsets, nbytes=packed.nbytes, out_offsets=(0, n), isizes=(n, n), file_bytes=size, text_bytes=2 * n):
        return engine.run_bgzf_inflate(dev, d_file, file_bytes, offsets, nbytes, out_offsets, isizes, d_text, text_bytes)

    bad = [dict(offsets=[packed.offsets[0], -1]), dict(offsets=[packed.offsets[0], size]), dict(nbytes=[packed.nbytes[0], -1]),
           dict(file_bytes=size - 5),                                   # the last body's CRC-32 leaves the span
           dict(file_bytes=-1), dict(text_bytes=-1), dict(out_offsets=[0, -1]), dict(out_offsets=[0, n + 1]), dict(text_bytes=2 * n - 1),
           dict(isizes=[n, -1]),
           dict(out_offsets=[0, n - 1]), dict(out_offsets=[5, 5]), dict(out_offsets=[n, 1])]          # texts that overlap
    for kwargs in bad:
        with pytest.raises(ValueError) as info:
            call(**kwargs)
        assert not isinstance(info.value, engine.CorruptChunks), kwargs
    with pytest.raises(NotImplementedError, match="65536"):
        call(isizes=[n, 65537], text_bytes=1 << 20)
    with pytest.raises(ValueError, match="differ in length"):
        call(isizes=[n])
    assert np.all(d_text.download() == CANARY)                           # nothing was launched
    status, last = call()
    assert not status.any() and d_text.download().tobytes() == raw * 2 and last == 2 * n - 1


# ---- a .pairs.gz, end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_pairs():
    """6 000 pairs over TOY and, at 7 places, a pair on a chromosome the header does not list."""
    cols = [c.copy() for c in cu.pairs_of_table(cu.toy_table(seed=5), seed=6)]
    other = np.arange(7) * 801 + 3
    cols[0][other[:4]] = len(TOY)
    cols[2][other[4:]] = len(TOY)
    return tuple(cols), [n for n, _ in TOY] + ["other"]


def _table_of(dcool):
    n = dcool.nnz
    return (dcool.indptr.download(), dcool.indices.download()[:n].copy(), dcool.data.download().view(dcool.val_dtype)[:n].copy(),
            np.dtype(dcool.val_dtype))


def _same_tables(a, b):
    ta, tb = _table_of(a), _table_of(b)
    return a.nnz == b.nnz and ta[3] == tb[3] and all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(ta[:3], tb[:3]))


def _piece(piece):
    return cload.TEXT_TILE_BYTES + 1 if piece == "T+1" else piece


@pytest.fixture(scope="module")
def toy_texts(tmp_path_factory, toy_pairs):
    """name -> (text of the file, the table of parse="host" over it): 6 000 lines with either line end, with and without the last one;
    300 lines; a header alone."""
    cols, names = toy_pairs
    root = tmp_path_factory.mktemp("bgzf_host")
    out = {}

    def add(name, text):
        path = root / f"{name}.pairs"
        path.write_bytes(text)
        out[name] = (text, pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="host"))

    for eol, tag in (("\n", "lf"), ("\r\n", "crlf")):
        for final in (True, False):
            add(f"{tag}-{'final' if final else 'open'}", pt.header(TOY, eol=eol).encode() + pt.body(names, *cols, eol=eol, final=final))
    add("small", pt.header(TOY).encode() + pt.body(names, *[c[:300] for c in cols]))
    add("header", pt.header(TOY).encode())
    return out


def _check_route(tmp_path, toy_texts, name, block_bytes, piece):
    text, host = toy_texts[name]
    path = tmp_path / f"{name}.pairs.gz"
    path.write_bytes(bu.bgzf_file(text, block_bytes))
    got = pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="device", inflate="device", piece_bytes=_piece(piece))
    assert _same_tables(got, host) and got.dropped == host.dropped
    assert got.names == host.names and got.upper and not got.has_weights and got.binsize == BINSIZE
    return got


@pytest.mark.parametrize("piece", [64, 1000, "T+1", None])
@pytest.mark.parametrize("block_bytes", [4096, 65280])
@pytest.mark.parametrize("name", ["lf-final", "lf-open", "crlf-final", "crlf-open"])
def test_a_bgzf_pairs_file_gives_the_host_routes_table(dev, tmp_path, toy_texts, name, block_bytes, piece):
    got = _check_route(tmp_path, toy_texts, name, block_bytes, piece)
    assert got.dropped == 7 and got.nnz > 1000


@pytest.mark.parametrize("piece", [64, 1000, "T+1", None])
@pytest.mark.parametrize("block_bytes", [1, 7])
def test_blocks_of_1_and_7_bytes(dev, tmp_path, toy_texts, block_bytes, piece):
    """The header ends at the end of a block (1 byte) and inside one (7 bytes), spans many blocks, and every line spans three or more."""
    text = toy_texts["small"][0]
    head = len(pt.header(TOY))
    assert head % 7 != 0 and head > 10 * 7 and min(len(line) for line in text[head:].split(b"\n")[:-1]) + 1 >= 2 * 7 + 2      # (with its '\n')
    _check_route(tmp_path, toy_texts, "small", block_bytes, piece)


@pytest.mark.parametrize("piece", [64, None])
@pytest.mark.parametrize("block_bytes", [7, 65280])
def test_a_header_alone(dev, tmp_path, toy_texts, block_bytes, piece):
    got = _check_route(tmp_path, toy_texts, "header", block_bytes, piece)
    assert got.nnz == 0 and got.dropped == 0


def test_open_pairs_takes_the_argument(dev, tmp_path, toy_texts):
    text, _ = toy_texts["lf-final"]
    path = tmp_path / "toy.pairs.gz"
    path.write_bytes(bu.bgzf_file(text))
    tables = [pipeline.open_pairs(path, BINSIZE, norm="force", resolution=2 * BINSIZE, inflate=inflate) for inflate in ("host", "device")]
    assert _same_tables(*tables) and tables[0].dropped == tables[1].dropped == 7
    assert np.array_equal(tables[0].host_weight, tables[1].host_weight, equal_nan=True)
    timings = {}
    cload.pairs_file_device(cio.read_pairs(str(path)), BINSIZE, timings=timings, inflate="device")
    assert timings["inflate"] > 0 and {"read", "upload", "count", "parse", "bin"} <= set(timings)


def test_a_flagged_line_in_a_later_piece_carries_its_file_line_number(dev, tmp_path, toy_pairs):
    cols, names = toy_pairs
    lines = pt.body(names, *[c[:2000] for c in cols], eol="\r\n").split(b"\n")[:-1]
    lines[1234] = lines[1234].replace(b"\t", b"\t ", 2)             # " <pos1>"
    head = pt.header(TOY)
    path = tmp_path / "late.pairs.gz"
    path.write_bytes(bu.bgzf_file(head.encode() + b"\n".join(lines) + b"\n", 4096))
    with pytest.raises(pipeline.DevicePairsRefused, match=rf"line {head.count(chr(10)) + 1235}: a position that is not 1 to 18 digits"):
        pipeline.DeviceCool.from_pairs_file(path, BINSIZE, parse="device", inflate="device", piece_bytes=5000)


def test_plain_gzip_is_refused_by_device_and_goes_to_the_host_with_auto(dev, tmp_path, toy_texts, monkeypatch):
    text, host = toy_texts["lf-open"]
    path = tmp_path / "plain.pairs.gz"
    path.write_bytes(gzip.compress(text))
    with pytest.raises(pipeline.DeviceInflateRefused, match="member 0 at byte 0"):
        pipeline.DeviceCool.from_pairs_file(path, BINSIZE, inflate="device")
    monkeypatch.setattr(pipeline, "AUTO_INFLATE_ON_DEVICE", True)
    auto = pipeline.DeviceCool.from_pairs_file(path, BINSIZE, inflate="auto")
    assert _same_tables(auto, host) and auto.dropped == host.dropped


def _outcome(call):
    try:
        return call()
    except Exception as exc:                        # noqa: BLE001 (the point is to compare whatever is raised)
        return exc


def test_a_corrupted_block_is_named_by_device_and_raised_by_the_host_with_auto(dev, tmp_path, toy_texts, monkeypatch):
    text, _ = toy_texts["lf-final"]
    data = bytearray(bu.bgzf_file(text, 4096))
    blocks = list(cload.bgzf_blocks(bytes(data)))
    k = 9
    b = blocks[k]
    data[b.body_offset + b.body_bytes // 2] ^= 0x55
    body = bytes(data[b.body_offset:b.body_offset + b.body_bytes])
    assert bu.body_verdict(body, b.isize, struct.unpack_from("<I", data, b.body_offset + b.body_bytes)[0]) is None
    path = tmp_path / "corrupt.pairs.gz"
    path.write_bytes(bytes(data))
    with pytest.raises(engine.CorruptChunks, match=rf"BGZF member {k} at byte {b.file_offset} does not decode") as info:
        pipeline.DeviceCool.from_pairs_file(path, BINSIZE, inflate="device", piece_bytes=10_000)
    assert info.value.block == k and info.value.file_offset == b.file_offset and 2 <= int(info.value.status[0]) <= 11
    monkeypatch.setattr(pipeline, "AUTO_INFLATE_ON_DEVICE", True)
    host = _outcome(lambda: pipeline.DeviceCool.from_pairs_file(path, BINSIZE, inflate="host"))
    auto = _outcome(lambda: pipeline.DeviceCool.from_pairs_file(path, BINSIZE, inflate="auto"))
    assert isinstance(host, Exception) and type(auto) is type(host) and str(auto) == str(host)
