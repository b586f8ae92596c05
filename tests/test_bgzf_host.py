"""The host side of the device inflate of a bgzip-compressed .pairs.gz: the fixtures of tests/bgzf_util.py against Python's gzip, the
member walker cload.bgzf_blocks on hand-built files, the rules by which from_pairs_file / open_pairs(inflate=) pick a route, and the
member decoder of cs_inflate.hip (cs_inflate_core.h inflate_member and its CRC-32) as a host program under the address and
undefined-behaviour sanitizers (tools/bgzf_check.cpp) on valid and corrupted bodies.  No GPU."""
import gzip
import pathlib
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from chromosight_amd import cload, engine, pipeline
from tests import bgzf_util as bu
from tests import inflate_util as iu
from tests import pairs_text_util as pt

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "chromosight_amd" / "csrc"


# ---- the fixtures are what gzip says they are ---------------------------------------------------------------------------------------------
def test_the_writer_gives_the_canonical_end_marker():
    assert bu.block(b"") == bu.END_MARKER and len(bu.END_MARKER) == 28
    assert bu.bgzf_file(b"") == bu.END_MARKER and gzip.decompress(bu.END_MARKER) == b""


def test_sixteen_of_the_seventeen_streams_rewrap_as_members():
    names = [name for name, _, _ in bu.bodies()]
    assert len(iu.gzip_streams()) == 17 and len(names) == 16
    assert [n for n, _, _ in iu.gzip_streams() if n not in names] == ["64 KiB at level 0"]
    big = [s for n, s, _ in iu.gzip_streams() if n == "64 KiB at level 0"][0]
    assert 12 + 6 + len(big) - 6 + 8 == 65572
    for name, body, raw in bu.bodies():
        member = bu.frame(body, len(raw), zlib.crc32(raw))
        assert gzip.decompress(member) == raw, name
        assert bu.body_of(member) == (body, len(raw), zlib.crc32(raw)), name
        assert bu.body_verdict(body, len(raw), zlib.crc32(raw)) == raw, name


def test_a_full_block_of_pairs_text_and_a_stored_bgzip_block_fit():
    text = bu.pairs_text_block()
    assert len(text) == 65536 and text.count(b"\n") > 1000
    for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
                            (6, zlib.Z_HUFFMAN_ONLY)):
        member = bu.block(text, level, strategy)
        assert 20_000 <= len(member) <= 33_000, (level, strategy, len(member))
        assert gzip.decompress(member) == text
    noise = np.random.default_rng(2).integers(0, 256, bu.BGZIP_BLOCK, dtype=np.uint8).tobytes()
    stored = bu.block(noise, level=0)
    assert len(stored) == 65316 and gzip.decompress(stored) == noise


def test_every_failure_body_is_refused_by_the_judge():
    cases = bu.failure_bodies()
    assert {s for s, *_ in cases} == {2, 3, 4, 5, 6, 7, 8, 9, 11}
    for _, label, body, isize, crc in cases:
        assert bu.body_verdict(body, isize, crc) is None, label


# ---- the walker -----------------------------------------------------------------------------------------------------------------------------
TEXT = b"".join(b"line %d\tof the text\n" % k for k in range(3000))


def _walk(data):
    return list(cload.bgzf_blocks(data))


def _check_walk(data, texts):
    blocks = _walk(data)
    assert [b.isize for b in blocks] == [len(t) for t in texts]
    at = 0
    for b, t in zip(blocks, texts):
        assert b.file_offset == at and at < b.body_offset
        body = data[b.body_offset:b.body_offset + b.body_bytes]
        crc, isize = struct.unpack_from("<II", data, b.body_offset + b.body_bytes)
        assert bu.body_verdict(body, isize, crc) == t and isize == b.isize
        at = b.body_offset + b.body_bytes + 8
    assert at == len(data)
    assert gzip.decompress(data) == b"".join(texts)


def test_the_walker_on_files_that_qualify():
    cut = [TEXT[at:at + 4096] for at in range(0, len(TEXT), 4096)]
    _check_walk(bu.bgzf_file(TEXT, 4096), cut + [b""])
    _check_walk(bu.bgzf_file(TEXT, 4096, end_marker=False), cut)             # a file without the end marker
    _check_walk(bu.bgzf_file(TEXT[:65536], 65536), [TEXT[:65536], b""])      # the most text a member holds
    _check_walk(b"", [])
    _check_walk(bu.END_MARKER + bu.block(TEXT[:10]) + bu.END_MARKER, [b"", TEXT[:10], b""])      # the marker is an ordinary member
    other = (82, 71, b"samtools")                                            # other subfields before and behind 'BC'
    _check_walk(bu.block(TEXT[:100], before=[other]) + bu.block(TEXT[100:300], after=[other, (1, 2, b"")])
                + bu.block(TEXT[300:400], before=[other], after=[other]), [TEXT[:100], TEXT[100:300], TEXT[300:400]])


def _flags(member, flags, insert=b""):
    """The member with other gzip flags and `insert` between its extra field and its body (BSIZE is what it was)."""
    xlen, = struct.unpack_from("<H", member, 10)
    return member[:3] + bytes([flags]) + member[4:12 + xlen] + insert + member[12 + xlen:]


@pytest.mark.parametrize("what, data", [
    ("plain gzip output", gzip.compress(TEXT)),
    ("plain gzip behind a member", bu.block(TEXT[:50]) + gzip.compress(TEXT[50:])),
    ("FNAME", _flags(bu.block(TEXT[:50]), 4 | 8, b"name\0")),
    ("FCOMMENT", _flags(bu.block(TEXT[:50]), 4 | 16, b"comment\0")),
    ("FHCRC", _flags(bu.block(TEXT[:50]), 4 | 2, b"\x12\x34")),
    ("no extra field", b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + bu.deflate_raw(TEXT[:50]) + struct.pack("<II", zlib.crc32(TEXT[:50]), 50)),
    ("zero padding between members", bu.block(TEXT[:50]) + bytes(4) + bu.block(TEXT[50:90])),
    ("trailing bytes", bu.bgzf_file(TEXT[:5000], 4096) + b"\0"),
    ("a trailing fraction of a header", bu.bgzf_file(TEXT[:5000], 4096) + bu.END_MARKER[:11]),
    ("a truncated last block", bu.bgzf_file(TEXT[:9000], 4096, end_marker=False)[:-1]),
    ("a truncated end marker", bu.bgzf_file(TEXT[:9000], 4096)[:-5]),
    ("an extra field without 'BC'", bu.block(TEXT[:50]).replace(b"BC\x02\x00", b"BD\x02\x00", 1)),
    ("two 'BC' subfields", bu.block(TEXT[:50], before=[(66, 67, b"\x01\x02")])),
    ("a 'BC' subfield of 4 bytes", bu.block(TEXT[:50]).replace(b"\x06\x00BC\x02\x00", b"\x06\x00BC\x04\x00", 1)),
    ("subfields that do not fill the extra field", bu.block(TEXT[:50], after=[(1, 2, b"abc")]).replace(b"\x01\x02\x03\x00abc", b"\x01\x02\x09\x00abc", 1)),
    ("another method", bu.block(TEXT[:50])[:2] + b"\x07" + bu.block(TEXT[:50])[3:]),
    ("a size that does not hold the header and trailer", bu.block(b"")[:16] + struct.pack("<H", 20) + bu.block(b"")[18:]),
])
def test_the_walker_refuses_what_does_not_qualify(what, data):
    with pytest.raises(pipeline.DeviceInflateRefused):
        _walk(data)
    assert issubclass(pipeline.DeviceInflateRefused, ValueError)


def test_an_isize_above_a_block_is_refused():
    member = bytearray(bu.block(TEXT[:50]))
    member[-4:] = struct.pack("<I", 65537)
    with pytest.raises(pipeline.DeviceInflateRefused, match="65537"):
        _walk(bytes(member))
    member[-4:] = struct.pack("<I", 65536)
    assert _walk(bytes(member))[0].isize == 65536


def test_the_refused_fixtures_are_gzip_files_where_they_claim_to_be():
    """What sends "auto" back to the host is readable there: gzip reads plain output, names, comments and padding."""
    assert gzip.decompress(gzip.compress(TEXT)) == TEXT
    assert gzip.decompress(_flags(bu.block(TEXT[:50]), 4 | 8, b"name\0")) == TEXT[:50]
    assert gzip.decompress(_flags(bu.block(TEXT[:50]), 4 | 16, b"comment\0")) == TEXT[:50]
    assert gzip.decompress(bu.block(TEXT[:50]) + bytes(4) + bu.block(TEXT[50:90])) == TEXT[:90]


# ---- routing --------------------------------------------------------------------------------------------------------------------------------
SIZES = (("chr1", 1000), ("chr2", 500))


def _toy(tmp_path, name, packer):
    text = pt.header(SIZES).encode() + b"r\tchr1\t5\tchr2\t7\t+\t-\n"
    path = tmp_path / name
    path.write_bytes(packer(text))
    return path


@pytest.fixture()
def routes(monkeypatch):
    """from_pairs_file with its loaders replaced: the list receives ("device parse", inflate) and "host reader"."""
    seen = []

    def fake_device(pairs_file, binsize, zero_based=False, piece_bytes=None, dev=None, timings=None, inflate="host"):
        seen.append(("device parse", inflate))
        if inflate == "device":
            list(cload.bgzf_blocks(pathlib.Path(pairs_file.path).read_bytes()))          # refuses what the walker refuses
        return "table"

    monkeypatch.setattr(cload, "pairs_file_device", fake_device)
    monkeypatch.setattr(pipeline.DeviceCool, "from_pairs", classmethod(lambda cls, *a, **k: seen.append("host reader") or "host table"))
    monkeypatch.setattr(pipeline, "AUTO_PARSE_ON_DEVICE", True)
    monkeypatch.delenv("CHROMOSIGHT_HIP_HOST_INFLATE", raising=False)
    monkeypatch.delenv("CHROMOSIGHT_HIP_HOST_PARSE", raising=False)
    return seen


def test_the_inflate_argument_picks_the_route(tmp_path, routes, monkeypatch):
    bgzf = _toy(tmp_path, "b.pairs.gz", lambda t: bu.bgzf_file(t, 64))
    plain_gz = _toy(tmp_path, "g.pairs.gz", gzip.compress)
    load = pipeline.DeviceCool.from_pairs_file
    assert load(bgzf, 100, inflate="host") == "table" and routes == [("device parse", "host")]
    routes.clear()
    assert load(bgzf, 100, inflate="device") == "table" and routes == [("device parse", "device")]
    routes.clear()
    with pytest.raises(pipeline.DeviceInflateRefused):
        load(plain_gz, 100, inflate="device")
    assert routes == [("device parse", "device")]
    for auto_on, want in ((True, [("device parse", "device")]), (False, [("device parse", "host")])):
        routes.clear()
        monkeypatch.setattr(pipeline, "AUTO_INFLATE_ON_DEVICE", auto_on)
        assert load(bgzf, 100, inflate="auto") == load(bgzf, 100) == "table" and routes == want * 2
    routes.clear()
    monkeypatch.setattr(pipeline, "AUTO_INFLATE_ON_DEVICE", True)
    assert load(plain_gz, 100) == "table" and routes == [("device parse", "device"), ("device parse", "host")]       # refused: the host inflates
    routes.clear()
    assert load(bgzf, 100, parse="host") == "host table" and routes == ["host reader"]
    routes.clear()
    monkeypatch.setenv("CHROMOSIGHT_HIP_HOST_INFLATE", "1")
    assert load(bgzf, 100) == "table" and routes == [("device parse", "host")]
    with pytest.raises(ValueError, match="CHROMOSIGHT_HIP_HOST_INFLATE"):
        load(bgzf, 100, inflate="device")


def test_a_corrupt_member_sends_auto_to_the_host_and_device_raises(tmp_path, routes, monkeypatch):
    bgzf = _toy(tmp_path, "b.pairs.gz", lambda t: bu.bgzf_file(t, 64))

    def corrupt(pairs_file, binsize, inflate="host", **_):
        routes.append(("device parse", inflate))
        if inflate == "device":
            raise engine.CorruptChunks("member 3", np.asarray([9]))
        return "table"

    monkeypatch.setattr(cload, "pairs_file_device", corrupt)
    monkeypatch.setattr(pipeline, "AUTO_INFLATE_ON_DEVICE", True)
    assert pipeline.DeviceCool.from_pairs_file(bgzf, 100) == "table" and routes == [("device parse", "device"), ("device parse", "host")]
    with pytest.raises(engine.CorruptChunks):
        pipeline.DeviceCool.from_pairs_file(bgzf, 100, inflate="device")


def test_value_errors_of_the_inflate_argument(tmp_path, routes):
    bgzf = _toy(tmp_path, "b.pairs.gz", lambda t: bu.bgzf_file(t, 64))
    plain = _toy(tmp_path, "p.pairs", lambda t: t)
    with pytest.raises(ValueError, match="inflate must be one of"):
        pipeline.DeviceCool.from_pairs_file(bgzf, 100, inflate="gpu")
    with pytest.raises(ValueError, match="parse='host'"):
        pipeline.DeviceCool.from_pairs_file(bgzf, 100, inflate="device", parse="host")
    with pytest.raises(ValueError, match=r"\.gz"):
        pipeline.DeviceCool.from_pairs_file(plain, 100, inflate="device")
    chunk = tuple(np.zeros(1, dtype=dt) for dt in (np.int32, np.int64, np.int32, np.int64))
    with pytest.raises(ValueError, match="chunks"):
        pipeline.open_pairs([chunk], 100, dict(SIZES), inflate="device")
    with pytest.raises(ValueError, match="chunks"):
        pipeline.open_pairs([chunk], 100, dict(SIZES), inflate="host")
    assert routes == []
    assert pipeline.DeviceCool.from_pairs_file(plain, 100) == "table" and routes == [("device parse", "host")]      # not a .gz: nothing to inflate


@pytest.mark.parametrize("what", ["a byte of the body", "the CRC-32", "ISIZE"])
def test_a_corrupt_member_of_the_header_is_named_by_the_host(what):
    """The members that hold the header are inflated by the host's zlib, before any device is asked for anything."""
    import types
    text = pt.header(SIZES).encode() + b"r\tchr1\t5\tchr2\t7\t+\t-\n" * 40
    data = bytearray(bu.bgzf_file(text, 50))
    second = list(cload.bgzf_blocks(bytes(data)))[1]
    assert len(pt.header(SIZES)) > 50                                        # the header's lines reach into the second member
    end = second.body_offset + second.body_bytes
    at = {"a byte of the body": second.body_offset + 3, "the CRC-32": end, "ISIZE": end + 4}[what]
    data[at] ^= 0x01
    pf = types.SimpleNamespace(path="toy.pairs.gz", header_lines=pt.header(SIZES).count("\n"))
    with pytest.raises(engine.CorruptChunks, match=rf"toy.pairs.gz: BGZF member 1 at byte {second.file_offset} does not decode") as info:
        next(cload._device_inflated_pieces(pf, bytes(data), 1000, None, None))
    assert info.value.block == 1 and info.value.file_offset == second.file_offset and info.value.status.tolist() == [-1]


def test_the_limit_of_a_block_needs_no_gpu():
    assert engine.bgzf_max_block_bytes() == cload.BGZF_MAX_ISIZE == bu.MAX_BLOCK == 65536
    assert len(engine.BGZF_STATUS) == 12 and engine.BGZF_STATUS[:9] == engine.INFLATE_STATUS[:9]


# ---- the member decoder under the sanitizers ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler")
    subprocess.run(["make", "-C", str(CSRC), "bgzf_check"], check=True, capture_output=True)
    return CSRC / "build" / "bgzf_check"


def _run(checker, tmp_path, records, buffer=b"", splits=()):
    path = tmp_path / "records.bin"
    bu.write_records(path, records, buffer, splits)
    res = subprocess.run([str(checker), str(path)], capture_output=True, text=True)
    assert res.returncode == 0, f"bgzf_check ended with {res.returncode} (a sanitizer report?)\n{res.stderr[-4000:]}"
    lines = res.stdout.splitlines()
    assert len(lines) == len(records) + len(splits)
    return [tuple(int(x) for x in line.split()) for line in lines[:len(records)]], lines[len(records):]


def test_core_decodes_the_sixteen_bodies_and_full_blocks(checker, tmp_path):
    cases = [(name, body, raw) for name, body, raw in bu.bodies()]
    text = bu.pairs_text_block()
    cases += [(f"pairs text, level {lv}", bu.deflate_raw(text, lv), text) for lv in (1, 6, 9)]
    cases += [("pairs text, Z_FIXED", bu.deflate_raw(text, 6, zlib.Z_FIXED), text), ("65 280 bytes stored", bu.deflate_raw(text[:65280], 0), text[:65280]),
              ("no text", bu.deflate_raw(b""), b""), ("one byte", bu.deflate_raw(b"\n"), b"\n")]
    got, _ = _run(checker, tmp_path, [(body, len(raw), zlib.crc32(raw), raw) for _, body, raw in cases])
    for (name, _, _), verdict in zip(cases, got):
        assert verdict == (0, 1), name


def test_core_names_every_failure(checker, tmp_path):
    cases = bu.failure_bodies()
    got, _ = _run(checker, tmp_path, [(body, isize, crc, None) for _, _, body, isize, crc in cases])
    for (want, label, *_), (status, equal) in zip(cases, got):
        assert (status, equal) == (want, 0), label


def test_core_gives_the_judges_verdict_on_corrupted_bodies(checker, tmp_path):
    """Each of 2 400 corruptions ends as the judge says -- the bytes where it takes the body, an error status where it does not --
    and never in a sanitizer report (which would end the program with a non-zero status)."""
    cases = list(bu.corruptions(2400))
    verdicts = [bu.body_verdict(body, isize, crc) for _, body, isize, crc in cases]
    got, _ = _run(checker, tmp_path, [(body, isize, crc, v) for (_, body, isize, crc), v in zip(cases, verdicts)])
    for (label, *_), verdict, (status, equal) in zip(cases, verdicts, got):
        assert (status == 0, equal == 1) == (verdict is not None, verdict is not None), label
    assert sum(v is None for v in verdicts) > 1000          # (the corruptions do corrupt)
    assert {s for s, _ in got} >= {0, 4, 8, 9, 11}


def test_crc32_of_spans_combines_to_zlibs(checker, tmp_path):
    """The remainder of a span and the shift by the bytes behind it, combined over splits into 1, 2, 3 and 64 spans of unequal
    length, empty ones included, and over the shares the kernel's 64 lanes take; the expected values are zlib.crc32's."""
    rng = np.random.default_rng(11)
    buffer = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    splits = [(n, ()) for n in (0, 1, 7, 15, 17, 63, 64, 65, 255, 256, 257, 1000, 4095, 65280, 65535, 65536)]     # the lanes' shares
    splits += [(65536, (65536,)), (1, (1,)), (0, (0,)), (65536, (1, 65535)), (65536, (65535, 1)), (1000, (0, 1000)), (1000, (1000, 0)),
               (65536, (0, 65536, 0)), (1000, (3, 0, 997)), (777, (333, 111, 333)), (0, (0, 0, 0))]
    for n in (64, 2080, 65536, 50):
        cuts = np.sort(rng.integers(0, n + 1, 63))
        splits.append((n, tuple(int(x) for x in np.diff(np.concatenate([[0], cuts, [n]])))))
    splits.append((2016, tuple(range(64))))
    assert all(sum(s) == n for n, s in splits if s) and {len(s) for _, s in splits} == {0, 1, 2, 3, 64}
    _, lines = _run(checker, tmp_path, [], buffer, splits)
    assert lines == ["crc 1"] * len(splits)
