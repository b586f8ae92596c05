"""What tests/test_bgzf_host.py and tests/test_gpu_bgzf.py share: a BGZF writer on Python's zlib, the list of member bodies the decoder of
cs_bgzf_inflate is held to (the zlib streams of tests/inflate_util.py rewrapped), corrupt bodies, and the file format of
tools/bgzf_check.cpp.  The judge of a file is gzip.decompress; the judge of one body is body_verdict."""
import functools
import struct
import zlib

import numpy as np

from tests import inflate_util as iu

END_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_BLOCK = 65536                   # the most text a member holds
BGZIP_BLOCK = 65280                 # what bgzip puts into one


def frame(body, raw_len, crc, before=(), after=()):
    """A member around the raw deflate `body`: the gzip header with FEXTRA, the subfields `before` ((si1, si2, data) each), the BC
    subfield, the subfields `after`, the body, CRC-32 and ISIZE."""
    sub = lambda si1, si2, data: bytes([si1, si2]) + struct.pack("<H", len(data)) + data          # noqa: E731
    xlen = sum(4 + len(d) for _, _, d in before) + 6 + sum(4 + len(d) for _, _, d in after)
    bsize = 12 + xlen + len(body) + 8 - 1
    assert bsize < 65536, "the member does not fit a BGZF block"
    extra = b"".join(sub(*s) for s in before) + sub(66, 67, struct.pack("<H", bsize)) + b"".join(sub(*s) for s in after)
    return b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", xlen) + extra + body + struct.pack("<II", crc, raw_len)


def deflate_raw(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return co.compress(raw) + co.flush()


def block(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, before=(), after=()):
    """One member holding `raw`."""
    return frame(deflate_raw(raw, level, strategy), len(raw), zlib.crc32(raw), before, after)


def bgzf_file(text, block_bytes=BGZIP_BLOCK, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, end_marker=True):
    """`text` cut into members of block_bytes, plus the end marker."""
    parts = [block(text[at:at + block_bytes], level, strategy) for at in range(0, len(text), block_bytes)]
    return b"".join(parts) + (block(b"") if end_marker else b"")


def body_of(member):
    """(body, isize, crc) of one member written by frame."""
    xlen, = struct.unpack_from("<H", member, 10)
    crc, isize = struct.unpack_from("<II", member, len(member) - 8)
    return member[12 + xlen:len(member) - 8], isize, crc


def body_verdict(body, isize, crc):
    """The judge of one body: its bytes, or None where it is not a whole raw deflate stream of isize bytes with that CRC-32 that fills
    the body."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(body)
    except zlib.error:
        return None
    ok = d.eof and not d.unused_data and len(out) == isize and zlib.crc32(out) == crc
    return out if ok else None


@functools.lru_cache(maxsize=None)
def bodies():
    """(name, body, raw) of every stream of inflate_util.gzip_streams() that fits a member: the zlib stream without its 2-byte header
    and its Adler-32."""
    out = []
    for name, stream, raw in iu.gzip_streams():
        body = stream[2:-4]
        if 12 + 6 + len(body) + 8 <= 65536:
            out.append((name, body, raw))
    return tuple(out)


def corruptions(n, seed=7):
    """inflate_util.corruptions rewrapped: (label, body, isize, crc) with isize and crc those of the valid stream.  A corruption that
    leaves less than the zlib frame is a body without bytes."""
    by_name = {name: zlib.crc32(raw) for name, _, raw in iu.gzip_streams()}
    for label, stream, cap in iu.corruptions(n, seed):
        name = label.split(": ")[0]
        yield label, stream[2:-4] if len(stream) > 6 else b"", cap, by_name[name]


def pairs_text_block(n=MAX_BLOCK, seed=3):
    """n bytes of pairs text: lines of a read id, two chromosomes, two positions and two strands."""
    rng = np.random.default_rng(seed)
    lines = []
    size = 0
    k = 0
    while size < n:
        c1, c2 = rng.integers(1, 17, 2)
        p1, p2 = rng.integers(1, 1_500_000, 2)
        line = f"r{k}\tchr{c1}\t{p1}\tchr{c2}\t{p2}\t{'+-'[k & 1]}\t{'+-'[(k >> 1) & 1]}\n".encode()
        lines.append(line)
        size += len(line)
        k += 1
    return b"".join(lines)[:n]


def last_newline(raw):
    return raw.rfind(b"\n")


# One corrupt body per failure the member decoder names (cs_inflate_core.h csz::Status; 1, a zlib header, and 10, a .cool's chunk, are
# not a member's), each as (status, label, body, isize, crc).  tests/test_bgzf_host.py runs every one through the sanitizer build first.
def failure_bodies():
    raw = iu.stream_cases()[1].raw
    good = deflate_raw(raw)
    crc, n = zlib.crc32(raw), len(raw)
    stored = deflate_raw(raw, level=0)
    out = []
    for status, label, stream, cap in iu.failure_streams():
        if status in (2, 3, 4, 5):
            out.append((status, label, stream[2:-4] if status in (2, 3) else stream[2:], cap, crc))
    out.append((6, "too long", deflate_raw(raw + b"\0"), n, crc))
    out.append((7, "too short", deflate_raw(raw[:-1]), n, crc))
    out.append((8, "input exhausted: cut in the body", good[:len(good) // 2], n, crc))
    out.append((8, "input exhausted: no bytes", b"", n, crc))
    out.append((9, "CRC-32 mismatch", good, n, crc ^ 1))
    payload = bytearray(stored)
    payload[100] ^= 0x40
    out.append((9, "CRC-32 mismatch: payload byte", bytes(payload), n, crc))
    out.append((11, "one byte behind the stream", good + b"\0", n, crc))
    out.append((11, "the trailer taken for body", good + struct.pack("<II", crc, n), n, crc))
    return out


def write_records(path, records, buffer=b"", splits=()):
    """tools/bgzf_check.cpp's input: records of (body, isize, crc, expected bytes or None), then the buffer and the splits of its
    prefixes, (n, spans) each -- spans: a list of lengths that add up to n, or () for the 64 lanes' shares."""
    with open(path, "wb") as f:
        f.write(b"CSBZ" + struct.pack("<I", len(records)))
        for body, isize, crc, expected in records:
            f.write(struct.pack("<IIIi", len(body), isize, crc, -1 if expected is None else len(expected)))
            f.write(body)
            if expected:
                f.write(expected)
        f.write(struct.pack("<I", len(buffer)) + buffer + struct.pack("<I", len(splits)))
        for n, spans in splits:
            f.write(struct.pack("<III", n, zlib.crc32(buffer[:n]), len(spans)) + struct.pack(f"<{len(spans)}I", *spans))
