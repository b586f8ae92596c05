"""What tests/test_inflate_host.py and tests/test_gpu_inflate.py share: the list of zlib streams the decoder of cs_inflate.hip is held
to, seeded corruptions of them, and the file format of tools/inflate_check.cpp.  The judge is zlib.decompress (plus numpy's
transpose for the shuffle filter); everything is compared byte for byte."""
import functools
import struct
import zlib
from typing import NamedTuple

import numpy as np

N_IDS = 1899                       # the chunk length of the reference's 2 kb yeast map


class Case(NamedTuple):
    name: str
    stored: bytes                  # the chunk as the file stores it
    raw: bytes                     # what the gzip filter decodes to (the chunk before the inverse shuffle)
    elem_bytes: int
    chunk_elems: int
    filters: tuple                 # HDF5 filter ids in pipeline order
    mask: int                      # the chunk's filter mask
    values: np.ndarray             # the chunk's elements as the column holds them


def shuffle(values):
    """HDF5's shuffle filter: byte plane p of element e at p * n + e."""
    values = np.ascontiguousarray(values)
    return values.view(np.uint8).reshape(values.size, values.dtype.itemsize).T.tobytes()


def unshuffle(raw, dtype):
    dtype = np.dtype(dtype)
    return np.frombuffer(np.frombuffer(raw, dtype=np.uint8).reshape(dtype.itemsize, -1).T.tobytes(), dtype=dtype)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if flush_at is None:
        return co.compress(raw) + co.flush()
    return co.compress(raw[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[flush_at:]) + co.flush()


class _Bits:
    """Deflate's bit order: fields from the least significant bit of each byte, Huffman codes most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def field(self, value, width):
        self.acc |= value << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, width):
        for i in reversed(range(width)):
            self.field((value >> i) & 1, 1)

    def done(self):
        if self.n:
            self.field(0, 8 - self.n)
        return bytes(self.out)


def far_match_stream(head):
    """A stream zlib never emits: a stored block of the 32 768 bytes `head`, then a fixed-Huffman block holding one match of length
    258 at distance 32 768.  Returns (stream, decoded)."""
    assert len(head) == 32768
    raw = head + head[:258]
    b = _Bits()
    b.field(0x78, 8)
    b.field(0x01, 8)
    b.field(0, 1)                   # not the last block
    b.field(0, 2)                   # stored
    b.field(0, 5)                   # to the byte boundary
    b.field(0x8000, 16)
    b.field(0x7FFF, 16)
    b.out += head
    b.field(1, 1)                   # the last block
    b.field(1, 2)                   # fixed codes
    b.code(0b11000000 + (285 - 280), 8)          # length symbol 285: 258, no extra bits
    b.code(29, 5)                   # distance symbol 29: 24 577 + 13 extra bits
    b.field(32768 - 24577, 13)
    b.code(0, 7)                    # end of block
    return b.done() + struct.pack(">I", zlib.adler32(raw)), raw


def _case(name, values, stored=None, *, filters=(2, 1), mask=0, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, raw=None):
    values = np.ascontiguousarray(values)
    if raw is None:
        raw = shuffle(values) if 2 in filters and not mask & (1 << filters.index(2)) else values.tobytes()
    if stored is None:
        stored = deflate(raw, level, strategy, flush_at)
    return Case(name, stored, raw, values.dtype.itemsize, values.size, tuple(filters), mask, values)


@functools.lru_cache(maxsize=None)
def stream_cases():
    """The stream list: every case is one chunk of a dataset of its own geometry."""
    rng = np.random.default_rng(20261019)
    ids = np.sort(rng.integers(0, 6_000_000, N_IDS)).astype(np.int64)
    ids32 = ids.astype(np.int32)
    noise = rng.integers(0, 256, 32768, dtype=np.uint8)
    period = rng.integers(0, 256, 32506, dtype=np.uint8)
    big = rng.integers(0, 256, 65536, dtype=np.uint8)
    far, far_raw = far_match_stream(noise.tobytes())
    cases = [_case(f"ids level {lv}", ids, level=lv) for lv in (1, 6, 9)]
    cases += [
        _case("ids level 0 (stored)", ids, level=0),
        _case("ids Z_FIXED", ids, strategy=zlib.Z_FIXED),
        _case("ids Z_HUFFMAN_ONLY", ids, strategy=zlib.Z_HUFFMAN_ONLY),
        _case("ids Z_RLE", ids, strategy=zlib.Z_RLE),
        _case("ids Z_FULL_FLUSH in the middle", ids, flush_at=7001),
        _case("32 768 random bytes", noise, filters=(1,)),
        _case("65 536 zero bytes", np.zeros(65536, dtype=np.uint8), filters=(1,)),
        _case("65 012 bytes of period 32 506", np.concatenate([period, period]), filters=(1,)),
        _case("far match, hand-assembled", np.frombuffer(far_raw, dtype=np.uint8), far, filters=(1,)),
        _case("64 KiB at level 0", big, filters=(1,), level=0),
        _case("int32 column", ids32),
        _case("no shuffle filter", ids, filters=(1,)),
        _case("mask skips gzip", ids, shuffle(ids), mask=2),
        _case("mask skips shuffle", ids, mask=1),
    ]
    fl = _case("Fletcher-32 tail", ids, filters=(2, 1, 3))
    cases.append(fl._replace(stored=fl.stored + b"\xde\xad\xbe\xef"))
    return tuple(cases)


def check_cases_against_zlib():
    """The list is what it says: zlib decodes every gzip stream to `raw`, and `raw` through the filters gives `values`."""
    for c in stream_cases():
        data = c.stored
        for k, fid in reversed(list(enumerate(c.filters))):
            if c.mask & (1 << k):
                continue
            if fid == 3:
                data = data[:-4]
            elif fid == 1:
                data = zlib.decompress(data)
                assert data == c.raw, c.name
            elif fid == 2:
                data = unshuffle(data, c.values.dtype).tobytes()
        assert data == c.values.tobytes(), c.name


def gzip_streams():
    """(name, zlib stream, decoded bytes) of every case that holds one."""
    out = []
    for c in stream_cases():
        if 1 in c.filters and not c.mask & (1 << c.filters.index(1)):
            out.append((c.name, c.stored[:-4] if 3 in c.filters else c.stored, c.raw))
    return out


def zlib_verdict(stream):
    """zlib.decompress's own answer: the bytes, or None where it raises."""
    try:
        return zlib.decompress(stream)
    except zlib.error:
        return None


def corruptions(n, seed=7):
    """n seeded corruptions of the valid streams: single byte flips (half of them in the first 64 bytes, where the headers and the
    code sets are), truncations and appended bytes.  Yields (label, stream, cap): cap is the decoded size of the valid stream."""
    rng = np.random.default_rng(seed)
    streams = gzip_streams()
    for i in range(n):
        name, stream, raw = streams[i % len(streams)]
        kind = (i // len(streams)) % 4
        data = bytearray(stream)
        if kind in (0, 1):
            at = int(rng.integers(0, min(len(data), 64) if kind == 0 else len(data)))
            data[at] ^= int(rng.integers(1, 256))
            label = f"{name}: byte {at} flipped"
        elif kind == 2:
            keep = int(rng.integers(0, len(data)))
            del data[keep:]
            label = f"{name}: cut to {keep} bytes"
        else:
            extra = rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()
            data += extra
            label = f"{name}: {len(extra)} bytes appended"
        yield label, bytes(data), len(raw)


def write_stream_file(path, records):
    """tools/inflate_check.cpp's input: records of (stream, cap, expected bytes or None)."""
    with open(path, "wb") as f:
        f.write(b"CSIF" + struct.pack("<I", len(records)))
        for stream, cap, expected in records:
            f.write(struct.pack("<IIi", len(stream), cap, -1 if expected is None else len(expected)))
            f.write(stream)
            if expected:
                f.write(expected)


# One corrupt stream per failure the decoder names (cs_inflate_core.h csz::Status), each derived from a valid stream of the 1899 int64
# ids, shuffled (cap 15 192 bytes).  tests/test_inflate_host.py runs every one of them through the sanitizer build first.
def failure_streams():
    ids = stream_cases()[1]
    raw, good = ids.raw, ids.stored
    cap = len(raw)
    stored0 = stream_cases()[3].stored
    out = {}
    out[1, "bad header: method 7"] = bytes([0x77, 0x01]) + good[2:]
    out[1, "bad header: check bits"] = bytes([0x78, 0x9D]) + good[2:]
    out[2, "reserved block type"] = good[:2] + bytes([good[2] | 0x06]) + good[3:]
    bad_len = bytearray(stored0)
    bad_len[5] ^= 0x10                                   # NLEN of the first stored block
    out[3, "stored block: LEN / ~LEN"] = bytes(bad_len)
    # a dynamic block whose code-length code is over-subscribed: HLIT 0, HDIST 0, HCLEN 15 (all 19 lengths), every length 1
    b = _Bits()
    b.field(0x78, 8), b.field(0x9C, 8), b.field(1, 1), b.field(2, 2), b.field(0, 5), b.field(0, 5), b.field(15, 4)
    for _ in range(19):
        b.field(1, 3)
    out[4, "over-subscribed code-length code"] = b.done() + bytes(8)
    # a fixed block that opens with a match: nothing to reach back to
    b = _Bits()
    b.field(0x78, 8), b.field(0x9C, 8), b.field(1, 1), b.field(1, 2)
    b.code(0b0000001, 7), b.code(0, 5), b.code(0, 7)                 # length 3, distance 1, end of block
    out[5, "distance before the start"] = b.done() + bytes(4)
    out[6, "too long"] = deflate(raw + b"\0")
    out[7, "too short"] = deflate(raw[:-1])
    out[8, "input exhausted: cut in the body"] = good[:len(good) // 2]
    out[8, "input exhausted: cut in the trailer"] = good[:-2]
    flipped = bytearray(good)
    flipped[-1] ^= 1
    out[9, "Adler-32 mismatch"] = bytes(flipped)
    literal = bytearray(stored0)
    literal[100] ^= 0x40                                 # a byte of a stored block's payload
    out[9, "Adler-32 mismatch: payload byte"] = bytes(literal)
    return [(status, label, stream, cap) for (status, label), stream in out.items()]
