"""Binning of read pairs into a pixel table on the device: cs_pairs_count / cs_pairs_fill (chromosight_amd/csrc/cs_pairs.hip).

The reference runs on a finished .cool and leaves every step before it to cooler.  The rules below restate what
`cooler cload pairs` writes; cooler is not part of this stack, so nothing here was captured from it:

- the geometry comes from `chromsizes` (ordered name -> length in bp, every length >= 1) and `binsize` (>= 1): chromosome c gets
  ceil(len_c / binsize) bins, bin_start = k * binsize, bin_end = min((k + 1) * binsize, len_c) -- the last bin of a chromosome may
  be short -- and chrom_offset is the prefix sum of the bin counts.  That is what a .cool of that bin size stores, so the result
  merges with such a file's table (merge.check_compatible);
- a pair is (chrom1 id, pos1, chrom2 id, pos2): ids are int32 indices into `chromsizes`, -1 for a chromosome that is not in it;
  positions are int64, 1-based as the pairs format defines them, or taken as they are with zero_based=True;
- a pair with an id of -1 on either side is dropped, and the number dropped is reported;
- a known chromosome with a zero-based position outside [0, len_c), or an id >= n_chrom or < -1, refuses the whole call with
  ValueError naming the number of offending pairs and the first one's index in the chunk; no table is returned and nothing
  resident is modified.  A side that refuses counts before a side that drops: (-1, x, 0, len_0 + 5) is refused;
- the genome bin of a position is chrom_offset[c] + pos0 // binsize; a pair whose bin1 > bin2 is reflected, so every stored pixel
  lies on or above the diagonal (`upper` is True);
- the table holds one pixel per distinct (bin1, bin2), its count the number of pairs there; rows are sorted by column, without
  duplicates or zero entries;
- the counts are float32 when every count is below 2^24, else float64 (the constructor's rule, the one cs_merge_count reports);
- sums are integers and exact: the table is bitwise the same for every order of the pairs, every split into chunks, and every
  launch shape, context and device (integer atomics only, no float atomics);
- fewer than 2^31 - 1 pairs per chunk, fewer than 2^31 - 1 pixels in any table, fewer than 2^31 genome bins (ValueError beyond);
- no weights are carried: the result is a table without weights, as a merged or coarsened one is.

The text of a .pairs file becomes such columns on the device too (cs_pairs_text_count / cs_pairs_text_parse,
chromosight_amd/csrc/cs_pairs_text.hip): parse_pairs_text for one piece of body text, pairs_file_device for a file, which is read
in pieces cut at a line end (text_pieces), each parsed, binned and merged like a chunk above.  The device takes a strict subset of
what io.PairsFile takes (include/chromosight_hip.h states it) and flags every other line, which then goes to the host reader."""
import ctypes as C
import zlib
from typing import NamedTuple

import numpy as np

from ._lib import CsPairsTextFormat, CsPairsTextReport, DeviceBuffer, get_device, load_library, np_dtype_of, plain_csr

MAX_CHUNK_PAIRS = 2 ** 31 - 2
PIECE_BYTES = 1 << 27           # the text of a file that goes to the device at a time (pairs_file_device)
FLAG_REASONS = {1: "an empty line", 2: "too few fields", 3: "too many fields", 4: "an empty name or position",
                5: "a position that is not 1 to 18 digits", 6: "a carriage return that does not end the line", 7: "a NUL byte",
                8: "a byte that is not ASCII", 9: "a line longer than the device takes"}


def __getattr__(name):
    if name == "BLOCK_PAIRS":                   # the sorted pairs one workgroup of the run-length pass covers; read from the
        return int(load_library().cs_pairs_block_pairs())           # library when asked for, so that importing needs none
    if name == "TEXT_TILE_BYTES":               # the text one workgroup of the parser covers
        return int(load_library().cs_pairs_text_tile_bytes())
    if name == "MAX_LINE_BYTES":                # the longest line the parser takes, without its terminator
        return int(load_library().cs_pairs_text_max_line_bytes())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class Geometry(NamedTuple):
    """The bins of a genome: what bin_geometry returns."""
    offsets: np.ndarray         # n_chrom + 1 chromosome offsets, in bins
    bin_start: np.ndarray       # per bin, bp within its chromosome
    bin_end: np.ndarray
    names: list
    lengths: np.ndarray         # per chromosome, bp
    binsize: int


def bin_geometry(chromsizes, binsize):
    """The bins of `chromsizes` (a mapping name -> length in bp, or a sequence of (name, length), in genome order) at `binsize` bp:
    a Geometry of offsets, bin_start, bin_end and names (and the lengths and the bin size it was built from).  ValueError for a
    length below 1, a bin size below 1, a name given twice and a genome of 2^31 bins or more."""
    if isinstance(binsize, bool) or int(binsize) != binsize or int(binsize) < 1:
        raise ValueError(f"the bin size must be an integer of at least 1 bp, got {binsize!r}")
    binsize = int(binsize)
    items = list(chromsizes.items()) if hasattr(chromsizes, "items") else [tuple(x) for x in chromsizes]
    names = [str(name) for name, _ in items]
    if len(set(names)) != len(names):
        raise ValueError("a chromosome name is given twice")
    lengths = np.asarray([int(length) for _, length in items], dtype=np.int64).reshape(-1)
    if np.any(lengths < 1):
        raise ValueError(f"every chromosome must be at least 1 bp long, got {lengths[lengths < 1][0]} for {names[int(np.argmax(lengths < 1))]}")
    n_bins = -(-lengths // binsize)
    offsets = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int64)
    if int(offsets[-1]) >= 2 ** 31:
        raise ValueError(f"a genome of {int(offsets[-1])} bins: 2^31 or more are not supported")
    local = np.arange(int(offsets[-1]), dtype=np.int64) - np.repeat(offsets[:-1], n_bins)
    start = local * binsize
    end = np.minimum(start + binsize, np.repeat(lengths, n_bins))
    return Geometry(offsets, start, end, names, lengths, binsize)


def check_chunk(chrom1, pos1, chrom2, pos2):
    """The host-side refusals of a chunk that need no pixel (ValueError): columns that are not one-dimensional or of different
    lengths, ids or positions that are not integers (or ids that do not fit int32, positions that do not fit int64), more than
    2^31 - 2 pairs.  Returns the columns as contiguous int32 / int64 / int32 / int64 arrays (no copy where they already are)."""
    cols = [np.asarray(x) for x in (chrom1, pos1, chrom2, pos2)]
    labels = ("chrom1", "pos1", "chrom2", "pos2")
    for label, col in zip(labels, cols):
        if col.ndim != 1:
            raise ValueError(f"{label} must be one-dimensional, got shape {col.shape}")
        if col.dtype.kind not in "iu":
            raise ValueError(f"{label} must hold integers, got {col.dtype}")
    n = cols[0].size
    if any(col.size != n for col in cols):
        raise ValueError("the columns of a chunk differ in length: " + ", ".join(f"{lb} {c.size}" for lb, c in zip(labels, cols)))
    if n > MAX_CHUNK_PAIRS:
        raise ValueError(f"a chunk of {n} pairs: more than 2^31 - 2 are not binned in one call")
    out = []
    for label, col, dtype in zip(labels, cols, (np.int32, np.int64, np.int32, np.int64)):
        info = np.iinfo(dtype)
        if n and col.dtype != dtype and (int(col.max()) > info.max or int(col.min()) < info.min):
            raise ValueError(f"{label} holds values outside {np.dtype(dtype).name}")
        out.append(np.ascontiguousarray(col, dtype=dtype))
    return tuple(out)


def pairs_csr(dev, geometry, chrom1, pos1, chrom2, pos2, zero_based=False):
    """Bin one chunk of pairs on `dev`.  Returns a dict like merge.merge_csr: `indptr` (bins + 1), `indices`, `data` (device buffers
    of exactly `nnz` pixels; one entry when there is none), `nnz`, `val_dtype`, plus `dropped`: the pairs with an id of -1.
    ValueError for the refusals of check_chunk, for ids and positions outside the genome and beyond the limits of the kernel."""
    cols = check_chunk(chrom1, pos1, chrom2, pos2)
    n = int(cols[0].size)
    with dev.lock:
        return pairs_csr_resident(dev, geometry, [dev.to_device(a) for a in cols] if n else [None] * 4, n, zero_based=zero_based)


def pairs_csr_resident(dev, geometry, columns, n, zero_based=False):
    """pairs_csr for columns already on the device: `columns` are the four device buffers (int32, int64, int32, int64; the list
    is emptied, so that the columns are released before the pixels are allocated when the caller holds no other reference) and
    `n` the number of pairs in them.  The columns are never written."""
    n = int(n)
    if n > MAX_CHUNK_PAIRS:
        raise ValueError(f"a chunk of {n} pairs: more than 2^31 - 2 are not binned in one call")
    n_bins = int(geometry.offsets[-1])
    offsets = np.ascontiguousarray(geometry.offsets, dtype=np.int64)
    lengths = np.ascontiguousarray(geometry.lengths, dtype=np.int64)
    if lengths.size == 0:
        lengths = np.zeros(1, dtype=np.int64)             # (an address to pass; never read)
    as_i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))          # noqa: E731
    out_nnz, out_dtype, out_dropped = C.c_int64(0), C.c_int32(0), C.c_int64(0)
    with dev.lock:
        try:
            indptr = dev.empty(n_bins + 1, np.int64)
            keys = dev.empty(max(n, 1), np.int64)
            dev._check(dev.lib.cs_pairs_count(dev.ctx, None, *[c.ptr if c is not None else None for c in columns], n, as_i64(offsets),
                                              as_i64(lengths), len(geometry.names), int(geometry.binsize), int(bool(zero_based)),
                                              keys.ptr, indptr.ptr, C.byref(out_nnz), C.byref(out_dtype), C.byref(out_dropped)))
            if isinstance(columns, list):
                columns.clear()
            nnz = int(out_nnz.value)
            val_dtype = np_dtype_of(out_dtype.value)
            indices = dev.empty(max(nnz, 1), np.int32)
            data = dev.empty(max(nnz, 1), val_dtype)
            out = plain_csr(n_bins, nnz, indptr, indices, data, val_dtype)
            dev._check(dev.lib.cs_pairs_fill(dev.ctx, None, keys.ptr, n, C.byref(out)))
        except NotImplementedError as exc:          # CS_ERR_UNSUPPORTED: a limit of the kernel, not a missing feature
            raise ValueError(str(exc)) from None
    return {"indptr": indptr, "indices": indices, "data": data, "nnz": nnz, "val_dtype": val_dtype, "dropped": int(out_dropped.value)}


def _is_single_chunk(chunks):
    return isinstance(chunks, (tuple, list)) and len(chunks) == 4 and all(np.ndim(c) == 1 for c in chunks)


def pairs_device(chunks, chromsizes, binsize, zero_based=False, dev=None):
    """DeviceCool.from_pairs: a DeviceCool over the table of all pairs of `chunks` -- any iterable of (chrom1, pos1, chrom2, pos2)
    tuples of arrays (io.read_pairs gives one), or one such tuple -- over the bins of bin_geometry(chromsizes, binsize).  Every
    chunk is binned into a table of its own, which is merged into the running table at once (merge.merge_csr: exact, so the result
    does not depend on the split into chunks), long before one merge call's 64 sources pile up; a chunk's buffers and the previous
    running table are released once merged.  The peak in HBM is one chunk's columns (24 bytes per pair) + its keys (8 bytes per
    pair) + the sort's scratch (the unsorted keys and the radix sort's own, some 8 bytes per pair each) + the running table, and,
    after the columns and scratch are gone, the chunk's table + the running table + the merged result.
    The result has no weights, upper = True, the geometry's names, bin_start and bin_end, and `.dropped`: the pairs dropped for an
    id of -1, summed over the chunks.  ValueError as pairs_csr; the chunks before a refused one have been consumed."""
    dev = dev or get_device()
    geo = chromsizes if isinstance(chromsizes, Geometry) and int(binsize) == chromsizes.binsize else bin_geometry(chromsizes, binsize)
    running = _RunningTable(geo, dev)
    for chunk in ([chunks] if _is_single_chunk(chunks) else chunks):
        chrom1, pos1, chrom2, pos2 = chunk
        running.add(pairs_csr(dev, geo, chrom1, pos1, chrom2, pos2, zero_based=zero_based))
    return running.result()


class _RunningTable:
    """The table of the chunks binned so far: what pairs_device and pairs_file_device fold their chunks into."""

    def __init__(self, geo, dev):
        self.geo, self.dev, self.dropped = geo, dev, 0
        # the CSR so far, as merge.merge_csr returns it; before the first chunk the table without pixels, as the constructor uploads it
        self.table = {"indptr": dev.zeros(int(geo.offsets[-1]) + 1, np.int64), "indices": dev.empty(0, np.int32),
                      "data": dev.empty(0, np.float32), "nnz": 0, "val_dtype": np.float32}

    def _over(self, table, dropped=None):
        """The DeviceCool of a table of pairs over the geometry: counts that are exact exactly when they are float32 (they are
        non-negative integers), every pixel on or above the diagonal, no weights."""
        from .pipeline import DeviceCool
        geo = self.geo
        return DeviceCool._from_table(self.dev, names=geo.names, offsets=geo.offsets, binsize=geo.binsize, bin_start=geo.bin_start,
                                      bin_end=geo.bin_end, counts_exact=table["val_dtype"] is np.float32, upper=True, weight=None,
                                      dropped=dropped, **table)

    def add(self, res):
        """Merge the table of one chunk (what pairs_csr returns; the caller keeps no reference to its buffers)."""
        from .merge import merge_csr
        self.dropped += res["dropped"]
        part = {key: res[key] for key in ("indptr", "indices", "data", "nnz", "val_dtype")}
        if self.table["nnz"] == 0:
            self.table = part
        elif part["nnz"]:
            self.table = merge_csr([self._over(self.table), self._over(part)])

    def result(self):
        return self._over(self.table, self.dropped)


# ---- the text of a .pairs file ------------------------------------------------------------------------------------------------------
class TextReport(NamedTuple):
    """What the device says about a piece of text: its lines, the index of the first flagged one (-1: none) and why (FLAG_REASONS)."""
    n_lines: int
    first_flagged: int
    reason: int


def parse_pairs_text(dev, text, columns, width, names, timings=None, nbytes=None, offset=0):
    """One piece of the body of a .pairs file parsed on `dev` (cs_pairs_text_count / cs_pairs_text_parse).  text: a bytes-like object,
    uploaded here, or a device buffer of uint8 that holds exactly the text (never written); columns: the 0-based fields of chr1, pos1,
    chr2, pos2; width: the most fields a line may have; names: the chromosome names in genome order.  Returns (columns, n, report):
    the four resident columns as pairs_csr_resident takes them (a list; int32, int64, int32, int64, n entries in line order), the
    number of lines and a TextReport.  With a flagged line the columns hold nothing of use.  ValueError for columns that are not four
    distinct fields below width, a name given twice and a text of 2^31 - 1 lines or more.  timings: a dict that receives the seconds
    of `upload`, `count` and `parse` (each ends in a synchronisation).  nbytes, offset: of a device buffer, the text is the nbytes
    bytes (default: all behind offset) from byte `offset`, a multiple of 16; the rest of the buffer is not read."""
    import time
    encoded = [str(name).encode("utf-8") for name in names]
    offsets = np.zeros(len(encoded) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in encoded], out=offsets[1:])
    gathered = b"".join(encoded)
    fmt = CsPairsTextFormat(*[int(c) for c in columns], int(width), len(encoded), C.cast(C.c_char_p(gathered), C.c_void_p),
                            offsets.ctypes.data_as(C.c_void_p))
    t0 = time.perf_counter()
    with dev.lock:
        if not isinstance(text, DeviceBuffer):
            host = np.frombuffer(text, dtype=np.uint8)
            text = dev.to_device(host) if host.size else dev.empty(0, np.uint8)
        offset = int(offset)
        nbytes = int(text.nbytes) - offset if nbytes is None else int(nbytes)
        if offset < 0 or offset % 16 or nbytes < 0 or offset + nbytes > int(text.nbytes):
            raise ValueError(f"a text of {nbytes} bytes at offset {offset} of a buffer of {int(text.nbytes)}: it must lie inside, at a multiple of 16")
        at = text.ptr + offset
        t1 = time.perf_counter()
        n_lines = C.c_int64(0)
        report = CsPairsTextReport()
        try:
            dev._check(dev.lib.cs_pairs_text_count(dev.ctx, None, at, nbytes, C.byref(n_lines)))
            n = int(n_lines.value)
            t2 = time.perf_counter()
            if n > MAX_CHUNK_PAIRS:
                raise ValueError(f"a text of {n} lines: more than 2^31 - 2 are not parsed in one call")
            cols = [dev.empty(max(n, 1), dtype) for dtype in (np.int32, np.int64, np.int32, np.int64)]
            dev._check(dev.lib.cs_pairs_text_parse(dev.ctx, None, at, nbytes, C.byref(fmt), *[c.ptr for c in cols], n, C.byref(report)))
        except NotImplementedError as exc:          # CS_ERR_UNSUPPORTED: a limit of the kernel, not a missing feature
            raise ValueError(str(exc)) from None
        t3 = time.perf_counter()
    if timings is not None:
        for key, dt in (("upload", t1 - t0), ("count", t2 - t1), ("parse", t3 - t2)):
            timings[key] = timings.get(key, 0.0) + dt
    return cols, n, TextReport(int(report.n_lines), int(report.first_flagged), int(report.reason))


class GzipSource:
    """read(n) over the inflated bytes of a gzip file, member after member (zlib.decompressobj(wbits=31)), never holding more than
    a block of the file and what one read returns.  EOFError for a file that ends inside a member, zlib.error for one that is none."""
    BLOCK = 1 << 20

    def __init__(self, handle):
        self.handle = handle
        self.inflater = zlib.decompressobj(wbits=31)
        self.raw = b""                      # bytes of the file not yet given to the inflater
        self.in_member = False

    def read(self, n):
        out, got = [], 0
        while got < n:
            if self.inflater.eof:
                self.raw = self.inflater.unused_data.lstrip(b"\0")        # (zero padding between members, as gzip allows)
                self.inflater = zlib.decompressobj(wbits=31)
                self.in_member = False
            if not self.raw:
                self.raw = self.handle.read(self.BLOCK)
                if not self.raw:
                    if not self.in_member:
                        break
                    data = self.inflater.decompress(b"", n - got)          # (output the inflater held back at the last limit)
                    if not data and not self.inflater.eof:
                        raise EOFError("Compressed file ended before the end-of-stream marker was reached")
                    out.append(data)
                    got += len(data)
                    continue
                if not self.in_member:
                    self.raw = self.raw.lstrip(b"\0")
                    if not self.raw:
                        continue
            self.in_member = True
            data = self.inflater.decompress(self.raw, n - got)
            self.raw = self.inflater.unconsumed_tail
            if data:
                out.append(data)
                got += len(data)
        return b"".join(out)


def text_pieces(read, piece_bytes, carry=b""):
    """The text that read(n) -> bytes (b"" at its end) delivers, behind `carry`, as pieces that end at a line end: about piece_bytes
    are read at a time and cut at their last '\n' (bytes.rfind), and the rest is carried into the next piece, of which that much
    less is read; a carry without a line end as long as a piece grows by whole reads until it has one or the text ends.  The last
    piece is whatever is left, with or without a final '\n'.  The pieces, joined, are the text; none is empty.  A piece is bytes-like:
    where it is the head of one read it is a memoryview of it, not a copy."""
    piece_bytes = int(piece_bytes)
    if piece_bytes < 1:
        raise ValueError(f"piece_bytes must be at least 1, got {piece_bytes}")
    if carry:                                       # served first, in reads like any other
        source, pending = read, [carry]

        def read(n):
            if pending[0]:
                out, pending[0] = pending[0][:n], pending[0][n:]
                return out
            return source(n)
    held, size = [], 0                              # bytes without a line end, in front of the next block
    block = read(piece_bytes)
    while block:
        cut = block.rfind(b"\n")
        if cut < 0:
            held.append(block)
            size += len(block)
        else:
            head = block if cut + 1 == len(block) else memoryview(block)[:cut + 1]
            yield b"".join(held + [head]) if held else head
            rest = block[cut + 1:]
            held, size = ([rest], len(rest)) if rest else ([], 0)
        block = read(piece_bytes - size if size < piece_bytes else piece_bytes)
    if held:
        yield b"".join(held)


def _skip_header(read, n_lines, path):
    """Reads past the first n_lines lines of a file (its header); returns the bytes read beyond them.  DevicePairsRefused for a
    header line with a carriage return that does not end it: the host reader counts lines in another way then."""
    from .pipeline import DevicePairsRefused
    buf, at = b"", 0
    for k in range(n_lines):
        while True:
            end = buf.find(b"\n", at)
            if end >= 0:
                break
            block = read(1 << 16)
            if not block:
                return b""                          # (the file ends in its header)
            buf = buf[at:] + block
            at = 0
        if b"\r" in buf[at:end - 1]:
            raise DevicePairsRefused(f"{path}, line {k + 1}: {FLAG_REASONS[6]}")
        at = end + 1
    return buf[at:]


class BgzfBlock(NamedTuple):
    """One member of a BGZF file: where it starts, where its raw deflate body lies, and the size of its text."""
    file_offset: int
    body_offset: int
    body_bytes: int
    isize: int


BGZF_MAX_ISIZE = 65536


def bgzf_blocks(buf):
    """The members of a bgzip-compressed file, one BgzfBlock after the other, walked over `buf`: the file's bytes as anything with the
    buffer protocol (a mapping of the file; only the header and the trailer of a member are read).  pipeline.DeviceInflateRefused (a
    ValueError) at the first thing that is not a qualifying member directly behind the one before it: a member has the magic 1f 8b,
    method 8 and the flags 4 (an extra field and nothing else), exactly one subfield 'BC' of 2 bytes among the subfields that fill its
    extra field (it holds the member's size - 1), ends inside the file and holds at most 65 536 bytes of text.  The 28-byte end marker
    is a member without text; a file without it, and a file without bytes, is walked all the same.  Plain gzip output, a member with a
    name, a comment or a header CRC, zero padding between members and trailing bytes are refused."""
    import struct
    from .pipeline import DeviceInflateRefused
    view = memoryview(buf)
    try:
        size, at, k = view.nbytes, 0, 0
        while at < size:
            where = f"member {k} at byte {at}"
            if size - at < 12:
                raise DeviceInflateRefused(f"{where}: {size - at} bytes are no gzip header")
            magic, method, flags, xlen = struct.unpack_from("<HBB6xH", view, at)
            if magic != 0x8B1F or method != 8:
                raise DeviceInflateRefused(f"{where}: not a gzip member")
            if flags != 4:
                raise DeviceInflateRefused(f"{where}: gzip flags {flags:#04x}, a BGZF member has an extra field and nothing else (0x04)")
            if at + 12 + xlen > size:
                raise DeviceInflateRefused(f"{where}: the extra field leaves the file")
            sub, end, bsize = at + 12, at + 12 + xlen, None
            while sub < end:
                if end - sub < 4:
                    raise DeviceInflateRefused(f"{where}: the subfields do not fill the extra field")
                si1, si2, slen = struct.unpack_from("<BBH", view, sub)
                if sub + 4 + slen > end:
                    raise DeviceInflateRefused(f"{where}: a subfield leaves the extra field")
                if (si1, si2) == (66, 67):
                    if slen != 2 or bsize is not None:
                        raise DeviceInflateRefused(f"{where}: more than one 'BC' subfield, or one that is not 2 bytes")
                    bsize, = struct.unpack_from("<H", view, sub + 4)
                sub += 4 + slen
            if bsize is None:
                raise DeviceInflateRefused(f"{where}: no 'BC' subfield: gzip, not bgzip")
            total = bsize + 1
            if total < 12 + xlen + 8:
                raise DeviceInflateRefused(f"{where}: a member of {total} bytes does not hold its own header and trailer")
            if at + total > size:
                raise DeviceInflateRefused(f"{where}: the member ({total} bytes) leaves the file: truncated")
            isize, = struct.unpack_from("<I", view, at + total - 4)
            if isize > BGZF_MAX_ISIZE:
                raise DeviceInflateRefused(f"{where}: {isize} bytes of text, a BGZF member holds at most {BGZF_MAX_ISIZE}")
            yield BgzfBlock(at, at + 12 + xlen, total - 12 - xlen - 8, isize)
            at += total
            k += 1
    finally:
        view.release()


def _corrupt_member(path, k, block, status):
    """engine.CorruptChunks for member k of a file; .block and .file_offset name it, .status holds its code (an index into
    engine.BGZF_STATUS; -1 for status None: a member of the header, which the host's zlib inflates and did not take)."""
    from .engine import BGZF_STATUS, CorruptChunks
    if status is None:
        why, status = "the host's zlib does not take it", -1
    else:
        why = f"{BGZF_STATUS[status] if 0 <= status < len(BGZF_STATUS) else 'unknown status'} (status {status})"
    exc = CorruptChunks(f"{path}: BGZF member {k} at byte {block.file_offset} does not decode: {why}", np.asarray([status]))
    exc.block, exc.file_offset = k, block.file_offset
    return exc


def _device_inflated_pieces(pf, mm, piece_bytes, dev, timings):
    """The body of a bgzip-compressed .pairs.gz (pf: its io.PairsFile; mm: a mapping of the file) as text on the device, piece by piece:
    yields (buffer, start, nbytes) -- a DeviceBuffer of uint8 and the span of it to parse, which starts at a multiple of 16 and ends
    behind a line end, or at the end of the file.  The header's members are inflated on the host (zlib, raw deflate) to find the member
    and the offset in it where the body starts; from there a piece is as many members as keep carry + their text within piece_bytes,
    one at the least.  Their bytes go to the device as they are in the file and are inflated there (cs_bgzf_inflate) behind the carry:
    the text behind the last '\\n' of the piece before (fetched from the device and uploaded again: a fraction of a line as a rule; a
    piece without a line end whole).  In the first piece the member is placed so that the body starts at a multiple of 16."""
    import time
    from . import engine

    def clocked(key, t0):
        if timings is not None:
            timings[key] = timings.get(key, 0.0) + time.perf_counter() - t0

    t0 = time.perf_counter()
    blocks = list(bgzf_blocks(mm))
    clocked("read", t0)
    # the header: member after member through the host's zlib until its lines are read
    state = {"next": 0}

    def read_header(_n):
        while state["next"] < len(blocks):
            k = state["next"]
            b = blocks[k]
            state["next"] += 1
            inflater = zlib.decompressobj(-15)
            end = b.body_offset + b.body_bytes
            try:
                text = inflater.decompress(mm[b.body_offset:end])
                whole = inflater.eof and not inflater.unused_data and len(text) == b.isize and \
                    zlib.crc32(text) == int.from_bytes(mm[end:end + 4], "little")
            except zlib.error:
                whole = False
            if not whole:
                raise _corrupt_member(pf.path, k, b, None)
            if text:
                return text
        return b""

    t0 = time.perf_counter()
    rest = _skip_header(read_header, pf.header_lines, pf.path)
    clocked("read", t0)
    k = state["next"]                               # the next member to inflate, and where in it the body starts
    skip = 0
    if rest:
        k -= 1
        skip = blocks[k].isize - len(rest)
    del rest
    carry = np.empty(0, dtype=np.uint8)
    while k < len(blocks) or carry.size:
        t0 = time.perf_counter()
        first = k
        room = int(carry.size) - skip               # (the header's part of the first member is no text of the piece)
        while k < len(blocks) and (k == first or room + blocks[k].isize <= piece_bytes):
            room += blocks[k].isize
            k += 1
        mine = blocks[first:k]
        pad = -skip % 16
        start = pad + skip
        out_offsets = np.cumsum([pad + int(carry.size)] + [b.isize for b in mine], dtype=np.int64)
        end = int(out_offsets[-1])
        clocked("cut", t0)
        with dev.lock:
            t0 = time.perf_counter()
            text = dev.empty(max(end, 1), np.uint8)
            if carry.size:
                dev._check(dev.lib.cs_memcpy_h2d(dev.ctx, text.ptr, carry.ctypes.data, int(carry.size), None))
            last = -1
            if mine:
                lo, hi = mine[0].file_offset, mine[-1].body_offset + mine[-1].body_bytes + 8
                span = np.frombuffer(mm, dtype=np.uint8, count=hi - lo, offset=lo)
                try:
                    d_file = dev.to_device(span)
                finally:
                    del span                        # (no view of the mapping outlives this block: it could not be closed)
                clocked("upload", t0)
                t0 = time.perf_counter()
                try:
                    _, last = engine.run_bgzf_inflate(dev, d_file, hi - lo, [b.body_offset - lo for b in mine], [b.body_bytes for b in mine],
                                                      out_offsets[:-1], [b.isize for b in mine], text, end)
                except engine.CorruptChunks as exc:
                    bad = int(np.flatnonzero(exc.status)[0])
                    raise _corrupt_member(pf.path, first + bad, mine[bad], int(exc.status[bad])) from None
                del d_file
                clocked("inflate", t0)
            else:
                clocked("upload", t0)
            t0 = time.perf_counter()
            if k >= len(blocks):                    # the last piece: to its end, with or without a final line end
                cut, carry = end, carry[:0]
            else:
                cut = last + 1 if last >= start else start
                carry = np.empty(end - cut, dtype=np.uint8)
                if carry.size:
                    dev._check(dev.lib.cs_memcpy_d2h(dev.ctx, carry.ctypes.data, text.ptr + cut, int(carry.size), None))
            clocked("cut", t0)
        skip = 0
        if cut > start:
            yield text, start, cut - start
        del text


def parsed_pieces(pairs_file, piece_bytes, parse, timings=None, inflate="host", dev=None):
    """The body of a .pairs file, piece by piece (text_pieces; .gz: inflated on the host as a stream, GzipSource), through
    parse(piece, columns, width, names) -> (columns, n, TextReport): yields (columns, n) per piece.  pairs_file: the io.PairsFile of
    the file -- its header pass gives the columns, the width and the number of header lines, which are skipped here.
    pipeline.DevicePairsRefused (a ValueError) for the first flagged line, named by its 1-based number in the file: the header's
    lines + the lines of the pieces before + its index + 1.  timings: a dict that receives the seconds spent in `read` and in
    `cut` (finding the line ends, carrying and joining).
    inflate="device" (a .gz written by bgzip; `dev` is needed): the members of the file are inflated on the device
    (_device_inflated_pieces), the host never sees the body's text, and parse receives (buffer, columns, width, names, start, nbytes)
    -- the text is nbytes bytes of the device buffer from `start`.  pipeline.DeviceInflateRefused for a file that is not BGZF
    throughout, before anything is parsed; engine.CorruptChunks for the first member that does not decode.  timings gains `inflate`."""
    import mmap
    import os
    import time
    from .pipeline import DevicePairsRefused
    pf = pairs_file
    width = max(pf.width, max(pf.columns) + 1)      # (a short first line: the parser flags it, as the host refuses it)
    names = list(pf.chromsizes)
    lines_before = pf.header_lines
    if inflate == "device":
        with open(pf.path, "rb") as handle:
            mm = mmap.mmap(handle.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(handle.fileno()).st_size else b""
            try:
                for text, start, nbytes in _device_inflated_pieces(pf, mm, piece_bytes, dev, timings):
                    cols, n, report = parse(text, pf.columns, width, names, start, nbytes)
                    if report.first_flagged >= 0:
                        raise DevicePairsRefused(f"{pf.path}, line {lines_before + report.first_flagged + 1}: "
                                                 f"{FLAG_REASONS.get(report.reason, f'reason {report.reason}')}")
                    del text
                    yield cols, n
                    lines_before += n
            finally:
                if mm:
                    mm.close()
        return
    with open(pf.path, "rb") as handle:
        read = GzipSource(handle).read if pf.path.endswith(".gz") else handle.read
        if timings is not None:
            raw_read = read

            def read(n):
                t0 = time.perf_counter()
                block = raw_read(n)
                timings["read"] = timings.get("read", 0.0) + time.perf_counter() - t0
                return block
        carry = _skip_header(read, pf.header_lines, pf.path)
        pieces = text_pieces(read, piece_bytes, carry)
        while True:
            t0, read0 = time.perf_counter(), (timings or {}).get("read", 0.0)
            piece = next(pieces, None)
            if timings is not None:
                timings["cut"] = timings.get("cut", 0.0) + time.perf_counter() - t0 - (timings.get("read", 0.0) - read0)
            if piece is None:
                break
            cols, n, report = parse(piece, pf.columns, width, names)
            if report.first_flagged >= 0:
                raise DevicePairsRefused(f"{pf.path}, line {lines_before + report.first_flagged + 1}: "
                                         f"{FLAG_REASONS.get(report.reason, f'reason {report.reason}')}")
            del piece
            yield cols, n
            lines_before += n


def pairs_file_device(pairs_file, binsize, zero_based=False, piece_bytes=None, dev=None, timings=None, inflate="host"):
    """DeviceCool.from_pairs_file on its device route: the table of a .pairs file (pairs_file: its io.PairsFile) whose text is parsed
    on the device.  Every piece of parsed_pieces goes through parse_pairs_text, is binned (pairs_csr_resident) and merged into the
    running table as pairs_device merges a chunk; the binning is exact, so the table is that of pairs_device over the host reader's
    chunks, bit for bit, for every piece_bytes (default PIECE_BYTES).  The peak in HBM is a piece's text + its columns (24 bytes per
    line), and, once the text is released, what pairs_device states for a chunk of that many pairs.  pipeline.DevicePairsRefused
    for a flagged line; ValueError as pairs_csr for pairs outside the genome.  timings: a dict that receives the seconds of `read`,
    `cut`, `upload`, `count`, `parse` and `bin` (binning and merge).  inflate: "host", or "device" for a .gz that bgzip wrote, whose
    members are then inflated in HBM too (parsed_pieces; timings gains `inflate`)."""
    import time
    dev = dev or get_device()
    piece_bytes = PIECE_BYTES if piece_bytes is None else int(piece_bytes)
    if piece_bytes < 1:
        raise ValueError(f"piece_bytes must be at least 1, got {piece_bytes}")
    geo = bin_geometry(pairs_file.chromsizes, binsize)
    running = _RunningTable(geo, dev)

    def parse(piece, columns, width, names, offset=0, nbytes=None):
        return parse_pairs_text(dev, piece, columns, width, names, timings=timings, nbytes=nbytes, offset=offset)

    for cols, n in parsed_pieces(pairs_file, piece_bytes, parse, timings, inflate=inflate, dev=dev):
        t0 = time.perf_counter()
        running.add(pairs_csr_resident(dev, geo, cols, n, zero_based=zero_based))
        if timings is not None:
            timings["bin"] = timings.get("bin", 0.0) + time.perf_counter() - t0
    return running.result()
