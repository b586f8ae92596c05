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
- no weights are carried: the result is a table without weights, as a merged or coarsened one is."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from ._lib import CS_F32, CsCsr, get_device, load_library, np_dtype_code

MAX_CHUNK_PAIRS = 2 ** 31 - 2


def __getattr__(name):
    if name == "BLOCK_PAIRS":                   # the sorted pairs one workgroup of the run-length pass covers; read from the
        return int(load_library().cs_pairs_block_pairs())           # library when asked for, so that importing needs none
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
            val_dtype = np.float32 if out_dtype.value == CS_F32 else np.float64
            indices = dev.empty(max(nnz, 1), np.int32)
            data = dev.empty(max(nnz, 1), val_dtype)
            out = CsCsr(n_bins, n_bins, nnz, indptr.ptr, indices.ptr, data.ptr, np_dtype_code(val_dtype), 0, None, None, None)
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
    from .pipeline import DeviceCool
    dev = dev or get_device()
    geo = chromsizes if isinstance(chromsizes, Geometry) and int(binsize) == chromsizes.binsize else bin_geometry(chromsizes, binsize)
    none = np.zeros(0, dtype=np.int64)
    table = DeviceCool({"binsize": geo.binsize, "chrom_offset": geo.offsets, "chrom_names": np.asarray(geo.names, dtype=str), "bin1_id": none,
                        "bin2_id": none, "count": none, "weight": None, "bin_start": geo.bin_start, "bin_end": geo.bin_end}, dev)
    empty = table                                   # the parent from_device_csr wants: the geometry, no pixels, no weights
    dropped = 0
    for chunk in ([chunks] if _is_single_chunk(chunks) else chunks):
        chrom1, pos1, chrom2, pos2 = chunk
        res = pairs_csr(dev, geo, chrom1, pos1, chrom2, pos2, zero_based=zero_based)
        dropped += res["dropped"]
        part = DeviceCool.from_device_csr(empty, res["indptr"], res["indices"], res["data"], res["nnz"], res["val_dtype"], weight=None,
                                          upper=True)
        del res
        table = part if table.nnz == 0 else (table if part.nnz == 0 else table.merged(part))
        del part
    table.dropped = dropped
    return table
