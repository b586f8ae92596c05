"""`detect` end to end on one genome: the callers either side of the hot path (SURVEY.md 8(f),
next-2 / next-3), so that "detect wall-clock on the test .cool" can be measured and the
reference's committed outputs reproduced.

Input is a *decoded* .cool (tools/dump_cool.py -> npz: pixels, ICE weights, chromosome offsets,
bin size); neither cooler nor h5py exists in this image.  The steps mirror the reference:
  block assembly        ContactMap.create_mat        contacts_map.py:527-548
  detrend + trim        ContactMap.detrend / remove_diags   contacts_map.py:603-638 (device)
  per kernel, per block pattern_detector(full=True)  cli/chromosight.py:601-614, 730-791 (device)
  post-processing       remove_neighbours, min_dist, NaN p-values, BH q-values
                        cli/chromosight.py:806-871
"""
import collections
import ctypes as C
import os

import threading
import zlib

import numpy as np
import pandas as pd
import scipy.sparse as sp

from . import engine
from ._lib import (COUNTS_HEADER_BYTES, CS_F32, CS_F64, FOCUS_DTYPE, LAYOUT_BAND, LAYOUT_BAND_COUNTS, LAYOUT_BAND_COUNTS_VIEW, LAYOUT_BAND_LAZY,
                   LAYOUT_BAND_PADDED, LAYOUT_DENSE, LAZY_BAND_BYTES, MASK_BINS, STAGE_SMOOTH, CsCsr, CsMatrix, CsStageBlock,
                   get_device, np_dtype_code, plain_csr)
from .utils import detection as cid
from .utils import preprocessing as preproc
from .utils.stats import fdr_correction

OUTPUT_COLUMNS = ["chrom1", "start1", "end1", "chrom2", "start2", "end2", "bin1", "bin2", "kernel_id",
                  "iteration", "score", "pvalue", "qvalue"]


class ContactBlock:
    """One intra-chromosomal sub-matrix, ready for pattern_detector (the four attributes it
    reads; reference contacts_map.py:453-526)."""

    def __init__(self, name, matrix, detectable_bins, max_dist, inter=False):
        self.name = name
        self.matrix = matrix
        self.detectable_bins = detectable_bins
        self.max_dist = max_dist
        self.inter = inter

    @property
    def shape(self):
        return self.matrix.shape


def balanced_intra_block(cool, chrom_idx):
    """count * w[bin1] * w[bin2] of one chromosome as a symmetric COO matrix, NaN where a bin
    has no weight -- what cooler's matrix(balance=True, sparse=True) returns for the block."""
    off = cool["chrom_offset"]
    s, e = int(off[chrom_idx]), int(off[chrom_idx + 1])
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    sel = (b1 >= s) & (b1 < e) & (b2 >= s) & (b2 < e)
    w = cool["weight"]
    r = (b1[sel] - s).astype(np.int64)
    c = (b2[sel] - s).astype(np.int64)
    v = cool["count"][sel] * w[b1[sel]] * w[b2[sel]]
    offd = r != c
    rows = np.concatenate([r, c[offd]])
    cols = np.concatenate([c, r[offd]])
    vals = np.concatenate([v, v[offd]])
    return sp.coo_matrix((vals, (rows, cols)), shape=(e - s, e - s))


def balanced_upper_band(cool, chrom_idx, keep):
    """Upper band (diagonals 0..keep) of the balanced intra block as CSR, built straight from the
    pixel table: cooler stores the upper triangle sorted by (bin1, bin2), so a chromosome is one
    contiguous run of pixels and the CSR row pointer is a searchsorted.  Everything the path uses
    downstream (distance law over diagonals >= 0, detrend, trim to 0..keep) only looks at this
    band, so the symmetric block of balanced_intra_block never needs to exist."""
    off = cool["chrom_offset"]
    s, e = int(off[chrom_idx]), int(off[chrom_idx + 1])
    n = e - s
    b1, b2, w = cool["bin1_id"], cool["bin2_id"], cool["weight"]
    if "_bin1_sorted" not in cool:
        cool["_bin1_sorted"] = bool(np.all(b1[1:] >= b1[:-1]))
    if cool["_bin1_sorted"]:
        lo, hi = np.searchsorted(b1, [s, e])
        r1, r2, cnt = b1[lo:hi], b2[lo:hi], cool["count"][lo:hi]
    else:
        sel = (b1 >= s) & (b1 < e)
        r1, r2, cnt = b1[sel], b2[sel], cool["count"][sel]
    d = r2 - r1
    sel = (r2 < e) & (d >= 0) & (d <= keep)
    r1, r2 = r1[sel], r2[sel]
    v = cnt[sel] * w[r1] * w[r2]
    r = (r1 - s).astype(np.int64)
    c = (r2 - s).astype(np.int32)
    if r.size == 0 or (np.all(r[1:] >= r[:-1]) and np.all((r[1:] > r[:-1]) | (c[1:] > c[:-1]))):
        indptr = np.searchsorted(r, np.arange(n + 1)).astype(np.int32 if r.size < 2 ** 31 else np.int64)
        return sp.csr_matrix((v, c, indptr), shape=(n, n))
    m = sp.coo_matrix((v, (r, c)), shape=(n, n)).tocsr()     # unsorted / duplicated pixel table
    return m


def prepare_intra_block(cool, chrom_idx, max_dist, largest_kernel, name=None):
    """ContactMap.create_mat for a balanced intra block: detrend by the distance law on the
    first keep_distance diagonals, set >= 10 to 1, keep the upper band, NaN -> 0."""
    off = cool["chrom_offset"]
    s, e = int(off[chrom_idx]), int(off[chrom_idx + 1])
    det_all = cool.get("_detectable")
    if det_all is None:
        det_all = cool["_detectable"] = np.flatnonzero(np.isfinite(cool["weight"]))
    lo, hi = np.searchsorted(det_all, [s, e])
    det = det_all[lo:hi] - s
    keep = min(max_dist, e - s) + largest_kernel
    band = balanced_upper_band(cool, chrom_idx, keep)
    mat = preproc.detrend(band, max_dist=keep, smooth=False, detectable_bins=det, max_val=10)
    mat.data[np.isnan(mat.data)] = 0
    mat.eliminate_zeros()
    return ContactBlock(name or f"chrom{chrom_idx}", mat, (det, det.copy()), max_dist)


def prepare_inter_block(cool, ca, cb, name=None):
    """ContactMap.create_mat for a balanced inter-chromosomal block (contacts_map.py:598-601,
    539-548): NaN -> 0, divide by the median of the stored values, drop zeros."""
    off = cool["chrom_offset"]
    s1, e1, s2, e2 = int(off[ca]), int(off[ca + 1]), int(off[cb]), int(off[cb + 1])
    b1, b2, w = cool["bin1_id"], cool["bin2_id"], cool["weight"]
    sel = (b1 >= s1) & (b1 < e1) & (b2 >= s2) & (b2 < e2)
    vals = cool["count"][sel] * w[b1[sel]] * w[b2[sel]]
    vals = np.where(np.isnan(vals), 0.0, vals)
    with np.errstate(all="ignore"):
        vals = vals / np.nanmedian(vals) if vals.size else vals
    vals = np.where(np.isnan(vals), 0.0, vals)
    mat = sp.coo_matrix((vals, (b1[sel] - s1, b2[sel] - s2)), shape=(e1 - s1, e2 - s2))
    mat.eliminate_zeros()
    det_all = np.flatnonzero(np.isfinite(w))
    det_r = det_all[(det_all >= s1) & (det_all < e1)] - s1
    det_c = det_all[(det_all >= s2) & (det_all < e2)] - s2
    return ContactBlock(name or f"chrom{ca}-chrom{cb}", mat.tocsr(), (det_r, det_c), None, inter=True)


def quantify_block(cool, ca, cb, coords, kernel_config, kernel, max_dist, largest_kernel, tsvd=None):
    """One task of `chromosight quantify` (cli/chromosight.py:229-260): scores of the given
    (bin1, bin2) block coordinates; rows that fail validation carry NaN scores."""
    if np.asarray(coords).shape[0] == 0:
        return None, None
    if ca == cb:
        block = prepare_intra_block(cool, ca, max_dist, largest_kernel)
    else:
        block = prepare_inter_block(cool, ca, cb)
    return cid.pattern_detector(block, kernel_config, kernel, coords=np.array(coords, dtype=int), full=True,
                                tsvd=tsvd)


# ================================================================================================
# device-resident genome: the .cool pixel table as ONE CSR in HBM, sub-matrices as views
# ================================================================================================
class _Ptr:
    """Anything the engine addresses through `.ptr` (a slice of a DeviceBuffer)."""

    def __init__(self, ptr):
        self.ptr = ptr


class _Scratch:
    """Grow-only device buffer reused by the blocks of one genome (they are staged one after the
    other on one stream, so reuse needs no synchronisation)."""

    def __init__(self, dev):
        self.dev, self.buf, self.nbytes = dev, None, 0

    def get(self, nbytes):
        if nbytes > self.nbytes:
            self.dev.sync()
            self.buf = self.dev.empty(int(nbytes * 1.25) + 256, np.uint8)
            self.nbytes = self.buf.nbytes
        return self.buf.ptr


def _pitch(width, quantum):
    """Row pitch (elements) of a staged map: `width` rounded up to `quantum`, and never a multiple of 4 KiB in float64 --
    with a power-of-two pitch the same slot of every row lies on the same memory channels, and the waves of the staging and
    tile kernels, which sweep their rows at the same pace, all hit those few channels at once (measured: the tiler of the
    23-block genome 2.9 -> see DESIGN.md)."""
    ld = (int(width) + quantum - 1) // quantum * quantum
    if (ld * 8) % 4096 == 0:
        ld += quantum
    return ld


IntraGeometry = collections.namedtuple("IntraGeometry", "keep n_diags in_w out_w band ld")


def intra_geometry(n, max_dist, largest_kernel):
    """How an intra block of n bins is staged for a scanning distance and the largest template -- the ONE statement of it, which
    _stage_fast, _stage_intra and view_for all read (a view stands in for a staging only while they agree).  keep: the
    reference's keep distance; n_diags: the diagonals its law covers; in_w / out_w: the stored and the scanned band width;
    band: the layout rule of the host path (_Staged) -- a band when it is less than half of the dense map; ld: the row pitch."""
    keep = min(max_dist, n) + largest_kernel
    in_w = min(keep, n - 1) + 1
    out_w = min(max_dist, n - 1) + 1
    band = 2 * max(in_w, out_w) < n
    return IntraGeometry(keep, min(n, keep + 1), in_w, out_w, band, _pitch(in_w, 64) if band else _pitch(n, 16))


class _FreeList:
    """Device buffers of released blocks, best fit first; every access under one lock (blocks are released by the
    garbage collector on whatever thread drops the last reference, taken by the staging threads)."""

    def __init__(self):
        self._lock = threading.Lock()
        self._bufs = []

    def release(self, buf):
        with self._lock:
            self._bufs.append(buf)

    def take(self, nbytes):
        with self._lock:
            best = None
            for k, buf in enumerate(self._bufs):
                if buf.nbytes >= nbytes and (best is None or buf.nbytes < self._bufs[best].nbytes):
                    best = k
            return self._bufs.pop(best) if best is not None else None


class _Shared:
    """HBM shared by the blocks of one staging call (laws and descriptors of lazily evaluated bands): back to the genome's
    free list when the last block that refers to it is gone."""

    def __init__(self, pool, buffer):
        self.pool, self.buffer = pool, buffer

    def __del__(self):
        try:
            self.pool.release(self.buffer)
        except Exception:
            pass


_FULL_LOCK = threading.RLock()


_BAND_LAYOUTS = (LAYOUT_BAND, LAYOUT_BAND_LAZY, LAYOUT_BAND_PADDED)


class StagedBlock:
    """One sub-matrix staged in HBM (detrended band or dense map + the flags of its undetectable bins): what pattern_detector works
    on after ContactMap.create_mat (contacts_map.py:453-526).  Every field a staging route sets is declared below; any other name raises."""

    __slots__ = ("name", "sig", "shape", "miss_row", "miss_col", "max_dist", "inter", "keep", "buffer", "pool", "row_window", "sig32", "restage",
                 "_full", "buffer32", "shared", "d_law", "n_diags", "smooth", "genome", "parent", "view", "view_row0", "strip_pool")

    def __init__(self, name, sig, shape, miss_row, miss_col, max_dist, inter, keep):
        self.name, self.sig, self.shape = name, sig, shape
        self.miss_row, self.miss_col = miss_row, miss_col
        self.max_dist, self.inter, self.keep = max_dist, inter, keep
        self.buffer, self.pool = None, None
        self.row_window = None          # (a, b): the block holds only these rows (+ halo) of the sub-matrix
        self.sig32 = None               # the same map in float32 (same layout), written by the same staging pass
        self.restage = None             # lazily evaluated float64 band (sig.layout == LAYOUT_BAND_LAZY): stages the block
        self._full = None               # again with the band stored, for the paths that read it themselves (full())
        self.buffer32 = None            # the buffer of sig32 when the block owns one beside `buffer` (released with it)
        self.shared = None              # one-call staging: the law / descriptor buffer every block of the call holds (_Shared)
        self.d_law, self.n_diags = None, None       # ... and the block's law in it: n_diags float64
        self.smooth = False             # detrended by a fitted law, which serves its own keep distance only (view_for)
        self.genome = None              # the DeviceCool a lazily evaluated band's descriptor points into (kept alive)
        self.parent = None              # view_for: the block whose buffers this view reads (kept alive; a view owns none)
        self.view, self.view_row0 = None, None      # a row strip of a trans block: the cs_csr of its staged rows, their first row
        self.strip_pool = None          # ... and the pool that owns its buffer (valid until the next strip is staged)

    @property
    def is_band(self):
        """A whole banded intra block: what the batched native entries take (view_for also takes the two counts layouts)."""
        return self.sig.layout in _BAND_LAYOUTS and not self.inter and self.row_window is None

    def full(self):
        """This block with its float64 band in memory.  The batched native entries read a lazily evaluated band through
        its descriptor (include/chromosight_hip.h cs_stage_block); every other path gets the block staged once more, the
        plain way (same values: the staging pass and the descriptor compute the same expression)."""
        if self.sig.layout != LAYOUT_BAND_LAZY:
            return self
        with _FULL_LOCK:                    # (the worker threads of a block-by-block pass ask for the same block's band at once)
            if self._full is None:
                self._full = self.restage()
        return self._full

    def __del__(self):
        # a resident block hands its HBM back to the genome's free list (hipFree synchronises and costs
        # ~0.2 ms; a genome is restaged for every pattern configuration).  The list is shared with the worker
        # threads (_resident pops under the same lock).  Reuse needs no event: every path that drops a block has
        # synchronised the streams that read it (detect / quantify return host tables), and the next staging of the
        # buffer is ordered after that synchronisation.
        try:
            if self.buffer is not None and self.pool is not None:
                self.pool.release(self.buffer)
                if self.buffer32 is not None:
                    self.pool.release(self.buffer32)
        except Exception:
            pass


class _Workers:
    """A few host threads, each with its own context (scratch, weights, pinned result buffers) and
    stream on the same GPU.  One (block, template) call is a chain of ~25 small launches and three
    host synchronisations; calls for different blocks are independent, so running several at once lets
    the GPU overlap their latency-bound kernels (ctypes releases the GIL during the native call)."""

    def __init__(self, index, n):
        import concurrent.futures
        import threading
        from ._lib import Device
        self.local = threading.local()
        self.index = index
        self.device_cls = Device
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=n)

    def device(self):
        dev = getattr(self.local, "dev", None)
        if dev is None:
            dev = self.local.dev = self.device_cls(self.index)
            # worker streams carry the short launch chains that run beside another pattern's tile kernels: served first
            self.local.stream = dev.new_stream(high_priority=True)
            self.local.scratch = _Scratch(dev)
        return dev, self.local.stream

    def scratch(self):
        self.device()
        return self.local.scratch

    def map(self, fn, items):
        return list(self.pool.map(fn, items))


# Trans blocks in row strips (detect / quantify with inter=True): the dense float64 staging of ONE strip stays below this many
# bytes unless the caller passes inter_budget.  8 GiB beside a resident genome: the float32 copy the tile
# kernel reads (context scratch) adds half of it.
INTER_BUDGET_DEFAULT = 8 << 30
_MAX_STRIP_ELEMENTS = (1 << 31) - 1


def _inter_ld(n_c):
    return (int(n_c) + 15) // 16 * 16             # (the row pitch of every staged trans block: the only place it is computed)


_InterGeometry = collections.namedtuple("_InterGeometry", "s1 e1 s2 e2 n_r n_c ld")


def plan_inter_strips(n_r, n_c, budget, halo, esz=8):
    """Row strips (a, b) of an n_r x n_c trans block whose dense staging -- rows a - halo .. b + halo - 1 clipped to the block,
    `esz`-byte values at the pitch of _stage_inter -- stays within `budget` bytes and below 2^31 elements.  Every row is owned
    by exactly one strip; the strips are as even as the budget allows.  One strip (0, n_r) when the whole block fits."""
    if budget is None or not budget > 0:
        raise ValueError("inter_budget must be a positive number of bytes")
    n_r, n_c, halo = int(n_r), int(n_c), int(halo)
    ld = _inter_ld(n_c)
    max_rows = min(int(budget) // (ld * esz), _MAX_STRIP_ELEMENTS // ld)
    if n_r <= max_rows:
        return [(0, n_r)]
    own = max_rows - 2 * halo
    if own < 1:
        raise ValueError(f"inter_budget of {int(budget)} bytes cannot hold one row and its halo of {halo} rows "
                         f"({(1 + 2 * halo) * ld * esz} bytes) of a block of {n_c} columns")
    n_strips = -(-n_r // own)
    per = -(-n_r // n_strips)
    return [(a, min(n_r, a + per)) for a in range(0, n_r, per)]


def _strip_rows(n_r, rows, halo):
    return max(0, rows[0] - halo), min(n_r, rows[1] + halo)


class _StripPool:
    """The device buffer of the row strips of trans blocks, staged one at a time: reused while it is large enough, freed before
    a larger one is allocated.  high_water: the largest number of bytes it held."""

    def __init__(self, dev):
        self.dev, self.buf, self.high_water = dev, None, 0

    def take(self, nbytes):
        nbytes = max(int(nbytes), 1)
        if self.buf is None or self.buf.nbytes < nbytes:
            if self.buf is not None:
                self.dev.sync()
                self.buf = None
            self.buf = self.dev.empty(nbytes, np.uint8)
            self.high_water = max(self.high_water, self.buf.nbytes)
        return self.buf

    def release(self):
        if self.buf is not None:
            self.dev.sync()
            self.buf = None


_WORKER_POOLS = {}
_STAGE_STREAMS = {}            # per device object: (stream, extent scratch) pairs of DeviceCool.stage_blocks


_PARENT = object()                  # DeviceCool.from_device_csr: "as the parent's"


class DeviceCool:
    """A decoded .cool resident in HBM. cooler stores the upper triangle of the whole genome
    sorted by (bin1, bin2): that table IS a CSR matrix (row pointer = searchsorted of bin1), so it
    is uploaded once -- counts, column bins, ICE weights -- and every sub-matrix is a view on it:
    balancing (count * w[bin1] * w[bin2], what cooler's matrix(balance=True) returns,
    contacts_map.py:531), the slicing of the block, diag_trim, the distance law, detrend and the
    band tiler all read the same arrays (cs_csr views, include/chromosight_hip.h)."""

    def __init__(self, cool, dev=None):
        if _is_path(cool):
            from . import io as cio
            cool = cio.load_cool(cool)                     # a .cool path: decoded here (chromosight_amd/io.py)
        dev = dev or get_device()
        off = np.asarray(cool["chrom_offset"], dtype=np.int64)
        b1 = np.asarray(cool["bin1_id"])
        b2 = np.asarray(cool["bin2_id"])
        cnt = np.asarray(cool["count"])
        if b1.size and not (np.all(b1[1:] >= b1[:-1]) and np.all((b1[1:] > b1[:-1]) | (b2[1:] > b2[:-1]))):
            order = np.lexsort((b2, b1))                      # unsorted / duplicated pixel table
            b1, b2, cnt = b1[order], b2[order], cnt[order]
        indptr = np.searchsorted(b1, np.arange(int(off[-1]) + 1)).astype(np.int64)
        # integer counts below 2^24 are exact in float32 (half the bytes of every pass)
        small = cnt.size == 0 or (np.issubdtype(cnt.dtype, np.integer) and cnt.max() < (1 << 24)) or \
            (cnt.max() < (1 << 24) and np.all(cnt == np.rint(cnt)))
        val_dtype = np.float32 if small else np.float64
        self._set_table(
            dev, names=cool["chrom_names"], offsets=off, binsize=cool["binsize"], bin_start=cool.get("bin_start"), bin_end=cool.get("bin_end"),
            indptr=dev.to_device(indptr, np.int64), indices=dev.to_device(b2, np.int32), data=dev.to_device(cnt, val_dtype),
            nnz=b1.size, val_dtype=val_dtype,
            # ... and, when none is negative, can be staged as a band of raw counts that its readers detrend (CS_LAYOUT_BAND_COUNTS)
            # (and no weight: the readers' NaN -> 0 is a max with 0)
            counts_exact=small and (cnt.size == 0 or cnt.min() >= 0),
            # what cs_stage_blocks needs: every stored pixel on or above the diagonal (a .cool's symmetric-upper storage)
            upper=b1.size == 0 or np.all(b2 >= b1),
            # no "weight" (or None): a table without balancing weights -- nothing is staged from it until set_weights()
            # (pipeline.open_cool balances it on the device: chromosight_amd/balance.py)
            weight=cool.get("weight"), host=(b1, b2, cnt))

    def _set_table(self, dev, *, names, offsets, binsize, bin_start, bin_end, indptr, indices, data, nnz, val_dtype, counts_exact, upper,
                   weight, host=None, host_dtypes=(np.int64, np.int64, np.int64), dropped=None):
        """What a resident pixel table consists of: the ONE place that fills in a DeviceCool (the constructor ends here, tables
        built on the device come through _from_table; nothing else assigns these fields).  indptr, indices, data: the device buffers
        of the CSR, the first nnz entries used.  counts_exact: every count is a non-negative integer below 2^24.  upper: every pixel
        lies on or above the diagonal; None has it checked on the pixels (a download).  weight: None for a table without.  host:
        the (bin1_id, bin2_id, count) columns where the caller holds them; None has `.host` download them when first read, in
        host_dtypes.  dropped: the pairs left out of a table binned from pairs, None for any other table."""
        self.dev, self.names, self.offsets, self.n_bins = dev, [str(n) for n in names], offsets, int(offsets[-1])
        self.binsize, self.bin_start, self.bin_end = int(binsize), bin_start, bin_end
        self.indptr, self.indices, self.data, self.nnz = indptr, indices, data, int(nnz)
        self.val_dtype, self._counts_exact, self.dropped = np.dtype(val_dtype).type, bool(counts_exact), dropped
        self._host_dtypes, self._host_weight = host_dtypes, None
        self._host = None if host is None else self._host_of(*host)
        self.upper = bool(np.all(self.host["bin2_id"] >= self.host["bin1_id"]) if upper is None else upper)
        self._retired = []
        self.weight = self.miss = self.det = self.miss_host = None
        self.counts_ok = False
        if weight is not None:
            self.set_weights(weight)
        self._band = _Scratch(self.dev)
        self._ext = _Scratch(self.dev)
        self._strips = _StripPool(self.dev)         # the row strips of trans blocks (allocates when the first one is staged)
        self._stage_lock = threading.RLock()
        self._free = _FreeList()        # HBM of released resident blocks, reused by the next staging
        self._workers = None

    @classmethod
    def _from_table(cls, dev, **table):
        """A DeviceCool over a table that is resident already: _set_table's arguments."""
        self = cls.__new__(cls)
        self._set_table(dev, **table)
        return self

    @classmethod
    def from_device_csr(cls, parent, indptr, indices, data, nnz, val_dtype, *, offsets=_PARENT, binsize=_PARENT, bin_start=_PARENT,
                        bin_end=_PARENT, weight=_PARENT, upper=_PARENT):
        """A DeviceCool over a pixel table already in HBM (device buffers of the CSR: n_bins + 1 row pointers, column bins and
        counts, the first `nnz` entries used -- the result of subsample.subsample_csr), with `parent`'s bins, names and weights.
        The counts are non-negative integers: val_dtype is float32 when they are all below 2^24, as the constructor would
        choose for an upload of the same table.  `.host` is downloaded once, when first read.
        offsets, binsize, bin_start, bin_end, weight: geometry and weights that differ from the parent's (a table of other bins:
        coarsen.coarsen_csr); weight=None makes a table without weights.  The chromosomes and their names stay the parent's, and a
        table whose pixels are the parent's regrouped by a monotone map of the bins is upper-triangle when the parent is.
        upper: whether every pixel lies on or above the diagonal, for a caller that knows (merge.merge_device: all sources do)."""
        offsets = parent.offsets if offsets is _PARENT else np.asarray(offsets, dtype=np.int64)
        if offsets.shape != parent.offsets.shape:
            raise ValueError(f"{offsets.size} chromosome offsets for the parent's {len(parent.names)} chromosomes")
        if upper is _PARENT:                # a subset of an upper-triangle table is one; anything else is checked on the pixels
            upper = True if parent.upper else None
        return cls._from_table(
            parent.dev, names=parent.names, offsets=offsets, binsize=parent.binsize if binsize is _PARENT else binsize,
            bin_start=parent.bin_start if bin_start is _PARENT else bin_start, bin_end=parent.bin_end if bin_end is _PARENT else bin_end,
            indptr=indptr, indices=indices, data=data, nnz=nnz, val_dtype=val_dtype,
            # (the counts are non-negative integers, so they are exact exactly when they fit float32)
            counts_exact=np.dtype(val_dtype) == np.float32, upper=upper, weight=parent.host_weight if weight is _PARENT else weight)

    @classmethod
    def from_pairs(cls, chunks, chromsizes, binsize, zero_based=False, dev=None):
        """A DeviceCool binned on the device from read pairs (chromosight_amd/cload.py, cs_pairs_count / cs_pairs_fill): what
        `cooler cload pairs` writes.  chunks: an iterable of (chrom1 id, pos1, chrom2 id, pos2) tuples of arrays (io.read_pairs
        yields them), or one such tuple; chromsizes: ordered name -> length in bp; binsize in bp; positions are 1-based unless
        zero_based.  Pairs with an id of -1 are dropped and counted in `.dropped`; ids or positions outside the genome refuse
        the call (ValueError).  Every pixel lies on or above the diagonal; the counts are exact, so the table is bitwise the same
        for every order of the pairs and every split into chunks.  The result has no weights: balance it (balance.ice_balance +
        set_weights, or pipeline.open_pairs)."""
        from .cload import pairs_device
        return pairs_device(chunks, chromsizes, binsize, zero_based=zero_based, dev=dev)

    @classmethod
    def from_pairs_file(cls, path, binsize, chromsizes=None, *, zero_based=False, parse="auto", piece_bytes=None, dev=None, inflate="auto"):
        """from_pairs for a 4DN .pairs / .pairs.gz file.  chromsizes: ordered name -> length in bp; None takes the #chromsize: lines
        of the file.  parse: where the text becomes columns.  "host": io.read_pairs (pandas), chunk by chunk into from_pairs.
        "device": the header pass stays on the host; the body goes to HBM in pieces of about `piece_bytes` (default
        cload.PIECE_BYTES; a .gz is inflated on the host as a stream), is parsed there (cs_pairs_text_parse, chromosight_amd/csrc/
        cs_pairs_text.hip) and binned and merged piece by piece -- the same table, bit for bit, for every piece size.  The device
        takes a strict subset of what the host reader takes (include/chromosight_hip.h: tab-separated ASCII lines of bounded
        length, positions of 1 to 18 digits, no empty line); DevicePairsRefused (a ValueError) names the first line it flags.
        "auto": the device when AUTO_PARSE_ON_DEVICE says so, and the host reader for the whole file -- its table, its `.dropped`
        and its exceptions -- as soon as the device route raises a ValueError.  CHROMOSIGHT_HIP_HOST_PARSE=1 in the environment
        forces the host route (ValueError together with parse="device").
        inflate: where a .gz on the device route becomes text.  "host": zlib on one host thread, as a stream.  "device": the file
        must be what bgzip writes (BGZF: gzip members of at most 64 KiB of text that state their own size, back to back from the
        first byte to the last, cload.bgzf_blocks); its members go to HBM as they are and are inflated there (cs_bgzf_inflate), so
        the host sees the header's members only.  DeviceInflateRefused (a ValueError) for any other .gz; engine.CorruptChunks names
        the first member that does not decode (index, file offset, status).  ValueError with parse="host", with a path that is
        not .gz.  "auto": the device for a qualifying file when AUTO_INFLATE_ON_DEVICE says so; a file that is refused or holds a
        corrupt member is read again from its start with the host's zlib, which raises what it raises.
        CHROMOSIGHT_HIP_HOST_INFLATE=1 in the environment forces the host (ValueError together with inflate="device").  Every
        route gives the same table, bit for bit."""
        from . import cload, io as cio
        from .engine import CorruptChunks
        route = _parse_route(parse)
        inflate_route = _inflate_route(inflate)
        is_gz = os.fsdecode(path).endswith(".gz")
        if inflate_route == "device":
            if route == "host":
                raise ValueError("inflate='device' inflates for the device parser: it does not go with parse='host'")
            if not is_gz:
                raise ValueError(f"inflate='device' takes a .gz file, got {path!r}")
        if piece_bytes is not None and (isinstance(piece_bytes, bool) or int(piece_bytes) != piece_bytes or int(piece_bytes) < 1):
            raise ValueError(f"piece_bytes must be a positive integer, got {piece_bytes!r}")
        pairs_file = cio.read_pairs(path, chromsizes)
        attempts = []                                   # of the device parser: over text inflated on the device, on the host
        if route != "host":
            attempts += ["device"] if is_gz and inflate_route != "host" else []
            attempts += ["host"] if inflate_route != "device" else []
        for how in attempts:
            try:
                return cload.pairs_file_device(pairs_file, binsize, zero_based=zero_based, piece_bytes=piece_bytes, dev=dev, inflate=how)
            except (ValueError, EOFError, zlib.error) as exc:   # (DevicePairsRefused and the two below are ValueErrors)
                if how == "device" and isinstance(exc, (DeviceInflateRefused, CorruptChunks)):
                    if inflate_route == "device":
                        raise
                    continue                            # "auto": the host inflates
                if route == "device":
                    raise
                break
        return cls.from_pairs(pairs_file, pairs_file.chromsizes, binsize, zero_based=zero_based, dev=dev)

    @classmethod
    def from_cool_file(cls, path, *, balance="weight", dev=None):
        """A DeviceCool whose pixel table was decoded on the device (cs_inflate_chunks, cs_table_from_columns_*): the stored chunks
        of pixels/bin1_id, bin2_id and count go to HBM as they are in the file, are inflated and unshuffled there, and one pass
        checks the table and builds what the constructor would upload for the same file -- row pointers, int32 column bins, counts
        as float32 or float64 -- bit for bit.  path: a .cool, or `file.mcool::/resolutions/<binsize>`.  The small datasets
        (chromosome names and offsets, bin starts and ends, the `bins/<balance>` column, taken as stored; a file without one gives a
        table without weights) are decoded on the host.  `.host` is downloaded when first read.  DeviceDecodeRefused (a ValueError)
        for a file that does not qualify: one hdf5_lite does not read, pixel columns that are not chunked int32 / int64 datasets with
        filters among shuffle, gzip and Fletcher-32 in that order, chunks beyond engine.inflate_max_chunk_bytes(), ids outside the
        bins, or a table that is not strictly sorted by (bin1, bin2).  engine.CorruptChunks for chunks that do not decode."""
        return _device_cool_from_file(path, balance, dev, lambda cool: cool["weight"])

    def set_weights(self, weight):
        """Take new balancing weights (n_bins values, NaN = bin without a weight): uploads `weight` and the missing /
        detectable flags, refreshes counts_ok and the host copy.  The pixel table stays as it is.  The buffers of the
        previous weights are kept alive (blocks staged before point into them); stage again to use the new ones."""
        weight = np.asarray(weight, dtype=np.float64)
        if weight.shape != (self.n_bins,):
            raise ValueError(f"weights of shape {weight.shape} for a table of {self.n_bins} bins")
        if self.weight is not None:
            self._retired.append((self.weight, self.miss, self.det))
        dev = self.dev
        self.counts_ok = bool(self._counts_exact and not np.any(weight < 0))
        self.weight = dev.to_device(weight, np.float64)
        miss = ~np.isfinite(weight)
        self.miss_host = miss
        self.miss = dev.to_device(miss.astype(np.uint8))
        self.det = dev.to_device((~miss).astype(np.uint8))
        self._host_weight = weight
        if self._host is not None:
            self._host["weight"] = weight

    @property
    def host(self):
        """The pixel table as a decoded-cool dictionary (bin1_id, bin2_id, count, weight, ...).  A table built on the device
        (from_device_csr, from_cool_file) downloads it here, once; one decoded from a file gets the dtypes io._read_cool gives."""
        if self._host is None:
            n = int(self.nnz)
            indptr = self.indptr.download()
            t1, t2, tc = self._host_dtypes
            b1 = np.repeat(np.arange(self.n_bins, dtype=t1), np.diff(indptr))
            b2 = self.indices.download()[:n].astype(t2)
            cnt = self.data.download().view(self.val_dtype)[:n].astype(tc)
            self._host = self._host_of(b1, b2, cnt)
        return self._host

    def _host_of(self, b1, b2, cnt):
        return {"binsize": self.binsize, "chrom_offset": self.offsets, "chrom_names": np.asarray(self.names), "bin1_id": b1, "bin2_id": b2,
                "count": cnt, "weight": self._host_weight, "bin_start": self.bin_start, "bin_end": self.bin_end}

    @property
    def upload_bytes(self):
        """The bytes an upload of the table and its weights moves (a buffer filled on the device may have room for more pixels)."""
        pixels = self.nnz * (self.indices.dtype.itemsize + np.dtype(self.val_dtype).itemsize)
        return self.indptr.nbytes + pixels + (0 if self.weight is None else self.weight.nbytes)

    @property
    def host_weight(self):
        """The balancing weights on the host (None before set_weights)."""
        return self._host_weight

    @property
    def has_weights(self):
        return self.weight is not None

    def _need_weights(self):
        if self.weight is None:
            raise ValueError("this pixel table has no balancing weights: balance it first (pipeline.open_cool, "
                             "balance.ice_balance + DeviceCool.set_weights)")

    def csr(self):
        """The whole-genome pixel table as a plain cs_csr (no weights)."""
        return plain_csr(self.n_bins, self.nnz, self.indptr, self.indices, self.data, self.val_dtype)

    def _resident(self, nbytes, dev=None):
        buf = self._free.take(nbytes)
        return buf if buf is not None else (dev or self.dev).empty(nbytes, np.uint8)

    def stage_blocks(self, chroms, max_dist, largest_kernel, workers=1, **options):
        """stage_intra(resident=True) of several chromosomes.  Default: one host thread deals the blocks to a few streams
        (below).  workers > 1: host threads with their own contexts stage several blocks at a time (see _Workers) --
        measured slower than ONE stream on the 23-block genome (the hand-over costs two synchronisations per block).
        Every block's staging is complete on return."""
        self._need_weights()
        chroms = list(chroms)
        lazy64 = options.pop("lazy64", False)                # (only the one-call staging knows lazily evaluated bands)
        counts = options.pop("counts", None)                 # (... and bands of raw counts)
        # One staging call at a time per pixel table: the calls share this context's staging scratch, its page-locked
        # table slots and the law scratch, and they are ordered on one stream.  (Patterns scanned side by side by several
        # host threads each stage the blocks they cannot take as views -- short chromosomes staged dense for a wider
        # pattern: two such calls at once handed each other's block tables to the kernels.)
        with self._stage_lock:
            fast = self._stage_fast(chroms, max_dist, largest_kernel, lazy64=lazy64, counts=counts, **options)
        if fast is not None:
            return fast
        if workers <= 1 or len(chroms) <= 1:
            # one host thread, the blocks dealt to a few streams of this context (each with its own extent scratch):
            # a block's chain is 7 short launches that leave most of the chip idle, the chains of different blocks
            # are independent, and issuing them costs the host less than running them costs the GPU (23-block genome,
            # per step: 1 stream 12.8 ms, 2: 12.5, 4: 11.4-11.7, 6-12: 11.2)
            n_streams = min(6, len(chroms))
            # (smooth here: what the one-call staging could not take -- the host fit between two copies, block after block)
            if n_streams <= 1 or options.get("reduce") is not None or options.get("smooth"):
                return [self.stage_intra(ci, max_dist, largest_kernel, resident=True, **options) for ci in chroms]
            # process-wide like the worker pools: creating streams per DeviceCool cost 8 ms per `detect` on a small genome
            pairs = _STAGE_STREAMS.setdefault(id(self.dev), (self.dev, []))[1]      # (the entry keeps the device alive)
            if len(pairs) < n_streams:
                pairs += [(self.dev.new_stream(), _Scratch(self.dev)) for _ in range(n_streams - len(pairs))]
            self.dev.sync()
            blocks = []
            for k, ci in enumerate(chroms):
                stream, ext = pairs[k % n_streams]
                blocks.append(self.stage_intra(ci, max_dist, largest_kernel, resident=True, stream=stream, ext=ext, **options))
            for stream, _ in pairs[:n_streams]:
                self.dev.sync(stream)
            return blocks
        self.dev.sync()                         # uploads / a previous pass on the default stream
        pool = self.workers(workers)

        def one(ci):
            dev, stream = pool.device()
            block = self.stage_intra(ci, max_dist, largest_kernel, resident=True, stream=stream, dev=dev, ext=pool.scratch(),
                                     **options)
            dev.sync(stream)
            return block

        return pool.map(one, chroms)

    def _stage_fast(self, chroms, max_dist, largest_kernel, smooth=False, band_dtype=np.float64, reduce=None, rows=None,
                    stream=None, lazy64=False, counts=None, **unused):
        """All the given chromosomes with ONE native call (cs_stage_blocks: three launches for the whole genome -- a
        pass over the pixel table for the distance laws, the laws' finish, and the detrend / tiler that writes every
        block once in float64 (exact re-scoring, windows) and float32 (what the matrix-core kernel stages)); None when
        an option needs the block-by-block path (a block split over ranks, a law of more than 4096 diagonals, a pixel table
        with a lower triangle).  smooth (--smooth-trend): one more launch fits every block's law on the device
        (cs_stage_blocks_opt, CS_STAGE_SMOOTH) before anything is detrended by it; lazily evaluated bands and bands of raw
        counts read the fitted law like any other."""
        if (reduce is not None or rows is not None or unused or not self.upper or not chroms
                or np.dtype(band_dtype) not in (np.dtype(np.float64), np.dtype(np.float32))):
            return None
        only32 = np.dtype(band_dtype) == np.float32       # float32 maps only (map-level callers: no exact re-scoring)
        dev, lib = self.dev, self.dev.lib
        geo = []
        for ci in chroms:
            s, e = int(self.offsets[ci]), int(self.offsets[ci + 1])
            g = intra_geometry(e - s, max_dist, largest_kernel)
            if g.n_diags > 4096:
                return None
            geo.append((ci, s, e - s, g))
        # lazy64: the float64 band of a banded block is NOT stored beyond its first `near` diagonals (where the runs of a
        # 1-D pattern live); the float64 kernels behind the batched entries recompute the few pixels they read from the
        # pixel table (include/chromosight_hip.h cs_stage_block: a third of the staging pass was writing that band).  The
        # laws and the descriptors then live as long as the blocks do: one shared buffer each, not the rewritten scratch.
        # (lazy64 = "all": every diagonal stored AND a descriptor -- what tests/test_gpu_device_pipeline.py checks the recomputed
        # pixels against)
        near = 64
        lazy = [bool(lazy64 and not only32 and g.band and (lazy64 == "all" or g.in_w > 2 * near)) for _, _, _, g in geo]
        # counts (default wherever the float64 band is lazily evaluated -- the detection path --; float32-only, map-level callers
        # ask for it): the float32 band of a banded block holds the RAW COUNTS, written by the pass that reduces the distance
        # law -- no detrend / tiler pass over the pixel table, no float64 near band; the tile kernel detrends the tiles it
        # fetches (float32) and the float64 kernels every pixel they read (the staging pass's own expression;
        # include/chromosight_hip.h CS_LAYOUT_BAND_COUNTS).  Needs counts that are exact in float32 and not negative (what a
        # .cool holds).  Measured (profiles/r05_counts_band.txt): the C3 step 0.222 -> 0.212 ms and a quarter less HBM
        # traffic; a rank's share of 8 of the C4 genome 0.520 -> 0.507 ms (rank 5) / 0.470 -> 0.445 (rank 0), the whole genome
        # 2.82 -> 2.81 ms.  CHROMOSIGHT_HIP_NO_COUNTS_BAND=1: the detrended bands of the tiler pass.
        if counts is None:
            counts = bool(lazy64) and lazy64 != "all"
        counts = bool(counts and self.counts_ok and not os.environ.get("CHROMOSIGHT_HIP_NO_COUNTS_BAND"))
        cnt = [bool(counts and g.band and (only32 or lazy[k])) for k, (_, _, _, g) in enumerate(geo)]
        # The laws (and the descriptors of lazily evaluated bands) live as long as the blocks do: one buffer per staging call,
        # held by every block of the call -- never the rewritten law scratch.  A recorded staging (plan.StepPlan replays the
        # cs_stage_blocks table verbatim, d_law included) must not point into a grow-only scratch that a later staging with a
        # longer law re-allocates (silent corruption on the next replay).
        # (counts: CS_COUNTS_LAW_BYTES -- the law, its reciprocals, float32 copies of the reciprocals and of the block's weights)
        law_len = [(2 * g.n_diags + 2 + (g.n_diags + 3) // 2 + (n + 1) // 2) if cnt[k] else g.n_diags for k, (_, _, n, g) in enumerate(geo)]
        shared = _Shared(self._free, self._resident(8 * sum(law_len) + 256 + LAZY_BAND_BYTES * len(geo)))
        laws = shared.buffer.ptr + LAZY_BAND_BYTES * len(geo)
        table = (CsStageBlock * len(geo))()
        blocks, off = [], 0
        for k, (ci, s, n, (keep, n_diags, in_w, _, band, ld)) in enumerate(geo):
            if cnt[k]:
                ld = _pitch(in_w + 4, 64)                       # (a band of raw counts: >= 4 zero slots behind every row's diagonals)
            near_k = in_w if lazy64 == "all" else near
            ld64 = (ld if lazy64 == "all" else _pitch(near, 2)) if lazy[k] else ld
            b64 = None if (only32 or cnt[k]) else self._resident(n * ld64 * 8)
            head = COUNTS_HEADER_BYTES if cnt[k] else 0
            b32 = self._resident(n * ld * 4 + head)
            p32 = b32.ptr + head
            desc = shared.buffer.ptr + LAZY_BAND_BYTES * k if lazy[k] else None
            if cnt[k]:
                table[k] = CsStageBlock(s, n, keep, LAYOUT_BAND, in_w, ld, None, p32, laws + off, 0, 0, 1, desc)
            else:
                table[k] = CsStageBlock(s, n, keep, LAYOUT_BAND if band else LAYOUT_DENSE, in_w if band else 0, ld,
                                        b64.ptr if b64 is not None else None, p32, laws + off,
                                        ld64 if lazy[k] else 0, near_k if lazy[k] else 0, 0, desc)
            off += 8 * law_len[k]
            layout = LAYOUT_BAND if band else LAYOUT_DENSE
            flags = _Ptr(self.miss.ptr + s)
            # (the staging pass assembles every row in zeroed pieces of ld slots: the float32 band is zero behind its stored
            # diagonals -- the tile kernel fetches its rim tiles like the inner ones, include/chromosight_hip.h)
            sig32 = CsMatrix(p32, CS_F32, LAYOUT_BAND_COUNTS if cnt[k] else LAYOUT_BAND_PADDED if band and ld >= in_w + 4 else layout, ld, 0,
                             in_w if band else 0, 0)
            if only32:
                sig64 = sig32
            elif lazy[k]:
                sig64 = CsMatrix(desc, CS_F64, LAYOUT_BAND_LAZY, ld, 0, in_w, 0)
            else:
                sig64 = CsMatrix(b64.ptr, CS_F64, layout, ld, 0, in_w if band else 0, 0)
            blk = StagedBlock(self.names[ci], sig64, (n, n), flags, flags, max_dist, False, keep)
            blk.sig32 = sig32
            blk.buffer, blk.pool = (b32 if (only32 or b64 is None) else b64), self._free
            blk.buffer32 = None if (only32 or b64 is None) else b32
            blk.shared = shared                                 # (the law buffer of the call)
            blk.d_law, blk.n_diags = laws + off - 8 * law_len[k], n_diags      # (the block's law in it: n_diags float64)
            blk.smooth = bool(smooth)                           # (a fitted law serves its own keep distance only: view_for)
            if lazy[k]:
                blk.genome = self                               # (the descriptor points into the pixel table)
                blk.restage = (lambda ci=ci: self._restage_synced(ci, max_dist, largest_kernel, band_dtype=band_dtype, smooth=smooth))
            blocks.append(blk)
        genome = self._view(0, self.n_bins, 0, self.n_bins)
        # asynchronous on `stream`: whoever reads the blocks on another stream or context synchronises first (the callers
        # that hand blocks to worker threads do; the law scratch is rewritten in stream order)
        with dev.lock:
            if smooth:
                dev._check(lib.cs_stage_blocks_opt(dev.ctx, stream, C.byref(genome), table, len(geo), 10.0, STAGE_SMOOTH))
            else:
                dev._check(lib.cs_stage_blocks(dev.ctx, stream, C.byref(genome), table, len(geo), 10.0))
        return blocks

    def _restage_synced(self, ci, max_dist, largest_kernel, **options):
        """One block staged again with its float64 band stored (StagedBlock.full), COMPLETE on return: the staging call is
        asynchronous on this genome's stream, and who asks for the full band is a per-block path on a worker thread with a
        context and stream of its own -- it read a band that was still being written (a 2-D pattern with pearson < 0.1 scanned
        beside a 1-D pattern lost a third of its records, differently every run: found by
        tests/test_gpu_device_pipeline.py::test_2d_chain_retry_and_fallback_paths)."""
        with self._stage_lock:
            block = self.stage_blocks([ci], max_dist, largest_kernel, **options)[0]
            self.dev.sync()
        return block

    def view_for(self, block, max_dist, largest_kernel):
        """The staged block of the same chromosome for a pattern with a shorter scanning distance, WITHOUT staging it again:
        ContactMap.create_mat with keep' = min(max_dist, n) + largest_kernel <= keep is the band of the first keep' + 1
        diagonals of the block staged with `keep` -- the distance law of a diagonal does not depend on how many others are
        kept (preprocessing.py:173-188, without --smooth-trend), so the detrended values are the same numbers, and a band
        view with fewer stored diagonals reads every pixel beyond them as 0 (diag_trim).  None when a view cannot stand in
        (dense-staged short chromosomes, row windows, a longer distance than the block holds)."""
        self._need_weights()
        keep, _, in_w, _, band, _ = intra_geometry(block.shape[0], max_dist, largest_kernel)
        # (beside the layouts of StagedBlock.is_band, a view can be cut from the two bands of raw counts)
        if (block.inter or block.sig.layout not in _BAND_LAYOUTS + (LAYOUT_BAND_COUNTS, LAYOUT_BAND_COUNTS_VIEW)
                or block.row_window is not None or block.keep is None or keep > block.keep or block.smooth):
            return None
        if not band:
            return None                              # this pattern would have been staged dense: keep the layouts identical
        s = block.sig
        # (a narrower view of a zero-padded band is a plain band: the slots behind ITS diagonals hold the block's further ones)
        narrower = {LAYOUT_BAND_PADDED: LAYOUT_BAND, LAYOUT_BAND_COUNTS: LAYOUT_BAND_COUNTS_VIEW}
        view = StagedBlock(block.name, CsMatrix(s.d_ptr, s.dtype, narrower.get(s.layout, s.layout), s.ld, 0, in_w, s.row0), block.shape, block.miss_row,
                           block.miss_col, max_dist, False, keep)
        if s.layout == LAYOUT_BAND_LAZY:                 # (a view shares the descriptor; read by itself it is staged for itself)
            ci = self.names.index(block.name)
            view.restage = lambda: self._restage_synced(ci, max_dist, largest_kernel)
        if block.sig32 is not None:
            t = block.sig32
            view.sig32 = CsMatrix(t.d_ptr, t.dtype, LAYOUT_BAND_COUNTS_VIEW if t.layout in (LAYOUT_BAND_COUNTS, LAYOUT_BAND_COUNTS_VIEW) else LAYOUT_BAND,
                                  t.ld, 0, in_w, t.row0)
        view.parent = block                          # keeps the buffers alive; the view owns none
        return view

    def workers(self, n=4):
        # process-wide: the workers' contexts, streams and scratch outlive this DeviceCool (creating them costs
        # several milliseconds, more than a whole detect on a small genome)
        key = (self.dev.index, n)
        if key not in _WORKER_POOLS:
            _WORKER_POOLS[key] = _Workers(self.dev.index, n)
        return _WORKER_POOLS[key]

    @property
    def n_chrom(self):
        return len(self.offsets) - 1

    def chrom_size(self, ci):
        return int(self.offsets[ci + 1] - self.offsets[ci])

    def _view(self, s, e, cs, ce, begin=None, end=None):
        return CsCsr(e - s, ce - cs, max(self.nnz, 1),
                     begin if begin is not None else self.indptr.ptr + 8 * s, self.indices.ptr, self.data.ptr,
                     np_dtype_code(self.val_dtype), cs, end, self.weight.ptr + 8 * s, self.weight.ptr + 8 * cs)

    def stage_intra(self, *args, dev=None, **options):
        """_stage_intra holding the context it uses (one call in flight per context: engine._one_call_per_context)."""
        self._need_weights()
        with (dev or self.dev).lock:
            return self._stage_intra(*args, dev=dev, **options)

    def stage_inter(self, *args, rows=None, largest_kernel=None, median=None, **options):
        """_stage_inter; rows = (a, b): only the rows a <= i < b of the block plus a halo of (largest_kernel - 1) // 2 rows on
        either side, dense, CsMatrix.row0 = a - halo (clipped to the block), in the strip pool (inter_high_water) -- the block
        scaled by the median of the WHOLE block (`median`, else computed here: inter_median), so a strip holds the same values
        as those rows of the unsplit block.  The strip's `view` (cs_csr of its staged rows) is valid until the next staging."""
        self._need_weights()
        with self.dev.lock:
            if rows is None:
                return self._stage_inter(*args, **options)
            return self._stage_inter_rows(*args, rows=rows, largest_kernel=largest_kernel, median=median, **options)

    @property
    def inter_high_water(self):
        """Largest number of device bytes the strip pool of trans blocks held (stage_inter(rows=...))."""
        return self._strips.high_water

    # The steps of trans staging, each written once: _stage_inter, _stage_inter_rows and stage_inter_many differ only in the rows
    # they cover, where the buffer comes from, how the median is obtained and how many uploads they make.
    def _inter_geometry(self, ca, cb):
        """The trans block (ca, cb): the genome bins of its rows s1 .. e1 and columns s2 .. e2, its shape and its row pitch."""
        s1, e1 = int(self.offsets[ca]), int(self.offsets[ca + 1])
        s2, e2 = int(self.offsets[cb]), int(self.offsets[cb + 1])
        return _InterGeometry(s1, e1, s2, e2, e1 - s1, e2 - s2, _inter_ld(e2 - s2))

    def _inter_extent(self, geo, ra, rb, d_begin, d_end, stream):
        """The extent pass over the rows ra .. rb - 1 of the block: their view (row r of the view = row ra + r of the block, the
        columns of chromosome cb), bounded to the block's columns by the row extents written at d_begin / d_end."""
        raw = self._view(geo.s1 + ra, geo.s1 + rb, geo.s2, geo.e2)
        self.dev._check(self.dev.lib.cs_csr_band_extent(self.dev.ctx, stream, C.byref(raw), -geo.n_r, geo.n_c, d_begin, d_end))
        return self._view(geo.s1 + ra, geo.s1 + rb, geo.s2, geo.e2, d_begin, d_end)

    def _inter_whole_median(self, geo, ext, stream):
        """(bounded view of the whole block, extents at `ext`; the median of its stored values)."""
        view = self._inter_extent(geo, 0, geo.n_r, ext, ext + 8 * geo.n_r, stream)
        med = C.c_double(0.0)
        self.dev._check(self.dev.lib.cs_csr_median(self.dev.ctx, stream, C.byref(view), C.byref(med)))
        return view, med.value

    def _inter_scatter(self, view, d_law, n_law, ptr, dtype, ld, stream):
        """The rows of `view` written dense at `ptr`: the "law" at d_law is the block's median on every diagonal, no cap --
        value / median, NaN -> 0.  Returns the matrix written (row0 = 0: the scatter addresses the view's own rows)."""
        sig = CsMatrix(ptr, np_dtype_code(dtype), LAYOUT_DENSE, ld, 0, 0, 0)
        self.dev._check(self.dev.lib.cs_csr_to_band(self.dev.ctx, stream, C.byref(view), d_law, n_law, 0.0, C.byref(sig)))
        return sig

    def _inter_block(self, ca, cb, geo, sig, name=None, own=None):
        block = StagedBlock(name or f"{self.names[ca]}-{self.names[cb]}", sig, (geo.n_r, geo.n_c), _Ptr(self.miss.ptr + geo.s1),
                            _Ptr(self.miss.ptr + geo.s2), None, True, None)
        block.buffer, block.pool = own, self._free       # (own: the buffer the block hands back to the free list when it goes)
        return block

    def inter_median(self, ca, cb, stream=None):
        """The median _stage_inter scales the trans block (ca, cb) by (cs_csr_median on the view of the whole block)."""
        self._need_weights()
        with self.dev.lock:
            geo = self._inter_geometry(ca, cb)
            return self._inter_whole_median(geo, self._ext.get(16 * geo.n_r + 512), stream)[1]

    def _stage_inter_rows(self, ca, cb, rows, largest_kernel=None, median=None, name=None, stream=None, dtype=np.float64):
        geo = self._inter_geometry(ca, cb)
        n_r, n_c, ld = geo.n_r, geo.n_c, geo.ld
        a, b = int(rows[0]), int(rows[1])
        if not (0 <= a < b <= n_r):
            raise ValueError("row window outside the block")
        if largest_kernel is None:
            raise ValueError("a row strip needs largest_kernel (its halo)")
        halo = (int(largest_kernel) - 1) // 2
        ra, rb = _strip_rows(n_r, (a, b), halo)
        m = rb - ra
        if m * ld > _MAX_STRIP_ELEMENTS:
            raise ValueError(f"a strip of {m} rows x {ld} is above 2^31 elements: cut the block into more strips")
        if median is None:
            median = self.inter_median(ca, cb, stream=stream)
        n_law = max(n_r, n_c)
        ext = self._ext.get(16 * m + 8 * n_law + 512)
        d_law = ext + 16 * m
        view = self._inter_extent(geo, ra, rb, ext, ext + 8 * m, stream)
        scale = np.full(n_law, float(median))
        self.dev._check(self.dev.lib.cs_memcpy_h2d(self.dev.ctx, d_law, scale.ctypes.data, scale.nbytes, stream))
        buf = self._strips.take(m * ld * np.dtype(dtype).itemsize)
        sig = self._inter_scatter(view, d_law, n_law, buf.ptr, dtype, ld, stream)
        sig.row0 = ra                                    # (the block's matrix carries the strip's first row)
        block = self._inter_block(ca, cb, geo, sig, name)
        block.row_window = (a, b)
        block.view, block.view_row0 = view, ra
        block.strip_pool = self._strips                  # (the pool owns the buffer; the strip is valid until the next staging)
        return block

    def _stage_intra(self, ci, max_dist, largest_kernel, smooth=False, band_dtype=np.float64, name=None, stream=None,
                     resident=False, rows=None, reduce=None, dev=None, ext=None):
        """ContactMap.create_mat of one balanced intra block, on the device: distance law over the
        first keep_distance diagonals of the detectable bins, detrend, >= 10 -> 1, NaN -> 0, upper
        band only (contacts_map.py:527-548, 603-638; preprocessing.py:129-197, 256-310).

        rows = (a, b): stage only the rows a <= i < b of the block plus the template's halo of
        (largest_kernel - 1) // 2 rows on either side (one block split over several GPUs, SURVEY.md
        8(e)); the distance law is then the sum of every part's per-diagonal (sum, count): `reduce`
        maps this part's float64 array (2, n_diags) to the total (an all-reduce).  The block's
        `row_window` is (a, b) and its matrix carries row0."""
        # dev / ext: a worker's own context and extent scratch (stage_blocks); the buffers live in the device's one
        # address space whichever context allocated them
        dev = dev or self.dev
        lib = dev.lib
        s, e = int(self.offsets[ci]), int(self.offsets[ci + 1])
        n = e - s
        keep, n_diags, in_w, _, band, ld = intra_geometry(n, max_dist, largest_kernel)
        a, b = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
        if not (0 <= a < b <= n):
            raise ValueError("row window outside the block")
        split = (a, b) != (0, n)
        if split and not band:
            raise ValueError("only blocks staged as a band can be split by rows")
        halo = (largest_kernel - 1) // 2 if split else 0
        ra, rb = max(0, a - halo), min(n, b + halo)
        m = rb - ra
        ext = (ext or self._ext).get(16 * m + 16 * (keep + 2) + 512)
        d_begin, d_end = ext, ext + 8 * m
        d_sum = d_end + 8 * m
        d_cnt, d_law = d_sum + 8 * (keep + 2), None
        # a view of the rows ra .. rb-1 whose column origin moves with it: diagonals are unchanged
        raw = self._view(s + ra, s + rb, s + ra, e)
        dev._check(lib.cs_csr_band_extent(dev.ctx, stream, C.byref(raw), 0, keep, d_begin, d_end))
        view = self._view(s + ra, s + rb, s + ra, e, d_begin, d_end)
        own = self._view(s + a, s + b, s + a, e, d_begin + 8 * (a - ra), d_end + 8 * (a - ra)) if split else view
        dev._check(lib.cs_distance_law_csr(dev.ctx, stream, C.byref(own), self.det.ptr + s + a, n_diags, d_sum, d_cnt))
        if (smooth and n > 2) or reduce is not None:
            sums = np.empty(n_diags)
            cnts = np.empty(n_diags, dtype=np.int64)
            dev._check(lib.cs_memcpy_d2h(dev.ctx, sums.ctypes.data, d_sum, 8 * n_diags, stream))
            dev._check(lib.cs_memcpy_d2h(dev.ctx, cnts.ctypes.data, d_cnt, 8 * n_diags, stream))
            if reduce is not None:
                total = np.asarray(reduce(np.stack([sums, cnts.astype(np.float64)])), dtype=np.float64)
                sums, cnts = np.ascontiguousarray(total[0]), np.rint(total[1]).astype(np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                law = np.where(cnts > 0, sums / np.maximum(cnts, 1), 0.0)      # cs_distance_law_finish
            if smooth and n > 2:
                full_law = np.zeros(n)
                full_law[:n_diags] = law
                law = preproc._isotonic_non_increasing(full_law)[:n_diags]
            law = np.ascontiguousarray(law, dtype=np.float64)
            law[np.isnan(law)] = 0.0
            dev._check(lib.cs_memcpy_h2d(dev.ctx, d_sum, law.ctypes.data, 8 * n_diags, stream))
            d_law = d_sum
        else:
            d_law = d_sum                                     # finished in place
            dev._check(lib.cs_distance_law_finish(dev.ctx, stream, d_sum, d_cnt, n_diags, d_law))
        esz = np.dtype(band_dtype).itemsize
        # resident: the block owns its buffer (288 GB of HBM hold every block of a genome at once, so
        # blocks are staged once and reused by all templates / iterations); else a shared scratch
        buf = self._resident(m * ld * esz, dev) if resident else None
        ptr = buf.ptr if resident else self._band.get(m * ld * esz)
        sig = CsMatrix(ptr, np_dtype_code(band_dtype), LAYOUT_BAND if band else LAYOUT_DENSE, ld, 0, in_w if band else 0, ra)
        dev._check(lib.cs_csr_to_band(dev.ctx, stream, C.byref(view), d_law, n_diags, 10.0, C.byref(sig)))
        flags = _Ptr(self.miss.ptr + s)
        block = StagedBlock(name or self.names[ci], sig, (n, n), flags, flags, max_dist, False, keep)
        block.buffer, block.pool = buf, self._free
        block.row_window = (a, b) if split else None
        block.smooth = bool(smooth)
        return block

    def _stage_inter(self, ca, cb, name=None, stream=None, resident=False, dtype=np.float64):
        """ContactMap.create_mat of a balanced inter-chromosomal block (ca < cb), on the device:
        NaN -> 0, divided by the median of its stored values (contacts_map.py:598-601), dense layout."""
        geo = self._inter_geometry(ca, cb)
        n_r, n_c, ld = geo.n_r, geo.n_c, geo.ld
        n_law = max(n_r, n_c)
        ext = self._ext.get(16 * n_r + 8 * n_law + 512)
        d_law = ext + 16 * n_r
        view, med = self._inter_whole_median(geo, ext, stream)
        scale = np.full(n_law, med)
        self.dev._check(self.dev.lib.cs_memcpy_h2d(self.dev.ctx, d_law, scale.ctypes.data, scale.nbytes, stream))
        nbytes = n_r * ld * np.dtype(dtype).itemsize
        own = self._resident(nbytes) if resident else None
        ptr = own.ptr if resident else self._band.get(nbytes)
        return self._inter_block(ca, cb, geo, self._inter_scatter(view, d_law, n_law, ptr, dtype, ld, stream), name, own)

    def stage_inter_many(self, pairs, dtype=np.float64, stream=None):
        """stage_inter(resident=True) for SEVERAL inter-chromosomal blocks: the extents of all of them, then their medians with
        one native call (cs_csr_median_many: two synchronisations in all instead of two per block), then the dense maps."""
        self._need_weights()
        pairs = list(pairs)
        if not pairs:
            return []
        with self.dev.lock:
            dev, lib = self.dev, self.dev.lib
            geos = [self._inter_geometry(ca, cb) for ca, cb in pairs]
            # (the blocks' row extents, then their "laws" -- their median on every diagonal -- side by side: ONE upload)
            ext_off, total, law_off, laws = [], 0, [], 0
            for geo in geos:
                ext_off.append(total)
                total += (16 * geo.n_r + 511) // 256 * 256
                law_off.append(laws)
                laws += (max(geo.n_r, geo.n_c) + 31) // 32 * 32
            ext = self._ext.get(total + 8 * laws + 512)
            views = (type(self._view(0, 1, 0, 1)) * len(pairs))()
            for i, geo in enumerate(geos):
                d_begin = ext + ext_off[i]
                views[i] = self._inter_extent(geo, 0, geo.n_r, d_begin, d_begin + 8 * geo.n_r, stream)
            med = (C.c_double * len(pairs))()
            dev._check(lib.cs_csr_median_many(dev.ctx, stream, views, len(pairs), med))
            scale = np.empty(laws)
            for i, geo in enumerate(geos):
                scale[law_off[i]:law_off[i] + max(geo.n_r, geo.n_c)] = med[i]
            dev._check(lib.cs_memcpy_h2d(dev.ctx, ext + total, scale.ctypes.data, scale.nbytes, stream))
            out = []
            for i, ((ca, cb), geo) in enumerate(zip(pairs, geos)):
                own = self._resident(geo.n_r * geo.ld * np.dtype(dtype).itemsize)
                sig = self._inter_scatter(views[i], ext + total + 8 * law_off[i], max(geo.n_r, geo.n_c), own.ptr, dtype, geo.ld, stream)
                out.append(self._inter_block(ca, cb, geo, sig, own=own))
            return out

    def subsampled(self, sample, seed=0, inter=False, sampler="numpy"):
        """A DeviceCool whose counts are a random subsample of this one's, drawn per sub-matrix without
        replacement like the reference's --subsample (contacts_map.py:552-596, preprocessing.py:359-401):
        `sample` in (0, 1] is the proportion of the contacts of every sub-matrix to keep.  Intra blocks
        are sampled as the reference sees them (symmetric matrix, both triangles drawn independently;
        the path then only reads the upper one).  Unlike the reference's unseeded np.random.choice the
        draw is reproducible: numpy Generator(seed), multivariate hypergeometric.
        sampler="device" draws the same pools on the device (chromosight_amd/subsample.py: exact hypergeometric split trees,
        counter-based uniforms): another table for a given seed than "numpy", the same on every device; the result stays in HBM."""
        if sampler not in ("numpy", "device"):
            raise ValueError(f"sampler must be 'numpy' or 'device', got {sampler!r}")
        if sampler == "device":
            from .subsample import subsample_device
            return subsample_device(self, sample, seed=seed, inter=inter)
        sample = float(sample)
        if sample < 0:
            raise ValueError("Subsample must be strictly positive.")
        if sample > 1:
            raise ValueError("Subsample cannot be above 1")
        rng = np.random.default_rng(seed)
        h = self.host
        b1, b2, cnt = h["bin1_id"], h["bin2_id"], np.asarray(h["count"]).astype(np.int64)
        off = self.offsets
        chrom_of = np.repeat(np.arange(self.n_chrom), np.diff(off))
        c1, c2 = chrom_of[b1], chrom_of[b2]
        new = np.zeros_like(cnt)
        for ca in range(self.n_chrom):
            for cb in range(ca, self.n_chrom if inter else ca + 1):
                sel = np.flatnonzero((c1 == ca) & (c2 == cb))
                if sel.size == 0:
                    continue
                x = cnt[sel]
                if ca == cb:
                    offd = b1[sel] != b2[sel]
                    pool = np.concatenate([x, x[offd]])            # upper triangle + diagonal, then the mirror
                    keep = int(sample * pool.sum())
                    drawn = rng.multivariate_hypergeometric(pool, keep, method="marginals") if keep < pool.sum() else pool
                    new[sel] = drawn[:x.size]
                else:
                    keep = int(sample * x.sum())
                    new[sel] = rng.multivariate_hypergeometric(x, keep, method="marginals") if keep < x.sum() else x
        cool = dict(h)
        nz = new > 0
        cool["bin1_id"], cool["bin2_id"], cool["count"] = b1[nz], b2[nz], new[nz]
        return DeviceCool(cool, self.dev)

    def coarsened(self, factor):
        """A DeviceCool of `factor` times the bin size, built on the device from this one's table (chromosight_amd/coarsen.py,
        cs_coarsen): what `cooler coarsen -k factor` writes -- every chromosome's bins regrouped `factor` at a time on their own,
        the stored pixels summed per coarse pixel, nothing mirrored.  The counts must be non-negative integers (ValueError
        otherwise).  The result has no weights (fine-bin weights mean nothing for coarse bins): balance it (balance.ice_balance +
        set_weights, or pipeline.open_cool(resolution=)).  factor 1 gives a table equal to this one, with its weights."""
        from .coarsen import coarsen_device
        return coarsen_device(self, factor)

    def merged(self, *others):
        """A DeviceCool over the pixel-wise sum of this table and `others` (DeviceCools over the same bins, resident on the same
        device), built on the device (chromosight_amd/merge.py, cs_merge_count / cs_merge_fill): what `cooler merge` writes --
        one pixel for every (bin1, bin2) stored in at least one source, the counts summed, nothing mirrored.  A pixel whose
        summed count is 0 is not stored.  The counts must be non-negative integers (ValueError otherwise, as for sources over
        different bins or devices, and for more than 64 of them).  The sum is exact, so the table is bitwise the same for every
        order of the sources, on every run and device.  The sources stay valid and untouched; the result has no weights (the sum
        of balanced tables is not balanced): balance it (balance.ice_balance + set_weights, or pipeline.open_cool([...])).
        Without `others` the result is a table equal to this one, with its weights."""
        from .merge import merge_device
        return merge_device([self, *others])

    def bins_of(self, chroms, positions):
        """Whole-genome bin of (chromosome name, base pair) pairs; -1 outside the genome
        (HicGenome.coords_to_bins, contacts_map.py:404-450, for fixed-size bins)."""
        ci = pd.Categorical(pd.Series(np.asarray(chroms, dtype=object)).astype(str), categories=list(self.names)).codes.astype(np.int64)
        local = np.asarray(positions, dtype=np.int64) // self.binsize
        sizes = np.diff(self.offsets)
        ok = (ci >= 0) & (local >= 0) & (local < sizes[np.maximum(ci, 0)])
        return np.where(ok, self.offsets[np.maximum(ci, 0)] + local, -1)

    def block_bins(self, ci):
        self._need_weights()
        s, e = int(self.offsets[ci]), int(self.offsets[ci + 1])
        return np.flatnonzero(~self.miss_host[s:e])


def detect_block(dcool, block, kernel_config, kernel, tsvd=None, coords=None, want_windows=True, raw=False, dev=None,
                 stream=None, all_gather=None, defer=False):
    """pattern_detector(full=True) on a staged block (cli/chromosight.py:601-614).  A block staged as a
    row window (stage_intra(rows=...)) is this rank's part of a sub-matrix split over several GPUs:
    `all_gather` exchanges the candidate pixels and the records (detect_split_on_device)."""
    kernel = np.asarray(kernel, dtype=np.float64)
    if min(block.shape) <= max(kernel.shape):
        return None, None
    _check_template(kernel)
    kspec = engine.KernelSpec(kernel, tsvd)
    block = block.full() if hasattr(block, "full") else block     # (the per-block entries read the float64 band themselves)
    if block.row_window is not None:
        if coords is not None or all_gather is None:
            raise ValueError("a row window of a block needs detect mode and an all_gather")
        return cid.detect_split_on_device(dev or dcool.dev, block.sig, block.shape, block.row_window, kspec,
                                          kernel_config, block.miss_row, block.miss_col, max_dist=block.max_dist,
                                          all_gather=all_gather, want_windows=want_windows, raw=raw, stream=stream)
    return cid.detect_on_device(dev or dcool.dev, block.sig, block.shape, kspec, kernel_config, block.miss_row,
                                block.miss_col, inter=block.inter, max_dist=block.max_dist, full=True, coords=coords,
                                want_windows=want_windows, raw=raw, stream=stream, defer=defer)


def _check_template(kernel):
    """normxcorr2's template check (detection.py:888-889).  It is what stops the reference when a 1-D pattern is
    iterated: the windows of intra maps carry NaN on the first sub-diagonals (detection.py:300-310), so does their
    pileup, and `kernel.std() > 0` is False for a template with NaN (tests/golden/iterations.npz: borders_error)."""
    if not (np.std(kernel) > 0):
        raise ValueError("Cannot have flat kernel.")


def detect_blocks(dcool, blocks, kernel_config, kernel, tsvd=None, raw=True, workers=4, batch=True, want_windows=True, defer=False,
                  dev=None, stream=None, merged=False, exclusive=True):
    """detect_block for every staged block of `blocks`; results in the order of `blocks`.  Banded intra blocks go to the
    device in ONE native call per template (1-D patterns: cs_detect_foci_batch; 2-D patterns: cs_detect_foci_blocks);
    what the library cannot batch (dense-staged short chromosomes, inter blocks, odd templates) goes block by block,
    several at a time (see _Workers).  defer=True: returns a callable that yields the results -- the native calls are
    done when detect_blocks returns, the acceptance rules (numpy on the returned records) run in the callable, so a
    caller can overlap them with the next template's device work (parallel.detect_genome).  dev / stream: another
    context and stream of the same GPU for the batched calls (templates scanned concurrently by several host threads).
    merged=True: when ONE native call covered every block, the result is the tuple (table of all blocks (k, 4), accepted
    records per block, windows or None) instead of the per-block list (the genome drivers concatenate the tables anyway).
    exclusive=False: other templates / patterns are being scanned on this GPU at the same time (parallel.detect_patterns)."""
    kernel = np.asarray(kernel, dtype=np.float64)
    bdev = dev or dcool.dev
    done = (lambda res: (lambda: res)) if defer else (lambda res: res)
    if any(min(b.shape) > max(kernel.shape) for b in blocks):
        _check_template(kernel)
    square = kernel.shape[0] == kernel.shape[1]
    one_d = kernel_config["max_dist"] == 0
    plain = raw and tsvd is None                             # the batch entries' own raw tables: deferred, merged on request
    if len(blocks) > 1 and batch and square and (plain or one_d):
        live = [k for k, b in enumerate(blocks) if min(b.shape) > max(kernel.shape)]
        banded = [k for k in live if blocks[k].is_band]
        kspec = engine.KernelSpec(kernel, tsvd)
        fin = None
        if len(banded) > 1 and plain:
            many = cid.detect_many_on_device if one_d else cid.detect_blocks_on_device
            extra = dict(raw=True) if one_d else dict(exclusive=exclusive)
            whole = merged and len(banded) == len(blocks)
            fin = many(bdev, [blocks[k] for k in banded], kspec, kernel_config, want_windows=want_windows, defer=True, stream=stream,
                       merged=whole, **extra)
            if fin is not None and whole:
                return fin if defer else fin()
        elif len(banded) > 1:
            # a truncated-SVD template, or tables as DataFrames (1-D patterns only): the same batch, accepted block by block in
            # the call (on the caller's context and stream: several host threads may be scanning templates side by side)
            res = cid.detect_many_on_device(bdev, [blocks[k] for k in banded], kspec, kernel_config, raw=raw, want_windows=want_windows,
                                            stream=stream)
            fin = None if res is None else (lambda: res)
        if fin is not None:
            # what the library cannot batch goes block by block
            rest = {k: detect_block(dcool, blocks[k], kernel_config, kernel, tsvd=tsvd, raw=raw, want_windows=want_windows, dev=dev,
                                    stream=stream)
                    for k in live if k not in banded}

            def finish():
                out = [(None, None)] * len(blocks)
                for k, r in zip(banded, fin()):
                    out[k] = r
                for k, r in rest.items():
                    out[k] = r
                return out

            return finish if defer else finish()
    if workers <= 1 or len(blocks) <= 1 or dev is not None:
        # (a caller that brought its own context and stream -- a template scanned beside others -- keeps every call on them:
        # that stream is the one that waited for the staging of the blocks)
        return done([detect_block(dcool, b, kernel_config, kernel, tsvd=tsvd, raw=raw, want_windows=want_windows, dev=dev, stream=stream)
                     for b in blocks])
    dcool.dev.sync()
    pool = dcool.workers(workers)

    # raw tables of banded intra blocks: the workers only run the native call; the acceptance rules are applied to all
    # their records in one go (numpy under the interpreter lock was a good part of a worker's time on a small block)
    deferred = raw and square and all(b.is_band and min(b.shape) > max(kernel.shape) for b in blocks)

    def one(block):
        dev, stream = pool.device()
        return detect_block(dcool, block, kernel_config, kernel, tsvd=tsvd, raw=raw, dev=dev, stream=stream,
                            want_windows=want_windows, defer=deferred)

    results = pool.map(one, blocks)
    if not deferred:
        return done(results)
    counts = [len(r[0]) for r in results]
    if sum(counts) == 0:
        return done([(None, None)] * len(blocks))
    rec = np.concatenate([r[0] for r in results])
    windows = np.concatenate([r[1] for r in results]) if want_windows else None
    return done(cid.accept_many(blocks, rec, windows, counts, engine.KernelSpec(kernel, tsvd), kernel_config, pvals=True))


def host_pileup():
    """True with CHROMOSIGHT_HIP_HOST_PILEUP=1: an iterated template's pileup is formed on the host from fetched windows
    (np.nansum over their count: np.nanmean) instead of on the device (pileup_blocks)."""
    return bool(os.environ.get("CHROMOSIGHT_HIP_HOST_PILEUP"))


def pileup_blocks(dcool, blocks, kernel_shape, blk, rows, cols, dev=None, stream=None):
    """Pileup of the windows of given pixels of staged blocks, reduced on the device (cs_pileup_blocks): position t is the
    block-local pixel (rows[t], cols[t]) of blocks[blk[t]] -- the (bin1, bin2) of a detect record of that block.  Returns
    (sum, cnt), (km, kn) arrays: per window pixel the sum of its non-NaN values over the positions (float64) and their number
    (int64); sum / cnt is the template `detect --iterations` continues with (cid.pileup_patterns of the same windows, summed
    in the fixed order of include/chromosight_hip.h instead of numpy's).  The windows are those of detect_blocks /
    quantify: nothing but the two small arrays leaves the device."""
    km, kn = (int(x) for x in kernel_shape)
    big = np.iinfo(np.int32).max // 2
    rows = np.clip(np.asarray(rows, dtype=np.int64), -big, big)
    cols = np.clip(np.asarray(cols, dtype=np.int64), -big, big)
    return engine.run_pileup_blocks(dev or dcool.dev, list(blocks), (km, kn), blk, rows, cols, stream=stream)


def _strip_reach(kernels):
    """The template side whose halo a row strip of a trans block needs for these templates: (reach - 1) // 2 rows cover the
    windows of the rows it owns, plus |kh - kw| for a non-square template (in full mode its score is read kh - kw rows away:
    detection._offset_scores)."""
    reach = 1
    for k in kernels:
        km, kn = np.shape(k)
        kh, kw = (km - 1) // 2, (kn - 1) // 2
        reach = max(reach, 2 * (kh + abs(kh - kw)) + 1)
    return reach


def _check_budget(inter_budget):
    if inter_budget is None:
        return INTER_BUDGET_DEFAULT
    if not inter_budget > 0:
        raise ValueError("inter_budget must be a positive number of bytes")
    return inter_budget


def _strip_common(block, kernel_config):
    return dict(inter=True, full=True, sym_upper=False, max_dist=None, missing_tol=kernel_config["max_perc_undetected"] / 100,
                mask_mode=MASK_BINS, miss_row=block.miss_row, miss_col=block.miss_col)


def detect_inter_block(dcool, ca, cb, kernel_config, kernel, tsvd=None, want_windows=True, inter_budget=None, reach=None, median=None,
                       stats=None):
    """detect_block(raw=True) of the trans block (ca, cb) without staging it whole: row strips of at most inter_budget bytes
    (plan_inter_strips), staged one at a time in the strip pool, each scanned only on the output tiles a stored pixel reaches
    (cs_csr_tile_occupancy -> cs_candidates_tiles); the strips' candidates are concatenated and labelled once (cs_label_foci),
    and each strip scores the foci whose row it owns (cs_quantify_pixels) -- the cut-merging of detection.detect_split_on_device
    with a local concatenation for its all-gather, so foci across a cut come out as from one piece.  Returns (table (k, 4),
    windows) or (None, None).  reach: template side of the halo (_strip_reach); median: the block's (inter_median).  stats: a
    dict that receives strips / tiles / tiles_listed."""
    kernel = np.asarray(kernel, dtype=np.float64)
    budget = _check_budget(inter_budget)
    n_r, n_c = dcool._inter_geometry(ca, cb)[4:6]
    if min(n_r, n_c) <= max(kernel.shape):
        return None, None
    _check_template(kernel)
    kspec = engine.KernelSpec(kernel, tsvd)
    km, kn = kspec.km, kspec.kn
    reach = max(reach or 1, _strip_reach([kernel]))
    strips = plan_inter_strips(n_r, n_c, budget, (reach - 1) // 2)
    if median is None:
        median = dcool.inter_median(ca, cb)
    dev = dcool.dev
    tiles_x = -(-n_c // 64)
    n_tiles = n_listed = 0
    rows_l, cols_l, vals_l = [], [], []
    held = None
    for rows in strips:
        held = None                                      # (the pool's buffer is restaged below)
        blk = dcool.stage_inter(ca, cb, rows=rows, largest_kernel=reach, median=median)
        tiles, nt = engine.run_tile_occupancy(dev, blk.view, blk.view_row0, km, kn, rows, n_c)
        n_tiles += tiles_x * -(-(rows[1] - rows[0]) // 64)
        n_listed += nt
        r, c, v = engine.run_candidates_tiles(dev, blk.sig, (n_r, n_c), kspec, rows, tiles, nt, pearson=kernel_config["pearson"],
                                              lo_diag=-(n_r - 1), hi_diag=n_c - 1, **_strip_common(blk, kernel_config))
        rows_l.append(r)
        cols_l.append(c)
        vals_l.append(v)
        held = blk
    if stats is not None:
        stats.update(strips=len(strips), tiles=n_tiles, tiles_listed=n_listed)
    cand_r, cand_c, cand_v = np.concatenate(rows_l), np.concatenate(cols_l), np.concatenate(vals_l)
    if cand_r.size == 0:
        return None, None
    f_rows, f_cols, f_size = engine.run_label_foci(dev, (n_r, n_c), cand_r, cand_c, cand_v, min_size=2, diag_only=0)
    if f_rows.size == 0:
        return None, None
    rec = np.zeros(f_rows.size, dtype=FOCUS_DTYPE)
    windows = np.zeros((f_rows.size, km, kn)) if want_windows else None
    conv = [np.zeros(f_rows.size, dtype=np.int64), np.zeros(f_rows.size, dtype=np.int64), np.zeros(f_rows.size)] if km != kn else None
    for rows in strips:
        mine = (f_rows >= rows[0]) & (f_rows < rows[1])
        if not mine.any():
            continue
        blk = held if held is not None and held.row_window == tuple(rows) else \
            dcool.stage_inter(ca, cb, rows=rows, largest_kernel=reach, median=median)
        common = _strip_common(blk, kernel_config)
        r, w = engine.run_quantify_pixels(dev, blk.sig, (n_r, n_c), kspec, f_rows[mine], f_cols[mine], want_windows=want_windows,
                                          **common)
        r["focus_size"] = f_size[mine]
        rec[mine] = r
        if want_windows:
            windows[mine] = w
        if conv is not None:
            rr_m, cc_m = r["bin1"].astype(np.int64), r["bin2"].astype(np.int64)
            for k, part in enumerate(cid._offset_scores(dev, blk.sig, (n_r, n_c), kspec, rr_m, cc_m, dict(common, stream=None))):
                conv[k][mine] = part
        held = blk
    rr, cc = rec["bin1"].astype(np.int64), rec["bin2"].astype(np.int64)
    return cid._accept_records(rec, windows, rr, cc, "detect", (n_r, n_c), kspec, kernel_config, inter=True, max_dist=None, full=True,
                               raw=True, conv=None if conv is None else tuple(conv))


def _row_groups(rows, n_r, n_c, budget, halo):
    """Groups of the (sorted, unique) rows that hold quantify positions: each (a, b) is staged as one strip (rows a - halo ..
    b + halo - 1) within `budget` bytes and below 2^31 elements."""
    ld = _inter_ld(n_c)
    max_rows = min(int(budget) // (ld * 8), _MAX_STRIP_ELEMENTS // ld)
    if max_rows < 1 + 2 * halo and max_rows < n_r:
        raise ValueError(f"inter_budget of {int(budget)} bytes cannot hold one row and its halo of {halo} rows of a block of {n_c} columns")
    groups, a = [], None
    for r in rows.tolist():
        if a is not None:
            lo, hi = _strip_rows(n_r, (a, r + 1), halo)
            if hi - lo <= max_rows:
                b = r + 1
                continue
            groups.append((a, b))
        a, b = r, r + 1
    if a is not None:
        groups.append((a, b))
    return groups


def quantify_inter_block(dcool, ca, cb, coords, kernels, kernel_config, tsvd=None, inter_budget=None, median=None):
    """The positions `coords` ((n, 2) block-local rows and columns) of the trans block (ca, cb) scored with every template, as
    quantify scores them on the whole block, staging only the rows that hold a position (plus the halo), grouped into strips
    within inter_budget bytes.  Returns, per template, (table (n, 4): bin1, bin2, score, pvalue; windows (n, km, kn))."""
    budget = _check_budget(inter_budget)
    kernels = [np.asarray(k, dtype=np.float64) for k in kernels]
    km, kn = kernels[0].shape
    n_r, n_c = dcool._inter_geometry(ca, cb)[4:6]
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    n = coords.shape[0]
    out = [(np.full((n, 4), np.nan), np.full((n, km, kn), np.nan)) for _ in kernels]
    if n == 0 or min(n_r, n_c) <= max(km, kn):
        return out
    reach = _strip_reach(kernels)
    halo = (reach - 1) // 2
    if median is None:
        median = dcool.inter_median(ca, cb)
    row_of = np.clip(coords[:, 0], 0, n_r - 1)
    batch = tsvd is None and not os.environ.get("CHROMOSIGHT_HIP_NO_QUANTIFY_BATCH")
    if batch:
        for k in kernels:
            _check_template(k)
    specs = [engine.KernelSpec(k, tsvd) for k in kernels]
    for a, b in _row_groups(np.unique(row_of), n_r, n_c, budget, halo):
        sel = np.flatnonzero((row_of >= a) & (row_of < b))
        blk = dcool.stage_inter(ca, cb, rows=(a, b), largest_kernel=reach, median=median)
        res = cid.quantify_many_on_device(dcool.dev, [blk], specs, kernel_config, [coords[sel]]) if batch else None
        for t, kspec in enumerate(specs):
            if res is not None:
                table, wins = res[t]
            else:
                table, wins = cid.detect_on_device(dcool.dev, blk.sig, blk.shape, kspec, kernel_config, blk.miss_row, blk.miss_col,
                                                   inter=True, max_dist=None, full=True, coords=coords[sel].copy(), raw=True)
            out[t][0][sel] = table
            out[t][1][sel] = wins
    return out


def detect_blocks_templates(dcool, blocks, kernel_config, kernels, want_windows=False, dev=None, stream=None, begin_only=False):
    """A 1-D pattern's templates (one size: the three borders templates, the one hairpins template) on banded intra blocks with ONE native call
    (cs_detect_foci_batch_templates) instead of one launch chain per template.  Returns a callable that yields, per template,
    the merged result of detect_blocks (table of all blocks, accepted records per block, windows) -- the native call is done
    when this returns, the acceptance rules run in the callable -- or None when the entry does not apply.
    begin_only=True: the chain is only enqueued on (dev, stream) when this returns; the callable waits for it first."""
    kernels = [np.asarray(k, dtype=np.float64) for k in kernels]
    if kernel_config["max_dist"] != 0 or len(kernels) < 1 or len(kernels) > 4 or len(blocks) < 1:
        return None
    if any(k.shape != kernels[0].shape or k.shape[0] != k.shape[1] for k in kernels):
        return None
    if not all(b.is_band and min(b.shape) > max(kernels[0].shape) for b in blocks):
        return None
    for k in kernels:
        _check_template(k)
    return cid.detect_many_on_device(dev or dcool.dev, blocks, [engine.KernelSpec(k) for k in kernels], kernel_config,
                                     want_windows=want_windows, raw=True, stream=stream, defer=True, merged=True, begin_only=begin_only)


def with_win_size(kernel_config, win_size):
    """--win-size of the reference's CLI (cli/chromosight.py:365-370, 689-695): every template of the
    config resized to win_size x win_size (odd), "auto" / None keeps the config's own sizes."""
    if win_size is None or win_size == "auto":
        return kernel_config
    win_size = int(win_size)
    if not win_size % 2:
        raise ValueError("--win-size must be odd")
    cfg = dict(kernel_config)
    cfg["kernels"] = [preproc.resize_kernel(np.asarray(k, dtype=np.float64), factor=win_size / np.shape(k)[0], quiet=True)
                      for k in kernel_config["kernels"]]
    return cfg


def sub_matrices(dcool, inter):
    """(chrom a, chrom b) of every sub-matrix in the reference's order (contacts_map.py:274-312)."""
    return [(a, b) for a in range(dcool.n_chrom) for b in range(dcool.n_chrom) if a == b or (a < b and inter)]


def _resolution_factor(resolution, binsize):
    """open_cool / open_pairs: the coarsening factor of `resolution` (None: 1) over a table of `binsize` bp."""
    if resolution is None:
        return 1
    if isinstance(resolution, bool) or int(resolution) != resolution or resolution <= 0 or int(resolution) % binsize:
        raise ValueError(f"resolution {resolution} is not a positive multiple of the file's bin size {binsize}")
    return int(resolution) // binsize


def _raw_weights(w):
    return np.where(np.isfinite(np.asarray(w, dtype=np.float64)), 1.0, np.nan)


def _coarsen_and_balance(dcool, factor, balance, norm, inter, n_mads):
    """The tail open_cool and open_pairs share: coarsen the resident table by `factor` (> 1), then, for a table that counts as one
    without stored weights (`balance`), ICE on the device with the reference's arguments -- the weights themselves, or 1.0 / NaN on
    its detectable bins for norm="raw"."""
    if factor > 1:
        dcool = dcool.coarsened(factor)
    if balance:
        from .balance import ice_balance
        weight, _ = ice_balance(dcool, cis_only=not inter, mad_max=n_mads, ignore_diags=2, min_nnz=10, max_iters=200)
        dcool.set_weights(_raw_weights(weight) if norm == "raw" else weight)
    return dcool


def _is_path(source):
    return isinstance(source, (str, bytes)) or hasattr(source, "__fspath__")


def _check_norm(norm):
    if norm not in ("auto", "raw", "force"):
        raise ValueError("norm must be one of: auto, raw, force")


class DeviceDecodeRefused(ValueError):
    """The file does not qualify for the device decode (DeviceCool.from_cool_file, open_cool(decode="device"))."""


AUTO_DECODE_ON_DEVICE = True        # what open_cool(decode="auto") does with a file that qualifies (tools/time_cool_decode.py)
_PIXEL_COLUMNS = ("bin1_id", "bin2_id", "count")


def _route(name, value, env, auto_on_device):
    """Where a loader does its work: the argument `name` = `value` under the environment variable `env` and the measured default
    for "auto" -- "auto" (the device, the host for a file it refuses), "host" or "device"."""
    if value not in ("auto", "host", "device"):
        raise ValueError(f"{name} must be one of: auto, host, device")
    if os.environ.get(env, "") not in ("", "0"):
        if value == "device":
            raise ValueError(f"{name}='device' while {env} forces the host route")
        return "host"
    return value if value != "auto" or auto_on_device else "host"


def _decode_route(decode):
    """open_cool's `decode`: _route."""
    return _route("decode", decode, "CHROMOSIGHT_HIP_HOST_DECODE", AUTO_DECODE_ON_DEVICE)


class DevicePairsRefused(ValueError):
    """A line of the file is outside what the device parses (DeviceCool.from_pairs_file, open_pairs(parse="device"))."""


AUTO_PARSE_ON_DEVICE = True         # what open_pairs(parse="auto") does with a .pairs file (tools/time_pairs_parse.py: the device
                                    # route is faster end to end on both inputs, profiles/pairs_parse_time.json)


def _parse_route(parse):
    """open_pairs' `parse`: _route."""
    return _route("parse", parse, "CHROMOSIGHT_HIP_HOST_PARSE", AUTO_PARSE_ON_DEVICE)


class DeviceInflateRefused(ValueError):
    """The .gz is not what bgzip writes (DeviceCool.from_pairs_file, open_pairs(inflate="device"))."""


AUTO_INFLATE_ON_DEVICE = True       # what open_pairs(inflate="auto") does with a bgzip-compressed .pairs.gz (tools/time_pairs_bgzf.py: on
                                    # both inputs the device route lies below the host inflate of the commit before by far more than
                                    # that one's run-to-run spread, profiles/pairs_bgzf_time.json)


def _inflate_route(inflate):
    """open_pairs' `inflate`: _route."""
    return _route("inflate", inflate, "CHROMOSIGHT_HIP_HOST_INFLATE", AUTO_INFLATE_ON_DEVICE)


def device_decode_refusal(indexes, max_chunk_bytes):
    """Why the pixel columns of a file are not decoded on the device, or None when they are.  indexes: name -> hdf5_lite.ChunkIndex
    of pixels/bin1_id, bin2_id and count (None: not a chunked dataset); max_chunk_bytes: engine.inflate_max_chunk_bytes()."""
    for name in _PIXEL_COLUMNS:
        idx = indexes.get(name)
        if idx is None:
            return f"pixels/{name} is not a chunked dataset"
        if idx.dtype.kind != "i" or idx.dtype.itemsize not in (4, 8):
            return f"pixels/{name} holds {idx.dtype}, not int32 or int64"
        stage = 0
        for fid, _ in idx.filters:
            at = {2: 1, 1: 2, 3: 3}.get(int(fid), 0)
            if at <= stage:
                return f"pixels/{name} has filter {fid}" if at == 0 else f"pixels/{name} has its filters in another order than shuffle, gzip, Fletcher-32"
            stage = at
        if idx.chunk < 1 or idx.chunk * idx.dtype.itemsize > max_chunk_bytes:
            return f"pixels/{name} has chunks of {idx.chunk * idx.dtype.itemsize} bytes, the device decodes up to {max_chunk_bytes}"
    if indexes["bin1_id"].dtype != indexes["bin2_id"].dtype:
        return "pixels/bin1_id and pixels/bin2_id differ in type"
    if len({indexes[name].length for name in _PIXEL_COLUMNS}) != 1:
        return "the pixel columns differ in length"
    return None


def _device_cool_from_file(uri, balance, dev, pick_weight):
    """DeviceCool.from_cool_file; pick_weight(cool) -> the weights to set, from everything of the file but its pixels."""
    from . import hdf5_lite, io as cio
    path, group = cio.split_uri(uri)
    if os.environ.get("CHROMOSIGHT_H5DUMP_ONLY"):
        raise DeviceDecodeRefused(f"{uri}: CHROMOSIGHT_H5DUMP_ONLY sends every file through the HDF5 command line tool")
    dev = dev or get_device()
    try:
        with hdf5_lite.File(path) as f:
            indexes = {}
            for name in _PIXEL_COLUMNS:
                try:
                    indexes[name] = f.chunk_index(f"{group}/pixels/{name}")
                except hdf5_lite.Hdf5Unsupported:
                    indexes[name] = None
            reason = device_decode_refusal(indexes, engine.inflate_max_chunk_bytes())
            if reason:
                raise DeviceDecodeRefused(f"{uri}: {reason}")
            cool = cio._read_cool_geometry(f, path, group, balance, None)
            with dev.lock:
                columns = {name: engine.run_inflate_chunks(dev, f.buf, indexes[name])[0] for name in _PIXEL_COLUMNS}
    except hdf5_lite.Hdf5Unsupported as exc:
        raise DeviceDecodeRefused(f"{uri}: {exc}") from None
    except NotImplementedError as exc:              # CS_ERR_UNSUPPORTED: a limit of the kernel the rule above does not know
        raise DeviceDecodeRefused(f"{uri}: {exc}") from None
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    n_bins, nnz = int(off[-1]), int(indexes["count"].length)
    with dev.lock:
        res = engine.run_table_from_columns(dev, columns["bin1_id"], columns["bin2_id"], columns["count"], nnz, n_bins)
    if not res["ids_ok"]:
        raise DeviceDecodeRefused(f"{uri}: bin ids outside [0, {n_bins})")
    if not res["sorted"]:
        raise DeviceDecodeRefused(f"{uri}: the pixel table is not strictly sorted by (bin1, bin2)")
    del columns
    # (io._load narrows the ids of a table that has pixels when all are below 2^31; here every id is below n_bins)
    ids = np.int32 if nnz and n_bins <= 2 ** 31 else indexes["bin1_id"].dtype.type
    return DeviceCool._from_table(
        dev, names=cool["chrom_names"], offsets=off, binsize=cool["binsize"], bin_start=cool.get("bin_start"),
        bin_end=cool.get("bin_end"), indptr=res["indptr"], indices=res["indices"], data=res["data"], nnz=nnz, val_dtype=res["val_dtype"],
        counts_exact=res["val_dtype"] is np.float32 and (nnz == 0 or res["count_min"] >= 0), upper=res["upper"],
        weight=pick_weight(cool), host_dtypes=(ids, ids, indexes["count"].dtype.type))


def open_cool(uri_or_cool, *, norm="auto", inter=False, n_mads=5, balance="weight", dev=None, resolution=None, decode="auto"):
    """A .cool (path, `file.mcool::/resolutions/<binsize>`, or a decoded dictionary) resident on the device with the
    weights the reference's HicGenome.normalize gives it (contacts_map.py:182-229):

    - norm="auto": the stored `bins/<balance>` column when the file has one, else ICE on the device;
    - norm="force": ICE on the device even when the file has weights;
    - norm="raw": raw counts; the detectable bins are those of the stored weights, or of ICE when there are none
      (weights 1.0 on them, NaN elsewhere).

    ICE runs with the reference's arguments (cooler.balance_cooler: cis_only = not inter, mad_max = n_mads, ignore_diags=2,
    min_nnz=10, max_iters=200; chromosight_amd/balance.py).  Unlike the reference, the new weights are NOT written back
    into the input file.  The result goes to detect / quantify / detect_to_files and the parallel drivers.

    A list or tuple of them (replicates over the same bins): each is read and uploaded, and all are merged on the device
    (DeviceCool.merged: what `cooler merge` writes, which the reference expects to have been run beforehand).  The sum of
    balanced tables is not balanced, so the merged table counts as a file without stored weights: ICE on it for "auto" and
    "force", its detectable bins with weights 1.0 / NaN for "raw".  The sources are released once merged; the peak in HBM is
    sources + result.  A list of one behaves exactly as its element alone.  The merge is exact, so every rank of a parallel run
    that merges its own copies gets the same table and the same weights.

    resolution: None, or the bin size in base pairs to work at, a positive multiple of the file's (ValueError otherwise).  A
    larger one coarsens the uploaded (and, for a list, merged) table on the device (DeviceCool.coarsened: what `cooler coarsen`
    writes, which the reference expects to have been run beforehand); the coarse table has no stored weights, so `norm` applies as
    to a file without any: ICE on the coarse table for "auto" and "force", its detectable bins with weights 1.0 / NaN for "raw".
    The file's own bin size: as without the argument.  Every rank of a parallel run that coarsens its own copy gets the same table
    and weights.

    decode: where the pixel columns of a file are decoded.  "auto": on the device (DeviceCool.from_cool_file) when the file
    qualifies -- hdf5_lite reads it, its pixel columns are chunked int32 / int64 datasets with filters among shuffle, gzip and
    Fletcher-32, no chunk decodes to more than engine.inflate_max_chunk_bytes(), and the table is strictly sorted -- and on the host,
    as before, when it does not.  "host": always on the host; CHROMOSIGHT_HIP_HOST_DECODE=1 in the environment does the same.
    "device": on the device, DeviceDecodeRefused (a ValueError) for a file that does not qualify and ValueError for a dictionary,
    which is decoded already.  Both routes give the same table, bit for bit."""
    _check_norm(norm)
    route = _decode_route(decode)
    sources = list(uri_or_cool) if isinstance(uri_or_cool, (list, tuple)) else [uri_or_cool]
    if not sources:
        raise ValueError("open_cool got an empty list: at least one .cool is needed")
    many = len(sources) > 1
    raw = _raw_weights if norm == "raw" else (lambda w: w)

    def pick_weight(cool):
        # a coarsened table has no stored weights (the fine bins' mean nothing for the coarse ones), nor has a merged one
        factor = _resolution_factor(resolution, int(cool["binsize"]))
        weight = None if norm == "force" or factor > 1 or many else cool.get("weight")
        return None if weight is None else raw(weight)

    def open_one(source):
        if not _is_path(source):
            if route == "device":
                raise ValueError("decode='device' takes files: a dictionary is a decoded table already")
            cool = dict(source)
        else:
            if route != "host":
                try:
                    return _device_cool_from_file(source, balance, dev, pick_weight)
                except DeviceDecodeRefused:
                    if route == "device":
                        raise
            from . import io as cio
            cool = cio._read_cool(source, balance)
        cool["weight"] = pick_weight(cool)
        return DeviceCool(cool, dev)

    parts = []
    while sources:
        parts.append(open_one(sources.pop(0)))          # (a source's host columns are released once it is uploaded)
    dcool = parts[0].merged(*parts[1:]) if many else parts[0]
    del parts                                       # the sources' HBM is released here
    factor = _resolution_factor(resolution, dcool.binsize)
    return _coarsen_and_balance(dcool, factor, many or not dcool.has_weights, norm, inter, n_mads)


def open_pairs(path_or_chunks, binsize, chromsizes=None, *, zero_based=False, norm="auto", inter=False, n_mads=5, dev=None,
               resolution=None, parse="auto", piece_bytes=None, inflate="auto"):
    """Read pairs (a 4DN .pairs / .pairs.gz path, or an iterable of (chrom1, pos1, chrom2, pos2) chunks of arrays as
    io.read_pairs yields them) binned at `binsize` bp on the device (DeviceCool.from_pairs: what `cooler cload pairs` writes, which
    the reference expects to have been run beforehand) and given weights as open_cool gives them to a file without stored ones:
    ICE on the device for norm="auto" and "force", its detectable bins with weights 1.0 / NaN for "raw".  chromsizes: ordered
    name -> length in bp; None takes the #chromsize: lines of the file (a path only).  zero_based: the positions are taken as they
    are instead of 1-based.  resolution: None, or a positive multiple of `binsize` to coarsen the binned table to first, as in
    open_cool.  `.dropped` is the number of pairs left out for a chromosome that is not in `chromsizes`.  The binning is exact, so
    every rank of a parallel run that bins its own copy gets the same table and weights.
    parse, piece_bytes: where the text of a file becomes columns, as in DeviceCool.from_pairs_file ("auto", "host" or "device"; both
    routes give the same table, bit for bit).  Chunks are parsed already: anything but "auto" with them is a ValueError.
    inflate: where a .pairs.gz becomes text, as in DeviceCool.from_pairs_file ("auto", "host", or "device" for a file bgzip wrote);
    anything but "auto" with chunks is a ValueError."""
    _check_norm(norm)
    geometry_binsize = int(binsize)
    factor = _resolution_factor(resolution, geometry_binsize)
    chunks = path_or_chunks
    if _is_path(chunks):                # (from_pairs_file checks `parse`)
        dcool = DeviceCool.from_pairs_file(chunks, geometry_binsize, chromsizes, zero_based=zero_based, parse=parse,
                                           piece_bytes=piece_bytes, dev=dev, inflate=inflate)
    elif parse != "auto":
        raise ValueError(f"parse={parse!r} takes files: chunks are parsed columns already")
    elif inflate != "auto":
        raise ValueError(f"inflate={inflate!r} takes files: chunks are parsed columns already")
    elif chromsizes is None:
        raise ValueError("open_pairs needs chromsizes for pairs that do not come from a file")
    else:
        dcool = DeviceCool.from_pairs(chunks, chromsizes, geometry_binsize, zero_based=zero_based, dev=dev)
    dropped = dcool.dropped
    dcool = _coarsen_and_balance(dcool, factor, True, norm, inter, n_mads)
    dcool.dropped = dropped
    return dcool


def detect(cool, kernel_config, tsvd=None, smooth=False, band_dtype=np.float64, inter=False, subsample=None, seed=0,
           return_windows=False, win_size=None, inter_budget=None, sampler="numpy", shard=None):
    """`chromosight detect` (balanced matrix) on a decoded cool (dict) or a DeviceCool; options
    --inter, --smooth-trend, --tsvd, --subsample (seeded), --iterations through the config.  Every
    block is staged once in HBM (distance law, detrend, band / median scaling) and stays resident
    across templates and iterations; each (block, template) is one native call.
    Returns the output table (same columns and row order as the reference's <prefix>.tsv); with
    return_windows also the windows of its rows (what the reference saves as <prefix>.json / .npy).
    With inter, the trans blocks are not resident: each is scanned in row strips of at most inter_budget bytes
    (default INTER_BUDGET_DEFAULT) by detect_inter_block, one block at a time.
    sampler: how --subsample draws, "numpy" (the host path) or "device" (DeviceCool.subsampled).
    shard: parallel.DetectShard, with inter only -- the sub-matrices (intra blocks and trans blocks, in strips) are dealt to the
    ranks, the per-block tables (and windows) are all-gathered after every template and iteration, and every rank returns
    the single-process result (parallel.detect_inter_genome)."""
    budget = _check_budget(inter_budget)
    kernel_config = with_win_size(kernel_config, win_size)
    if shard is not None:
        if not inter:
            raise ValueError("detect(shard=...) runs the --inter route only; intra-only sharding is parallel.detect_genome")
        shard.check(kernel_config)
    dcool = cool if isinstance(cool, DeviceCool) else DeviceCool(cool)
    if subsample is not None:
        dcool = dcool.subsampled(subsample, seed=seed, inter=inter, sampler=sampler)
    binsize = dcool.binsize
    off = dcool.offsets
    names = dcool.names
    n_chrom = dcool.n_chrom
    max_dist = max(kernel_config["max_dist"] // binsize, 1)
    largest = max(np.shape(k)[0] for k in kernel_config["kernels"])
    if not inter and not return_windows and np.dtype(band_dtype) == np.float64 and dcool.upper and hasattr(dcool, "view_for"):
        # ONE orchestration: the intra-chromosomal blocks of a plain `detect` go through the genome drivers bench.py times
        # (parallel.genome_step: blocks staged by one native call, batched chains, and -- for the configurations a StepPlan covers,
        # chromosight_amd/plan.py -- every call after the first on this DeviceCool as one native call list); the per-block
        # machinery below keeps --inter and the runs that return windows.
        from . import parallel
        # (local: `detect` is this process's call -- under an initialised process group it neither shards nor gathers; the sharded
        # driver is parallel.detect_genome / genome_step)
        rec = parallel.genome_step(dcool, [kernel_config], tsvd=tsvd, local=True, smooth=smooth)[0]
        if rec.shape[0] == 0:
            return pd.DataFrame(columns=OUTPUT_COLUMNS)
        first = np.asarray(off, dtype=np.int64)[rec[:, 0].astype(np.int64)]
        coords = {"bin1": rec[:, 1].astype(np.int64) + first, "bin2": rec[:, 2].astype(np.int64) + first, "score": rec[:, 3],
                  "pvalue": rec[:, 4], "kernel_id": rec[:, 5].astype(np.int64), "iteration": rec[:, 6].astype(np.int64)}
        return postprocess(coords, kernel_config, binsize, off, names, dcool.bin_start, dcool.bin_end)
    pairs = sub_matrices(dcool, inter)
    # this rank's sub-matrices (indices into pairs, in pairs order): all of them without a shard
    units = list(range(len(pairs))) if shard is None else shard.select(pairs, np.diff(off), max_dist, largest)
    own = [pairs[u] for u in units]
    intra = dict(zip([a for a, b in own if a == b],
                     dcool.stage_blocks([a for a, b in own if a == b], max_dist, largest, smooth=smooth, band_dtype=band_dtype)))
    # trans blocks: staged strip by strip for every template and iteration (detect_inter_block), scaled by their median
    trans = [(a, b) for a, b in own if a != b]
    medians = {pair: dcool.inter_median(*pair) for pair in trans}
    reach = _strip_reach(kernel_config["kernels"])
    blocks = [intra[a] for a, b in own if a == b]
    all_coords, all_windows = [], []
    for kernel_id, kernel in enumerate(kernel_config["kernels"]):
        for it in range(kernel_config["max_iterations"]):
            tables, windows = [], []
            # windows feed the next iteration's template and the optional output; otherwise they stay on the device
            need_windows = return_windows or it + 1 < kernel_config["max_iterations"]
            cis = iter(detect_blocks(dcool, blocks, kernel_config, kernel, tsvd=tsvd, raw=True, want_windows=need_windows) if blocks else [])
            results = [next(cis) if a == b else
                       detect_inter_block(dcool, a, b, kernel_config, kernel, tsvd=tsvd, want_windows=need_windows, inter_budget=budget,
                                          reach=reach, median=medians[(a, b)])
                       for a, b in own]
            done = units
            if shard is not None:
                # every rank issues this exchange, whatever it owns or found: afterwards the tables (and windows) of ALL units, in
                # pairs order -- the list the single process builds
                done, results = shard.merge(units, results, np.shape(kernel), need_windows)
            for (ca, cb), (tab, win) in zip([pairs[u] for u in done], results):
                if tab is None or len(tab) == 0:
                    continue
                tab[:, 0] += int(off[ca])
                tab[:, 1] += int(off[cb])
                tables.append(tab)
                windows.append(win)
            if not tables:
                break
            rec = np.concatenate(tables, axis=0)
            all_coords.append({"bin1": rec[:, 0].astype(np.int64), "bin2": rec[:, 1].astype(np.int64), "score": rec[:, 2],
                               "pvalue": rec[:, 3], "kernel_id": np.full(len(rec), kernel_id, dtype=np.int64),
                               "iteration": np.full(len(rec), it, dtype=np.int64)})
            if need_windows:
                kernel_windows = np.concatenate(windows, axis=0)
                all_windows.append(kernel_windows)
                kernel = cid.pileup_patterns(kernel_windows)
    if trans:
        dcool._strips.release()
    if not all_coords:
        empty = pd.DataFrame(columns=OUTPUT_COLUMNS)
        return (empty, np.zeros((0,) + np.shape(kernel_config["kernels"][0]))) if return_windows else empty
    coords = {k: np.concatenate([c[k] for c in all_coords]) for k in all_coords[0]}
    # windows of different templates may differ in size only across configs, never inside one
    windows = np.concatenate(all_windows, axis=0) if return_windows else None
    return postprocess(coords, kernel_config, binsize, off, names, dcool.bin_start, dcool.bin_end, windows=windows)


def detect_to_files(cool, kernel_config, prefix, win_fmt="json", dec=10, **options):
    """detect + the two files `chromosight detect` leaves behind (cli/chromosight.py:873-881):
    <prefix>.tsv and <prefix>.json | .npy.  Returns the table.  With shard=parallel.DetectShard() (and inter=True) under a
    launcher, only rank 0 should call this -- two ranks would write the same files --, every other rank calls
    parallel.detect_inter_genome with the same options (each rank takes part in every exchange)."""
    from . import io as cio
    cio.check_prefix_dir(prefix)
    table, windows = detect(cool, kernel_config, return_windows=True, **options)
    cio.write_patterns(table, prefix, dec=dec)
    cio.save_windows(windows, prefix, fmt=win_fmt)
    return table


def postprocess(coords, kernel_config, binsize, off, names, bin_start, bin_end, windows=None):
    """cmd_detect after the per-block loop (cli/chromosight.py:806-871): neighbour removal, bins ->
    genomic coordinates, min_dist and NaN-p filters, Benjamini-Hochberg q-values, column order.
    `coords`: DataFrame or dict of columns bin1, bin2, score, pvalue, kernel_id, iteration.
    `windows` (one per row of coords) are filtered alongside and returned as a second value.
    Column arithmetic is plain numpy and the table is built once (pandas' per-column inserts cost more
    than the detection itself on a small genome)."""
    col = {k: np.asarray(coords[k]) for k in ("bin1", "bin2", "score", "pvalue", "kernel_id", "iteration")}
    b1 = col["bin1"].astype(np.int64, copy=False)
    b2 = col["bin2"].astype(np.int64, copy=False)
    separation = max(int(kernel_config["min_separation"] // binsize), 1)
    sel = np.flatnonzero(cid.remove_neighbours_arrays(b1, b2, col["score"], win_size=separation))
    # bins -> genomic coordinates
    bin_chrom = np.repeat(np.arange(len(names)), np.diff(off))
    b1, b2 = b1[sel], b2[sel]
    c1, c2 = bin_chrom[b1], bin_chrom[b2]
    bin_start, bin_end = np.asarray(bin_start), np.asarray(bin_end)
    s1, s2 = bin_start[b1], bin_start[b2]
    pval = col["pvalue"][sel].astype(np.float64, copy=False)
    too_close = (c1 == c2) & (np.abs(s2 - s1) < kernel_config["min_dist"])
    keep = ~too_close & ~np.isnan(pval)
    sel, b1, b2, c1, c2, pval = sel[keep], b1[keep], b2[keep], c1[keep], c2[keep], pval[keep]
    name_arr = np.asarray(names, dtype=object)
    table = pd.DataFrame({
        "chrom1": name_arr[c1], "start1": bin_start[b1], "end1": bin_end[b1],
        "chrom2": name_arr[c2], "start2": bin_start[b2], "end2": bin_end[b2],
        "bin1": b1, "bin2": b2, "kernel_id": col["kernel_id"][sel], "iteration": col["iteration"][sel],
        "score": col["score"][sel], "pvalue": pval, "qvalue": fdr_correction(pval)}, columns=OUTPUT_COLUMNS)
    if windows is not None:
        return table, windows[sel]
    return table


def quantify(cool, positions, kernel_config, inter=False, tsvd=None, subsample=None, seed=0, smooth=False,
             max_dist_bp=None, win_size=None, shard=None, inter_budget=None, sampler="numpy"):
    """`chromosight quantify` (cli/chromosight.py:264-470): score the given 2-D positions with every
    template of the config and keep, per position, the row the reference keeps (sorted by score,
    last of each (chrom1, start1, chrom2, start2) group).  `positions`: DataFrame with chrom1, start1,
    end1, chrom2, start2, end2.  Returns (table in the reference's output order and columns, windows).
    shard: parallel.QuantifyShard -- the sub-matrices are dealt to the ranks (parallel.quantify_genome).
    With inter (with a shard or without), a trans block is never staged whole: only the rows that hold a position, plus the
    halo, in strips of at most inter_budget bytes (quantify_inter_block).  sampler: how --subsample draws, "numpy" or "device"
    (DeviceCool.subsampled)."""
    budget = _check_budget(inter_budget)
    dcool = cool if isinstance(cool, DeviceCool) else DeviceCool(cool)
    if subsample is not None:
        dcool = dcool.subsampled(subsample, seed=seed, inter=inter, sampler=sampler)
    cfg = dict(with_win_size(kernel_config, win_size))
    bed2d = positions.loc[:, ["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].reset_index(drop=True).copy()
    furthest = np.max(bed2d.start2 - bed2d.start1)
    cfg["max_dist"] = min(furthest, dcool.n_bins * dcool.binsize)       # scan up to the furthest pattern
    if max_dist_bp is not None:
        cfg["max_dist"] = int(max_dist_bp)                              # (tests: pin the scanning distance)
    cfg["min_dist"] = 0
    kernels = [np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]
    km, kn = kernels[0].shape
    max_dist = int(max(cfg["max_dist"] // dcool.binsize, 1))        # (a numpy integer from the positions: ctypes takes ints)
    largest = max(k.shape[0] for k in kernels)
    # chromosome of every position, once (the four bin lookups below share it); HicGenome.coords_to_bins
    # (contacts_map.py:404-450): -1 where the genome has no such bin
    c1 = pd.Categorical(bed2d.chrom1.astype(str), categories=list(dcool.names)).codes.astype(np.int64)
    c2 = pd.Categorical(bed2d.chrom2.astype(str), categories=list(dcool.names)).codes.astype(np.int64)
    sizes = np.diff(dcool.offsets)

    def bins(codes, bp):
        local = np.asarray(bp, dtype=np.int64) // dcool.binsize
        ok = (codes >= 0) & (local >= 0) & (local < sizes[np.maximum(codes, 0)])
        return np.where(ok, dcool.offsets[np.maximum(codes, 0)] + local, -1)

    s1, e1, s2, e2 = (bed2d[c].to_numpy() for c in ("start1", "end1", "start2", "end2"))
    g1 = bins(c1, (s1 + e1) // 2)
    g2 = bins(c2, (s2 + e2) // 2)
    n_pos = len(bed2d)
    # plain arrays while the blocks are scanned (one pandas assignment per block and template cost more than the
    # native calls); the tables are assembled once below
    score_out = [np.full(n_pos, np.nan) for _ in kernels]
    pval_out = [np.full(n_pos, np.nan) for _ in kernels]
    # windows: in position order where a path needs them there (block-by-block fall-back, sharded runs); the batched path hands
    # its windows on in block order with the positions they belong to (three 2.4 MB scatters and as many NaN fills less)
    win_out = [None for _ in kernels]
    win_src = [None for _ in kernels]

    def win_array(k):
        if win_out[k] is None:
            win_out[k] = np.full((n_pos, km, kn), np.nan)
        return win_out[k]
    located = (g1 >= 0) & (g2 >= 0)
    # positions of every sub-matrix, in input order: one stable sort by (chrom1, chrom2); only the sub-matrices that hold a
    # position are visited (no pattern on a sub-matrix: it is not scanned, :240), in the order of sub_matrices()
    pair_key = np.where(located, c1 * (dcool.n_chrom + 1) + c2, -1)
    order = np.argsort(pair_key, kind="stable")
    keys_sorted = pair_key[order]
    present, first = np.unique(keys_sorted, return_index=True)
    ends = np.append(first[1:], keys_sorted.size)
    todo = []
    for key, lo, hi in zip(present.tolist(), first.tolist(), ends.tolist()):
        ca, cb = divmod(key, dcool.n_chrom + 1)
        if key < 0 or ca > cb or (ca != cb and not inter):
            continue                                        # (sub_matrices(): upper blocks, inter ones only with --inter)
        sel = order[lo:hi]
        todo.append((ca, cb, sel, np.column_stack([g1[sel] - dcool.offsets[ca], g2[sel] - dcool.offsets[cb]]).astype(int)))
    # Sharded run (parallel.quantify_genome): this rank scores the positions of its own sub-matrices, the scores of all ranks
    # are exchanged once below -- the reference's pool over sub-matrices (cli/chromosight.py:396-410)
    if shard is None:
        mine = todo
    elif getattr(shard, "prices_strips", False):         # (parallel.QuantifyShard: trans units priced by the rows they stage)
        mine = shard.select(todo, dcool, max_dist, budget=budget, reach=_strip_reach(kernels))
    else:
        mine = shard.select(todo, dcool, max_dist)
    # trans sub-matrices, with a shard or without: never staged whole, only the rows of their positions (quantify_inter_block)
    strips = [t for t in mine if t[0] != t[1]]
    mine = [t for t in mine if t[0] == t[1]]
    # every intra sub-matrix that holds a position is staged once, with ONE native call (cs_stage_blocks)
    intra = [ca for ca, _, _, _ in mine]
    staged = dict(zip(intra, dcool.stage_blocks(intra, max_dist, largest, smooth=smooth))) if intra else {}
    blocks = [staged[ca] for ca, _, _, _ in mine]
    # one native call per template for the positions of all sub-matrices (cs_quantify_blocks), the coordinate lists prepared
    # once for all templates ...
    res_all = None
    if mine and tsvd is None and not os.environ.get("CHROMOSIGHT_HIP_NO_QUANTIFY_BATCH"):
        for kernel in kernels:
            _check_template(kernel)
        res_all = cid.quantify_many_on_device(dcool.dev, blocks, [engine.KernelSpec(k) for k in kernels], cfg, [c for _, _, _, c in mine])
    if res_all is not None:
        where = np.concatenate([sel for _, _, sel, _ in mine])
        for kernel_id, (table, wins) in enumerate(res_all):
            score_out[kernel_id][where] = table[:, 2]
            pval_out[kernel_id][where] = table[:, 3]
            if shard is None:
                win_src[kernel_id] = (wins, where)
            else:
                win_array(kernel_id)[where] = wins
    for kernel_id, kernel in enumerate(kernels):
        if res_all is not None:
            continue
        # ... or, where the batch does not apply (truncated SVD, non-square templates), one per sub-matrix and template
        for (ca, cb, sel, coords), block in zip(mine, blocks):
            rec, wins = detect_block(dcool, block, cfg, kernel, tsvd=tsvd, coords=coords.copy(), raw=True)
            if rec is None:
                continue
            score_out[kernel_id][sel] = rec[:, 2]
            pval_out[kernel_id][sel] = rec[:, 3]
            win_array(kernel_id)[sel] = wins
    if strips:
        for k in range(len(kernels)):
            if win_src[k] is not None:                  # (the batched windows in position order beside the trans blocks' below)
                wins, where = win_src[k]
                win_array(k)[where] = wins
                win_src[k] = None
        for ca, cb, sel, coords in strips:
            res = quantify_inter_block(dcool, ca, cb, coords, kernels, cfg, tsvd=tsvd, inter_budget=budget)
            for kernel_id, (table, wins) in enumerate(res):
                score_out[kernel_id][sel] = table[:, 2]
                pval_out[kernel_id][sel] = table[:, 3]
                win_array(kernel_id)[sel] = wins
        dcool._strips.release()
    if shard is not None:
        win_out = [win_array(k) for k in range(len(kernels))]
        score_out, pval_out, win_out = shard.merge(score_out, pval_out, win_out, [sel for _, _, sel, _ in mine + strips])
    # best score of every coordinate among the templates, as the reference selects it (:432-441): the tables of the templates
    # one below the other, sort_values("score"), last row of every (chrom1, start1, chrom2, start2) group.  In numpy -- the
    # same argsort pandas runs (quicksort on the finite scores, NaN last), so ties fall as they do there -- because the
    # pandas version (three assigns, a concat of 3 n rows, a sort and a groupby) cost more than scoring the positions.
    n_k = len(kernels)
    score_all, pval_all = np.concatenate(score_out), np.concatenate(pval_out)
    idx = np.arange(score_all.size)
    nan = np.isnan(score_all)
    in_sorted = np.concatenate([idx[~nan][np.argsort(score_all[~nan], kind="quicksort")], idx[nan]])
    # (group key: the four columns factorised into one integer -- a row-wise np.unique costs ten times as much)
    gid = np.zeros(n_pos, dtype=np.int64)
    for col in (bed2d.chrom1, s1, bed2d.chrom2, s2):
        codes, uniques = pd.factorize(col)
        gid = gid * (len(uniques) + 1) + (codes + 1)
    groups_sorted = np.tile(gid, n_k)[in_sorted]
    _, first_from_end = np.unique(groups_sorted[::-1], return_index=True)
    pick = in_sorted[np.sort(groups_sorted.size - 1 - first_from_end)]          # groupby(sort=False).tail(1): in sorted-frame order
    src = pick % n_pos
    score, pvalue = score_all[pick], pval_all[pick]
    windows = np.empty((pick.size, km, kn))
    for k in range(n_k):
        m = pick // n_pos == k
        if win_src[k] is not None:
            wins, where = win_src[k]
            inv = np.full(n_pos, -1, dtype=np.int64)
            inv[where] = np.arange(where.size)
            at = inv[src[m]]
            if (at >= 0).all():
                windows[m] = wins[at]
            else:                                       # (positions no sub-matrix holds: NaN windows, as the position-order arrays had)
                w = np.full((at.size, km, kn), np.nan)
                w[at >= 0] = wins[at[at >= 0]]
                windows[m] = w
        else:
            windows[m] = win_array(k)[src[m]]
    # the bin columns come from the interval STARTS (coords_to_bins of start1 / start2, :446-455), the scores from
    # the interval midpoints: they differ for intervals wider than one bin
    out1, out2 = bins(c1[src], s1[src]), bins(c2[src], s2[src])
    if (out1 < 0).any() or (out2 < 0).any():            # no such bin: NaN, as the reference's merge leaves it
        out1, out2 = np.where(out1 < 0, np.nan, out1), np.where(out2 < 0, np.nan, out2)
    qvalue = np.asarray(fdr_correction(pvalue), dtype=np.float64)
    bad = np.isnan(score)
    pvalue = np.where(bad, np.nan, pvalue)
    qvalue = np.where(bad, np.nan, qvalue)
    final = np.lexsort((out2, out1))                    # sort_values(["bin1", "bin2"]): stable, NaN last
    cols = {c: bed2d[c].to_numpy()[src][final] for c in ("chrom1", "start1", "end1", "chrom2", "start2", "end2")}
    cols.update(bin1=out1[final], bin2=out2[final], score=score[final], pvalue=pvalue[final], qvalue=qvalue[final])
    return pd.DataFrame(cols), windows                   # (the windows keep the selection order, as before the final sort of the table: cli/chromosight.py:441-470)
