"""Merging of resident pixel tables on the device: cs_merge_count / cs_merge_fill (chromosight_amd/csrc/cs_merge.hip).

The reference leaves the pooling of replicates to `cooler merge`, run before chromosight is started.  The rules below restate
what `cooler merge` writes; cooler is not part of this stack, so nothing here was captured from it:

- all sources describe the same bins (equal chromosome names, offsets and bin size, equal bin_start / bin_end where both have
  them) and are resident on the same device; anything else is refused with ValueError on the host, before any launch;
- the merged table holds one pixel for every (bin1, bin2) stored in at least one source, its count the sum of the sources'
  counts there, rows sorted by column.  Nothing is mirrored: the result is upper-triangle exactly when every source is;
- a pixel whose summed count is 0 (explicit zeros stored in every source that has it) is NOT stored -- cs_coarsen's rule, and
  staging eliminates zeros anyway;
- counts are finite, non-negative integers (in float32 or float64 containers, mixed freely between the sources) with a grand
  total over all sources below 2^53, so every sum is exact and the table is bitwise the same on every run, for every order of
  the sources, on every context, device and rank; anything else is refused with ValueError;
- the counts come out as float32 when every summed count is below 2^24, else float64 (the constructor's rule);
- no weights are carried: the sum of balanced tables is not balanced.  A single table is returned with its weights;
- at most 64 sources per call, fewer than 2^31 - 1 pixels in each source and in the result (ValueError beyond).

The result is allocated at its exact size, in HBM, next to the sources: the peak is sources + result."""
import ctypes as C

import numpy as np

from ._lib import CsCsr, load_library, np_dtype_of, plain_csr

MAX_SOURCES = 64


def __getattr__(name):
    if name == "TILE_COLUMNS":                  # the columns of a row that one pass through on-chip memory covers; read from
        return int(load_library().cs_merge_tile_columns())          # the library when asked for, so that importing needs none
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _same_or_absent(a, b):
    return a is None or b is None or np.array_equal(np.asarray(a), np.asarray(b))


def check_compatible(dcools):
    """The host-side refusals of a merge (ValueError): no source, more than 64, sources on different devices, or over different
    bins (chromosome names, offsets, bin size; bin_start / bin_end where both tables have them).  Reads only the geometry:
    .dev, .names, .offsets, .binsize, .bin_start, .bin_end.  Returns the sources as a list."""
    dcools = list(dcools)
    if not dcools:
        raise ValueError("nothing to merge: at least one pixel table is needed")
    if len(dcools) > MAX_SOURCES:
        raise ValueError(f"at most {MAX_SOURCES} pixel tables are merged in one call, got {len(dcools)}")
    first = dcools[0]
    for i, other in enumerate(dcools[1:], start=1):
        if other.dev is not first.dev:
            raise ValueError(f"pixel table {i} is resident on another device than table 0")
        if [str(x) for x in other.names] != [str(x) for x in first.names]:
            raise ValueError(f"pixel table {i} has other chromosome names than table 0")
        if not np.array_equal(np.asarray(other.offsets), np.asarray(first.offsets)):
            raise ValueError(f"pixel table {i} has other chromosome offsets than table 0")
        if int(other.binsize) != int(first.binsize):
            raise ValueError(f"pixel table {i} has bins of {int(other.binsize)} bp, table 0 of {int(first.binsize)} bp")
        if not _same_or_absent(other.bin_start, first.bin_start) or not _same_or_absent(other.bin_end, first.bin_end):
            raise ValueError(f"pixel table {i} has other bin coordinates than table 0")
    return dcools


def merge_csr(dcools):
    """Merge the tables of pipeline.DeviceCool objects on their device.  Returns a dict: `indptr` (bins + 1), `indices`, `data`
    (device buffers of exactly `nnz` pixels; one entry when there is none), `nnz` and `val_dtype` (float32 when every summed
    count is below 2^24, else float64).  Pixels whose summed count is 0 are not stored.  ValueError for incompatible sources,
    for counts that are not finite non-negative integers with a total below 2^53, and beyond the limits of the kernel."""
    dcools = check_compatible(dcools)
    dev = dcools[0].dev
    n = int(dcools[0].n_bins)
    csrs = [d.csr() for d in dcools]
    tables = (C.POINTER(CsCsr) * len(csrs))(*[C.pointer(c) for c in csrs])
    indptr = dev.empty(n + 1, np.int64)
    out_nnz, out_dtype = C.c_int64(0), C.c_int32(0)
    with dev.lock:
        try:
            dev._check(dev.lib.cs_merge_count(dev.ctx, None, tables, len(csrs), indptr.ptr, C.byref(out_nnz), C.byref(out_dtype)))
            nnz = int(out_nnz.value)
            val_dtype = np_dtype_of(out_dtype.value)
            indices = dev.empty(max(nnz, 1), np.int32)
            data = dev.empty(max(nnz, 1), val_dtype)
            out = plain_csr(n, nnz, indptr, indices, data, val_dtype)
            dev._check(dev.lib.cs_merge_fill(dev.ctx, None, tables, len(csrs), C.byref(out)))
        except NotImplementedError as exc:          # CS_ERR_UNSUPPORTED: a limit of the kernel, not a missing feature
            raise ValueError(str(exc)) from None
    return {"indptr": indptr, "indices": indices, "data": data, "nnz": nnz, "val_dtype": val_dtype}


def merge_device(dcools):
    """DeviceCool.merged: a DeviceCool on the same device over the merged table, with the first source's bins and names, upper
    exactly when every source is, and no weights (a single source: its weights)."""
    from .pipeline import DeviceCool
    dcools = check_compatible(dcools)
    res = merge_csr(dcools)
    first = dcools[0]
    return DeviceCool.from_device_csr(first, res["indptr"], res["indices"], res["data"], res["nnz"], res["val_dtype"],
                                      weight=first.host_weight if len(dcools) == 1 else None,
                                      upper=all(bool(d.upper) for d in dcools))
