"""Coarsening of a resident pixel table on the device: cs_coarsen (chromosight_amd/csrc/cs_coarsen.hip).

The reference leaves this step to `cooler coarsen` / `cooler zoomify`, run before chromosight is started.  The rules below restate
what `cooler coarsen -k factor` writes; cooler is not part of this stack, so nothing here was captured from it:

- every chromosome is regrouped on its own: one of n_c bins gets ceil(n_c / factor) coarse bins, coarse(b) = off'[c] +
  (b - off[c]) // factor, and the last coarse bin of a chromosome may cover fewer than `factor` fine bins;
- the stored pixels are grouped by (coarse(bin1), coarse(bin2)) and their counts summed.  Nothing is mirrored: a coarse diagonal
  pixel is the sum of the stored (upper-triangle) fine pixels that fall into it, and an upper-triangle table stays one;
- counts are finite, non-negative integers (in float32 or float64 containers) with a grand total below 2^53, so every sum is exact
  and the table is the same on every run, context and device; anything else is refused with ValueError;
- no weights are carried: fine-bin weights mean nothing for coarse bins.  The new table stays in HBM."""
import ctypes as C

import numpy as np

from ._lib import np_dtype_of, plain_csr


def check_factor(factor):
    if isinstance(factor, bool) or int(factor) != factor:
        raise ValueError(f"the coarsening factor must be an integer, got {factor!r}")
    factor = int(factor)
    if factor < 1:
        raise ValueError(f"the coarsening factor must be at least 1, got {factor}")
    if factor >= 2 ** 31:
        raise ValueError(f"the coarsening factor must be below 2^31, got {factor}")
    return factor


def coarse_geometry(offsets, binsize, bin_end, factor):
    """The bins of a table coarsened by `factor`, on the host: (coarse chromosome offsets, bin_start, bin_end, binsize * factor).
    offsets: the n_chrom + 1 chromosome offsets of the fine bins; bin_end: the fine bins' end coordinates, or None.
    bin_start = local * factor * binsize; bin_end = min(bin_start + factor * binsize, chromosome length), where the length is the
    parent's bin_end of the chromosome's last bin, or n_c * binsize when the parent has none."""
    factor = check_factor(factor)
    offsets = np.asarray(offsets, dtype=np.int64)
    binsize = int(binsize)
    sizes = np.diff(offsets)
    if offsets.ndim != 1 or offsets.size < 2 or offsets[0] != 0 or np.any(sizes < 0):
        raise ValueError("chromosome offsets must run upwards from 0")
    coarse_sizes = -(-sizes // factor)
    coarse_off = np.concatenate([[0], np.cumsum(coarse_sizes)]).astype(np.int64)
    if bin_end is None:
        length = sizes * binsize
    else:
        bin_end = np.asarray(bin_end, dtype=np.int64)
        if bin_end.shape != (int(offsets[-1]),):
            raise ValueError(f"bin_end of shape {bin_end.shape} for {int(offsets[-1])} bins")
        last = np.maximum(offsets[1:] - 1, 0)
        length = np.where(sizes > 0, bin_end[last], 0) if bin_end.size else np.zeros_like(sizes)
    local = np.arange(int(coarse_off[-1]), dtype=np.int64) - np.repeat(coarse_off[:-1], coarse_sizes)
    start = local * (factor * binsize)
    end = np.minimum(start + factor * binsize, np.repeat(length, coarse_sizes))
    return coarse_off, start, end, binsize * factor


def coarsen_csr(dcool, factor):
    """Coarsen the table of a pipeline.DeviceCool on its device.  Returns a dict: `indptr` (coarse bins + 1), `indices`, `data`
    (device buffers with room for dcool.nnz pixels, the first `nnz` used), `nnz`, `val_dtype` (float32 when every summed count is
    below 2^24, else float64) and the coarse geometry: `offsets`, `bin_start`, `bin_end`, `binsize`.  ValueError for a factor
    below 1 and for counts that are not finite non-negative integers with a total below 2^53."""
    factor = check_factor(factor)
    offsets, start, end, binsize = coarse_geometry(dcool.offsets, dcool.binsize, dcool.bin_end, factor)
    dev = dcool.dev
    n_chrom = int(dcool.offsets.size - 1)
    fine_off = np.ascontiguousarray(dcool.offsets, dtype=np.int64)
    n_coarse = int(offsets[-1])
    nnz = int(dcool.nnz)
    indptr = dev.empty(n_coarse + 1, np.int64)
    indices = dev.empty(max(nnz, 1), np.int32)
    data = dev.empty(max(nnz, 1), np.float64)
    out = plain_csr(n_coarse, 0, indptr, indices, data, np.float32)
    out_nnz = C.c_int64(0)
    genome = dcool.csr()
    with dev.lock:
        dev._check(dev.lib.cs_coarsen(dev.ctx, None, C.byref(genome), fine_off.ctypes.data_as(C.POINTER(C.c_int64)), n_chrom, factor,
                                      C.byref(out), C.byref(out_nnz)))
    if out.n_rows != n_coarse:
        raise RuntimeError(f"cs_coarsen made {out.n_rows} coarse bins, the host geometry {n_coarse}")
    return {"indptr": indptr, "indices": indices, "data": data, "nnz": int(out_nnz.value),
            "val_dtype": np_dtype_of(out.dtype), "offsets": offsets, "bin_start": start, "bin_end": end, "binsize": binsize}


def coarsen_device(dcool, factor):
    """DeviceCool.coarsened(factor): a DeviceCool on the same device over the coarse table, with the coarse bins and no weights
    (factor 1: the parent's bins and weights)."""
    from .pipeline import DeviceCool
    res = coarsen_csr(dcool, factor)
    keep = int(factor) == 1
    return DeviceCool.from_device_csr(dcool, res["indptr"], res["indices"], res["data"], res["nnz"], res["val_dtype"],
                                      offsets=res["offsets"], binsize=res["binsize"],
                                      bin_start=dcool.bin_start if keep else res["bin_start"],
                                      bin_end=dcool.bin_end if keep else res["bin_end"],
                                      weight=dcool.host_weight if keep else None)
