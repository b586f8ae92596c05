"""`--subsample` of a resident pixel table on the device (the reference's preprocessing.py:359-401 subsample_contacts on every
sub-matrix, contacts_map.py:555-596): cs_subsample (chromosight_amd/csrc/cs_subsample.hip).

The pools and the proportion kept are those of pipeline.DeviceCool.subsampled's numpy path; the draw differs (a split tree of exact
hypergeometric draws with counter-based uniforms instead of numpy's sequential sampler), so a seed gives another table than
sampler="numpy" -- but the same one on every device, context and launch shape.  The new table never leaves HBM."""
import ctypes as C

import numpy as np

from ._lib import CsSubsampleBlock, CsSubsampleParams, np_dtype_of, plain_csr

BLOCK_DTYPE = np.dtype([("chrom1", np.int32), ("chrom2", np.int32), ("total", np.int64), ("keep", np.int64)])


def check_sample(sample):
    """The host path's argument checks (DeviceCool.subsampled): 0 <= sample <= 1."""
    sample = float(sample)
    if sample < 0:
        raise ValueError("Subsample must be strictly positive.")
    if sample > 1:
        raise ValueError("Subsample cannot be above 1")
    if not np.isfinite(sample):
        raise ValueError(f"Subsample must be a proportion, got {sample}")
    return sample


def subsample_csr(dcool, sample, seed=0, inter=False, drawn=False):
    """Draw the subsample of a pipeline.DeviceCool's table on its device.  Returns a dict: `indptr`, `indices`, `data` (device
    buffers with room for dcool.nnz pixels, the first `nnz` used), `nnz`, `val_dtype` (float32 when every kept count is below
    2^24), `blocks` (BLOCK_DTYPE array: every sampled sub-matrix in (chrom1, chrom2) row-major order with its pool total and the
    contacts kept) and, with drawn=True, `drawn`: each pixel's share of its pool draw before the upper / mirror split (int64,
    table order, 0 outside the sampled blocks)."""
    sample = check_sample(sample)
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be a non-negative 64-bit integer, got {seed}")
    dev = dcool.dev
    n_chrom = int(dcool.offsets.size - 1)
    n_blocks = n_chrom * (n_chrom + 1) // 2 if inter else n_chrom
    offsets = np.ascontiguousarray(dcool.offsets, dtype=np.int64)
    nnz = int(dcool.nnz)
    indptr = dev.empty(dcool.n_bins + 1, np.int64)
    indices = dev.empty(max(nnz, 1), np.int32)
    data = dev.empty(max(nnz, 1), np.float64)
    d_drawn = dev.empty(max(nnz, 1), np.int64) if drawn else None
    out = plain_csr(dcool.n_bins, 0, indptr, indices, data, np.float32)
    params = CsSubsampleParams(sample, seed, int(bool(inter)), 0)
    blocks = (CsSubsampleBlock * max(n_blocks, 1))()
    out_nnz = C.c_int64(0)
    genome = dcool.csr()
    with dev.lock:
        dev._check(dev.lib.cs_subsample(dev.ctx, None, C.byref(genome), offsets.ctypes.data_as(C.POINTER(C.c_int64)), n_chrom,
                                        C.byref(params), C.byref(out), C.byref(out_nnz), blocks,
                                        d_drawn.ptr if d_drawn is not None else None))
    table = np.frombuffer(bytes(blocks), dtype=BLOCK_DTYPE, count=n_blocks).copy() if n_blocks else np.zeros(0, BLOCK_DTYPE)
    res = {"indptr": indptr, "indices": indices, "data": data, "nnz": int(out_nnz.value), "val_dtype": np_dtype_of(out.dtype),
           "blocks": table, "drawn": None}
    if d_drawn is not None:
        res["drawn"] = d_drawn.download()[:nnz].copy()
    return res


def subsample_device(dcool, sample, seed=0, inter=False):
    """DeviceCool.subsampled(..., sampler="device"): a DeviceCool on the same device built from the drawn CSR, with the parent's
    bins, names and weights."""
    from .pipeline import DeviceCool
    res = subsample_csr(dcool, sample, seed=seed, inter=inter)
    return DeviceCool.from_device_csr(dcool, res["indptr"], res["indices"], res["data"], res["nnz"], res["val_dtype"])
