"""ICE balancing of a resident pixel table (cooler.balance_cooler, what the reference's HicGenome.normalize runs on a file
without weights: contacts_map.py:203-221) on the device: cs_ice_balance (chromosight_amd/csrc/cs_balance.hip).

The weights come back to the caller; nothing is written to any file (the reference stores them in the input .cool)."""
import ctypes as C
import warnings

import numpy as np

from ._lib import CsIceParams, CsIceSpanStats


class ConvergenceWarning(UserWarning):
    """A span of the balancing reached max_iters before the variance of its marginals fell below tol (cooler's warning)."""


def ice_balance(dcool, *, cis_only=True, mad_max=5, min_nnz=10, min_count=0, ignore_diags=2, tol=1e-5, max_iters=200,
                rescale_marginals=True):
    """ICE weights of a pipeline.DeviceCool's pixel table, with the arguments of cooler.balance_cooler.

    cis_only: every chromosome is balanced on its own cis pixels (a span per chromosome); else one genome-wide span,
    trans pixels included.  Bins with fewer than min_nnz nonzero pixels, a marginal below min_count, or a log marginal more
    than mad_max MADs below the median (each chromosome scaled by its median first) get NaN; pixels closer to the diagonal
    than ignore_diags are dropped.  Returns (weights: float64 array of n_bins, info: dict of per-span arrays `scale`, `var`,
    `converged`, `iterations`); a ConvergenceWarning is issued for every span that did not converge.  The weights are bitwise
    identical from call to call (fixed-order float64 sums on the device).  dcool's own weights are left as they are."""
    dev = dcool.dev
    n_chrom = int(dcool.offsets.size - 1)
    p = CsIceParams(int(bool(cis_only)), int(ignore_diags), int(min_nnz), int(max_iters), float(min_count), float(mad_max),
                    float(tol), int(bool(rescale_marginals)), 0)
    n_spans = n_chrom if cis_only else 1
    stats = (CsIceSpanStats * max(n_spans, 1))()
    offsets = np.ascontiguousarray(dcool.offsets, dtype=np.int64)
    bias = dev.empty(max(dcool.n_bins, 1), np.float64)
    genome = dcool.csr()
    with dev.lock:
        dev._check(dev.lib.cs_ice_balance(dev.ctx, None, C.byref(genome), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                          n_chrom, C.byref(p), bias.ptr, stats))
    weights = bias.download()[:dcool.n_bins].copy()
    rows = list(stats)[:n_spans]
    info = {"scale": np.array([s.scale for s in rows]), "var": np.array([s.var for s in rows]),
            "converged": np.array([bool(s.converged) for s in rows]), "iterations": np.array([s.iterations for s in rows])}
    for k in np.flatnonzero(~info["converged"]):
        where = f"chromosome {dcool.names[k]}" if cis_only else "the genome"
        warnings.warn(f"ICE balancing of {where}: iteration limit ({max_iters}) reached without convergence "
                      f"(variance {info['var'][k]:.3g} >= tol {tol:g})", ConvergenceWarning, stacklevel=2)
    return weights, info
