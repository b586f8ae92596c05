"""Shared by tests/test_pileup_host.py and tests/test_gpu_pileup.py: the summation order of cs_pileup_blocks
(include/chromosight_hip.h) restated in numpy, and the CPU detect pipeline of the pinned oracles for one template.  Imports
nothing from a test module."""
import numpy as np

from chromosight_amd import engine


def restated_pileup(windows, chunk=None):
    """(sum, cnt) over a stack of windows (n, km, kn) in the order the header documents: the windows cut into consecutive
    chunks of S = cs_pileup_chunk(n); within a chunk a pixel is accumulated from +0.0 in window order, NaN skipped; the chunks'
    partial sums are then added from +0.0 in chunk order."""
    w = np.asarray(windows, dtype=np.float64)
    n, shape = w.shape[0], w.shape[1:]
    s = engine.pileup_chunk(n) if chunk is None else int(chunk)
    total, count = np.zeros(shape), np.zeros(shape, dtype=np.int64)
    for a in range(0, n, s):
        part, k = np.zeros(shape), np.zeros(shape, dtype=np.int64)
        for t in range(a, min(n, a + s)):
            m = ~np.isnan(w[t])
            part[m] += w[t][m]
            k[m] += 1
        total += part
        count += k
    return total, count


def sum_bound(windows, per_value=0.0):
    """Per pixel: 2 (c - 1) 2^-53 sum|x| -- two orderings of a float64 sum of the pixel's c non-NaN values -- plus c times
    `per_value` (the tolerance granted to each window value)."""
    w = np.asarray(windows, dtype=np.float64)
    c = np.sum(~np.isnan(w), axis=0)
    return 2.0 * np.maximum(c - 1, 0) * 2.0 ** -53 * np.nansum(np.abs(w), axis=0) + c * per_value


def oracle_block_tables(cool, ci, cfg, max_dist, kernels):
    """(bin1, bin2, score) tables of one chromosome, one per template, from the CPU oracles (oracle/detrend_oracle.py,
    oracle/oracle.c, oracle/foci_oracle.py)."""
    from oracle import c_oracle, detrend_oracle, foci_oracle
    largest = max(k.shape[0] for k in kernels)
    off = cool["chrom_offset"]
    n = int(off[ci + 1] - off[ci])
    keep = min(max_dist, n) + largest
    band, det = detrend_oracle.balanced_band(cool, ci, keep)
    prepared, _ = detrend_oracle.prepare_band(band, det)
    miss = ~det
    out = []
    for kern in kernels:
        if n <= max(kern.shape):
            out.append(np.zeros((0, 3)))
            continue
        out_w = min(max_dist, n - 1) + 1
        corr, _ = c_oracle.normxcorr2_band(prepared, n, 0, prepared.shape[1], kern, 0, n, 0, out_w, max_dist=max_dist, miss_row=miss,
                                           miss_col=miss, missing_tol=cfg["max_perc_undetected"] / 100)
        out.append(foci_oracle.detect_table_band(prepared, 0, corr, 0, n, miss, kern.shape, cfg["pearson"], cfg["max_perc_zero"] / 100,
                                                 cfg["max_perc_undetected"] / 100, diag_only=cfg["max_dist"] == 0))
    return out
