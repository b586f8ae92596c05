"""numpy oracle of the coarsening of a pixel table (chromosight_amd/coarsen.py, cs_coarsen): a restatement of what
`cooler coarsen -k factor` writes.  cooler is not part of this stack, so nothing here was captured from it; the oracle is pinned
against an independent dense formulation in tests/test_coarsen_host.py.

- bins: every chromosome on its own, ceil(n_c / k) coarse bins, coarse(b) = off'[c] + (b - off[c]) // k;
- pixels: keys I * n' + J of the stored pixels, np.unique(return_inverse=True), int64 sums; zero sums dropped; nothing mirrored;
- geometry: bin_start = local * k * binsize, bin_end = min(bin_start + k * binsize, chromosome length)."""
import numpy as np


def coarse_bins(offsets, factor):
    """(coarse bin of every fine bin, coarse chromosome offsets)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(offsets)
    coarse_off = np.concatenate([[0], np.cumsum(-(-sizes // factor))]).astype(np.int64)
    chrom = np.repeat(np.arange(sizes.size), sizes)
    fine = np.arange(int(offsets[-1]), dtype=np.int64)
    return coarse_off[chrom] + (fine - offsets[chrom]) // factor, coarse_off


def oracle_geometry(offsets, binsize, bin_end, factor):
    """(coarse offsets, bin_start, bin_end, binsize * factor), chromosome by chromosome."""
    offsets = np.asarray(offsets, dtype=np.int64)
    _, coarse_off = coarse_bins(offsets, factor)
    start, end = [], []
    for c in range(offsets.size - 1):
        n_c = int(offsets[c + 1] - offsets[c])
        if n_c == 0:
            continue
        length = n_c * binsize if bin_end is None else int(np.asarray(bin_end)[offsets[c + 1] - 1])
        for j in range(-(-n_c // factor)):
            start.append(j * factor * binsize)
            end.append(min((j + 1) * factor * binsize, length))
    return coarse_off, np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64), binsize * factor


def oracle_coarsen(cool, factor):
    """The decoded-cool dictionary of `cool` coarsened by `factor`: int64 counts, no weights."""
    offsets = np.asarray(cool["chrom_offset"], dtype=np.int64)
    cmap, coarse_off = coarse_bins(offsets, factor)
    n_coarse = int(coarse_off[-1])
    b1 = cmap[np.asarray(cool["bin1_id"], dtype=np.int64)]
    b2 = cmap[np.asarray(cool["bin2_id"], dtype=np.int64)]
    cnt = np.asarray(cool["count"])
    assert np.all(cnt == np.rint(cnt)) and np.all(cnt >= 0)
    keys, inv = np.unique(b1 * n_coarse + b2, return_inverse=True)
    sums = np.zeros(keys.size, dtype=np.int64)
    np.add.at(sums, inv.ravel(), cnt.astype(np.int64))
    keep = sums > 0
    keys, sums = keys[keep], sums[keep]
    _, start, end, binsize = oracle_geometry(offsets, int(cool["binsize"]), cool.get("bin_end"), factor)
    return {"binsize": binsize, "chrom_offset": coarse_off, "chrom_names": np.asarray(cool["chrom_names"]),
            "bin1_id": keys // max(n_coarse, 1), "bin2_id": keys % max(n_coarse, 1), "count": sums, "weight": None,
            "bin_start": start, "bin_end": end}


def csr_of(cool):
    """(indptr, indices int32, counts int64, value dtype) of a decoded-cool dictionary sorted by (bin1, bin2): float32 when every
    count is below 2^24, else float64 (DeviceCool's rule)."""
    n = int(np.asarray(cool["chrom_offset"])[-1])
    b1 = np.asarray(cool["bin1_id"], dtype=np.int64)
    cnt = np.asarray(cool["count"], dtype=np.int64)
    indptr = np.searchsorted(b1, np.arange(n + 1)).astype(np.int64)
    dtype = np.float32 if cnt.size == 0 or cnt.max() < (1 << 24) else np.float64
    return indptr, np.asarray(cool["bin2_id"]).astype(np.int32), cnt, dtype


def block_totals(cool):
    """int64 matrix: the contacts stored in every (chromosome, chromosome) block."""
    offsets = np.asarray(cool["chrom_offset"], dtype=np.int64)
    n_chrom = offsets.size - 1
    chrom = np.repeat(np.arange(n_chrom), np.diff(offsets))
    out = np.zeros(n_chrom * n_chrom, dtype=np.int64)
    np.add.at(out, chrom[np.asarray(cool["bin1_id"], dtype=np.int64)] * n_chrom + chrom[np.asarray(cool["bin2_id"], dtype=np.int64)],
              np.asarray(cool["count"]).astype(np.int64))
    return out.reshape(n_chrom, n_chrom)
