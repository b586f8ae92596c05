"""numpy oracle of the binning of read pairs (chromosight_amd/cload.py, cs_pairs_count / cs_pairs_fill): a restatement of what
`cooler cload pairs` writes.  cooler is not part of this stack, so nothing here was captured from it; the oracle is held to a
dense per-pair loop in tests/test_cload_host.py.

- geometry: chromosome c of len_c bp gets ceil(len_c / binsize) bins, the last one possibly short; offsets are their prefix sum;
- a pair with an id of -1 on either side is dropped; an id outside [-1, n_chrom) or a zero-based position outside [0, len_c) of a
  known chromosome refuses the chunk (ValueError with the number of such pairs and the first one's index); refusing comes first;
- bin = offset[c] + pos0 // binsize; bin1 > bin2 is reflected; np.unique(..., return_counts=True) over bin1 * n + bin2;
- dtype of the counts: float32 when every count is below 2^24, else float64 (DeviceCool's rule).

Also: the expansion of a pixel table into read pairs, and the adversarial chunks of the device tests (seeds only)."""
import numpy as np

BINSIZE = 1000
# the toy genome of the device tests: 257 bins -- a last bin of 37 bp, a chromosome shorter than a bin, an exact multiple
TOY = (("a", 100 * BINSIZE + 37), ("b", 5), ("c", 155 * BINSIZE))
TOY_BINS = 257
FAMILIES = ("distinct", "one_pixel", "block_runs", "lone_last")


def geometry(chromsizes, binsize):
    """(names, lengths, offsets, bin_start, bin_end) of `chromsizes` (pairs or a mapping) at `binsize`."""
    items = list(chromsizes.items()) if hasattr(chromsizes, "items") else list(chromsizes)
    names = [str(n) for n, _ in items]
    lengths = np.asarray([int(x) for _, x in items], dtype=np.int64)
    assert np.all(lengths >= 1) and binsize >= 1
    n_bins = (lengths + binsize - 1) // binsize
    offsets = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int64)
    start = np.concatenate([np.arange(k, dtype=np.int64) * binsize for k in n_bins]) if len(names) else np.zeros(0, dtype=np.int64)
    end = np.concatenate([np.minimum((np.arange(k, dtype=np.int64) + 1) * binsize, ln) for k, ln in zip(n_bins, lengths)]) \
        if len(names) else np.zeros(0, dtype=np.int64)
    return names, lengths, offsets, start, end


def oracle_cload(chromsizes, binsize, chrom1, pos1, chrom2, pos2, zero_based=False):
    """The decoded-cool dictionary of the binned pairs (int64 counts, no weights), with `val_dtype` (the dtype the counts take on
    the device) and `dropped`.  ValueError("<k> of <n> pairs refused ...; the first is pair <i> ...") as the device call."""
    names, lengths, offsets, start, end = geometry(chromsizes, binsize)
    n_chrom, n = len(names), int(offsets[-1])
    cols = [np.asarray(x, dtype=np.int64) for x in (chrom1, pos1, chrom2, pos2)]
    shift = 0 if zero_based else 1
    refused = np.zeros(cols[0].size, dtype=bool)
    dropped = np.zeros(cols[0].size, dtype=bool)
    bins = []
    for c, p in ((cols[0], cols[1]), (cols[2], cols[3])):
        known = (c >= 0) & (c < n_chrom)
        safe = np.where(known, c, 0)
        # (python integers where the shift could wrap: only the minimum of int64 can)
        pos0 = np.where(p == np.iinfo(np.int64).min, -1, p - shift * (p != np.iinfo(np.int64).min))
        inside = (pos0 >= 0) & (pos0 < (lengths[safe] if n_chrom else 0))
        refused |= (c < -1) | (c >= n_chrom) | (known & ~inside)
        dropped |= c == -1
        bins.append(np.where(known & inside, (offsets[safe] if n_chrom else 0) + pos0 // binsize, 0))
    if refused.any():
        raise ValueError(f"{int(refused.sum())} of {refused.size} pairs refused; the first is pair {int(np.argmax(refused))} of the chunk")
    keep = ~dropped
    b1, b2 = np.minimum(bins[0], bins[1])[keep], np.maximum(bins[0], bins[1])[keep]
    keys, counts = np.unique(b1 * max(n, 1) + b2, return_counts=True)
    counts = counts.astype(np.int64)
    return {"binsize": int(binsize), "chrom_offset": offsets, "chrom_names": np.asarray(names, dtype=str), "bin1_id": keys // max(n, 1),
            "bin2_id": keys % max(n, 1), "count": counts, "weight": None, "bin_start": start, "bin_end": end,
            "val_dtype": np.float32 if counts.size == 0 or counts.max() < (1 << 24) else np.float64, "dropped": int(dropped.sum())}


def csr_of(want):
    """(row pointers, column bins, counts in the device's dtype) of an oracle table."""
    n = int(want["chrom_offset"][-1])
    indptr = np.searchsorted(want["bin1_id"], np.arange(n + 1)).astype(np.int64)
    return indptr, want["bin2_id"].astype(np.int32), want["count"].astype(want["val_dtype"])


def chromsizes_of(cool):
    """Ordered (name, length in bp) of a decoded-cool dictionary: the end of every chromosome's last bin."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    end = cool.get("bin_end")
    sizes = np.diff(off) * int(cool["binsize"]) if end is None else np.asarray(end, dtype=np.int64)[off[1:] - 1]
    return [(str(n), int(s)) for n, s in zip(cool["chrom_names"], sizes)]


def pairs_of_table(cool, seed):
    """A decoded pixel table expanded into read pairs (chrom1, pos1, chrom2, pos2): a pixel of count c becomes c pairs at seeded
    uniform positions inside its two bins, half of them swapped to the lower triangle, positions 1-based, the list shuffled."""
    rng = np.random.default_rng(seed)
    names, lengths, offsets, start, end = geometry(chromsizes_of(cool), int(cool["binsize"]))
    cnt = np.asarray(cool["count"]).astype(np.int64)
    b1 = np.repeat(np.asarray(cool["bin1_id"], dtype=np.int64), cnt)
    b2 = np.repeat(np.asarray(cool["bin2_id"], dtype=np.int64), cnt)
    swap = rng.random(b1.size) < 0.5
    b1, b2 = np.where(swap, b2, b1), np.where(swap, b1, b2)
    order = rng.permutation(b1.size)
    b1, b2 = b1[order], b2[order]
    out = []
    for b in (b1, b2):
        chrom = (np.searchsorted(offsets, b, side="right") - 1).astype(np.int32)
        pos = start[b] + rng.integers(0, end[b] - start[b]) + 1
        out += [chrom, pos.astype(np.int64)]
    return tuple(out)


def pairs_at(chromsizes, binsize, b1, b2, where="mid"):
    """1-based pairs that fall into the genome bins (b1[i], b2[i]), as given (not oriented): at the first base of a bin ("lo"), its
    last ("hi") or its middle ("mid")."""
    names, lengths, offsets, start, end = geometry(chromsizes, binsize)
    out = []
    for b in (np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64)):
        chrom = (np.searchsorted(offsets, b, side="right") - 1).astype(np.int32)
        pos0 = {"lo": start[b], "hi": end[b] - 1, "mid": (start[b] + end[b] - 1) // 2}[where]
        out += [chrom, (pos0 + 1).astype(np.int64)]
    return tuple(out)


def toy_table(seed, n_pairs=6000):
    """A decoded-cool table over TOY with about n_pairs contacts near the diagonal and some trans ones (from the seed alone)."""
    rng = np.random.default_rng([7, seed])
    a = rng.integers(0, TOY_BINS, size=n_pairs)
    b = np.clip(a + rng.geometric(0.15, size=n_pairs) - 1, 0, TOY_BINS - 1)
    far = rng.random(n_pairs) < 0.05
    b = np.where(far, rng.integers(0, TOY_BINS, size=n_pairs), b)
    want = oracle_cload(TOY, BINSIZE, *pairs_at(TOY, BINSIZE, a, b))
    return want


def adversarial_chunk(family, n, block, seed=0):
    """n pairs over TOY (1-based, shuffled, half of them lower-triangle) whose sorted keys stress the run-length pass, `block`
    being the pairs one workgroup covers there:
    - "distinct": n different pixels;
    - "one_pixel": all in one pixel -- one run across every block boundary;
    - "block_runs": runs of exactly `block` pairs (the last one shorter): runs begin and end at the multiples of `block`;
    - "lone_last": runs of 3, then the largest pixel of the table once: with n = k * block + 1 it is alone in the last block."""
    rng = np.random.default_rng([11, seed, n, FAMILIES.index(family)])
    iu, ju = np.triu_indices(TOY_BINS)
    if family == "distinct":
        pick = rng.choice(iu.size, size=n, replace=False)
    elif family == "one_pixel":
        pick = np.full(n, int(rng.integers(iu.size)))
    elif family == "block_runs":
        k = -(-n // block) if n else 0
        pick = np.repeat(np.sort(rng.choice(iu.size, size=k, replace=False)), block)[:n]
    else:
        k = -(-max(n - 1, 0) // 3)
        body = np.repeat(np.sort(rng.choice(iu.size - 1, size=k, replace=False)), 3)[:max(n - 1, 0)]
        pick = np.concatenate([body, [iu.size - 1]])[:n]
    b1, b2 = iu[pick], ju[pick]
    swap = rng.random(n) < 0.5
    b1, b2 = np.where(swap, b2, b1), np.where(swap, b1, b2)
    order = rng.permutation(n)
    return pairs_at(TOY, BINSIZE, b1[order], b2[order], where=("lo", "mid", "hi")[seed % 3])
