"""numpy oracle of the merging of pixel tables (chromosight_amd/merge.py, cs_merge_count / cs_merge_fill): a restatement of what
`cooler merge` writes.  cooler is not part of this stack, so nothing here was captured from it; the oracle is pinned on a
hand-written example in tests/test_merge_host.py.

- pixels: the tables concatenated, keys bin1 * n + bin2, np.unique + np.add.at on int64; zero sums dropped; nothing mirrored;
- dtype of the counts: float32 when every sum is below 2^24, else float64 (DeviceCool's rule).

Also: the multinomial split of a table into replicates that sum back to it, and the adversarial genome of the device tests."""
import numpy as np

ASSUMED_TILE_COLUMNS = 2048        # what the adversarial genome is sized for; tests/test_gpu_merge.py checks it against the library
SIZES = (5, 70, 2 * ASSUMED_TILE_COLUMNS + 137)      # bins of the adversarial genome's chromosomes
SOURCE_COUNTS = (1, 2, 3, 8, 64)

# rows of the adversarial genome (whole-genome bins) and what they hold
ROW_IDENTICAL, ROW_ONE_SOURCE, ROW_EMPTY, ROW_INTERLEAVED, ROW_LONE_PIXEL, ROW_DENSE, ROW_ZEROS, ROW_TRANS = 0, 1, 2, 3, 4, 6, 10, 70
COL_ZERO_IN_ALL, COL_ZERO_MEETS_COUNT, COL_ZERO_ALONE = 20, 30, 40
RUN_LENGTHS = (63, 64, 65, 257)


def make_cool(sizes, b1, b2, cnt, binsize=1000, names=None):
    """A decoded-cool dictionary over chromosomes of `sizes` bins with the given pixels, sorted by (bin1, bin2)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    b1, b2, cnt = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64), np.asarray(cnt)
    order = np.lexsort((b2, b1))
    names = [f"c{i}" for i in range(sizes.size)] if names is None else names
    return {"binsize": binsize, "chrom_offset": off, "chrom_names": np.asarray(names), "bin1_id": b1[order], "bin2_id": b2[order],
            "count": cnt[order], "weight": None, "bin_start": None, "bin_end": None}


def oracle_merge(cools):
    """The decoded-cool dictionary of the merged tables (int64 counts, no weights), with `val_dtype`: the dtype the counts take
    on the device."""
    first = cools[0]
    n = int(np.asarray(first["chrom_offset"])[-1])
    b1 = np.concatenate([np.asarray(c["bin1_id"], dtype=np.int64) for c in cools])
    b2 = np.concatenate([np.asarray(c["bin2_id"], dtype=np.int64) for c in cools])
    parts = [np.asarray(c["count"]) for c in cools]
    for cnt in parts:
        assert np.all(cnt == np.rint(cnt)) and np.all(cnt >= 0)
    cnt = np.concatenate([p.astype(np.int64) for p in parts])
    keys, inv = np.unique(b1 * n + b2, return_inverse=True)
    sums = np.zeros(keys.size, dtype=np.int64)
    np.add.at(sums, inv.ravel(), cnt)
    keep = sums > 0
    keys, sums = keys[keep], sums[keep]
    return {"binsize": first["binsize"], "chrom_offset": np.asarray(first["chrom_offset"], dtype=np.int64),
            "chrom_names": np.asarray(first["chrom_names"]), "bin1_id": keys // max(n, 1), "bin2_id": keys % max(n, 1), "count": sums,
            "weight": None, "bin_start": first.get("bin_start"), "bin_end": first.get("bin_end"),
            "val_dtype": np.float32 if sums.size == 0 or sums.max() < (1 << 24) else np.float64}


def split_counts(cool, k, seed):
    """`cool` thinned into k replicates: every count is split multinomially (equal odds), and a pixel that gets 0 in a replicate
    stays there as a stored zero, so that every replicate has the pixels of `cool` and the replicates sum back to it."""
    rng = np.random.default_rng(seed)
    cnt = np.asarray(cool["count"])
    assert np.all(cnt == np.rint(cnt)) and np.all(cnt >= 0)
    shares = rng.multinomial(cnt.astype(np.int64), np.full(k, 1.0 / k))
    out = []
    for s in range(k):
        part = dict(cool)
        part["count"] = np.ascontiguousarray(shares[:, s]).astype(np.int64)
        part["weight"] = None
        out.append(part)
    return out


def adversarial_sources(k, seed=0):
    """k decoded-cool dictionaries over the adversarial genome (SIZES: the last chromosome is wider than two column tiles), all
    upper-triangle, from the seed alone.  What the rows hold is asserted from the tables in tests/test_merge_host.py."""
    rng = np.random.default_rng([seed, k])
    n = int(sum(SIZES))
    px = [dict() for _ in range(k)]                 # per source: (row, column) -> count

    def put(s, row, cols, counts):
        for c, v in zip(np.atleast_1d(cols).tolist(), np.broadcast_to(counts, np.atleast_1d(cols).shape).tolist()):
            px[s][row, int(c)] = int(v)

    def some_columns(row, size):
        return row + rng.choice(n - row, size=size, replace=False)

    for s in range(k):
        # the same row in every source, with the first and the last column of the table
        put(s, ROW_IDENTICAL, [0, 3, 7, 80, ASSUMED_TILE_COLUMNS - 1, ASSUMED_TILE_COLUMNS, n - 1], [5, 1, 2, 9, 4, 6, 3])
        # source s holds the columns = s mod k: together every column from the diagonal to the last bin
        cols = np.arange(ROW_INTERLEAVED, n)
        put(s, ROW_INTERLEAVED, cols[cols % k == s], 1 + cols[cols % k == s] % 7)
        # the last row: its diagonal pixel, the last column of the table
        put(s, n - 1, [n - 1], 2 + s)
    # a row that only one source has (ROW_EMPTY is in none)
    put(1 % k, ROW_ONE_SOURCE, some_columns(ROW_ONE_SOURCE, 40), rng.integers(1, 50, size=40))
    # one pixel in source 0 against runs of 63 / 64 / 65 / 257 in the others
    put(0, ROW_LONE_PIXEL, [2000], 11)
    for s in range(1, k):
        size = RUN_LENGTHS[(s - 1) % len(RUN_LENGTHS)]
        put(s, ROW_LONE_PIXEL, some_columns(ROW_LONE_PIXEL, size), rng.integers(1, 50, size=size))
    # every column from the diagonal to the last bin in source 0, a few pixels in the others: every tile boundary
    put(0, ROW_DENSE, np.arange(ROW_DENSE, n), rng.integers(1, 9, size=n - ROW_DENSE))
    for s in range(1, k):
        put(s, ROW_DENSE, some_columns(ROW_DENSE, 5), rng.integers(1, 9, size=5))
    # stored zeros: zero in every source (dropped), zero in source 0 alone (dropped), zero that meets a count (kept, k > 1)
    for s in range(k):
        put(s, ROW_ZEROS, [COL_ZERO_IN_ALL], 0)
        put(s, ROW_ZEROS, [100 + s], 1 + s)
    put(0, ROW_ZEROS, [COL_ZERO_ALONE], 0)
    put(0, ROW_ZEROS, [COL_ZERO_MEETS_COUNT], 0)
    if k > 1:
        put(k - 1, ROW_ZEROS, [COL_ZERO_MEETS_COUNT], 5)
    # trans pixels: a row of the second chromosome with columns in the third, other columns in every source, some shared
    for s in range(k):
        cols = SIZES[0] + SIZES[1] + rng.choice(SIZES[2], size=30, replace=False)
        put(s, ROW_TRANS, cols, rng.integers(1, 20, size=30))
        put(s, ROW_TRANS, [n - 1 - s % 3], 7)
    # scattered rows, some beyond the second tile boundary
    for row in list(range(100, 160, 3)) + [2 * ASSUMED_TILE_COLUMNS + 90, n - 3]:
        for s in rng.choice(k, size=min(k, 3), replace=False).tolist():
            size = int(min(rng.integers(1, 60), n - row))
            put(s, row, some_columns(row, size), rng.integers(1, 50, size=size))
    out = []
    for s in range(k):
        keys = np.asarray(list(px[s].keys()), dtype=np.int64).reshape(-1, 2)
        out.append(make_cool(SIZES, keys[:, 0], keys[:, 1], np.asarray(list(px[s].values()), dtype=np.int64)))
    return out
