"""Trans blocks for the row-strip route of `detect --inter` / `quantify --inter` (pipeline.detect_inter_block):

- occupancy_reference: numpy restatement of cs_csr_tile_occupancy (which 64 x 64 output tiles a stored pixel reaches);
- occupancy_brute: the same from the dense map by brute-force dilation (what the restatement is checked against);
- make_trans_cool: a decoded-.cool dictionary with a short intra band and sparse trans contacts with planted trans patterns,
  chromosomes in hg38 proportions (tools/synthetic_genome.py HG38_MB)."""
import numpy as np

from tools.synthetic_genome import genome_sizes

TILE = 64


def _survives(vals, row_w, col_w):
    with np.errstate(invalid="ignore"):
        return (vals > 0) & np.isfinite(row_w) & np.isfinite(col_w)


def occupancy_reference(rows, cols, vals, row_w, col_w, n_cols, km, kn, row_begin, row_end):
    """Sorted tile indices ty * ceil(n_cols / 64) + tx of the output rows row_begin .. row_end - 1 whose windows of a km x kn
    template reach a stored pixel (rows[k], cols[k]) (block coordinates) with vals > 0 and finite row / column weights."""
    tiles_x = -(-int(n_cols) // TILE)
    kh, kw = (km - 1) // 2, (kn - 1) // 2
    up, left = km - 1 - kh, kn - 1 - kw
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    ok = _survives(np.asarray(vals, dtype=np.float64), np.asarray(row_w, dtype=np.float64), np.asarray(col_w, dtype=np.float64))
    ok &= (cols >= 0) & (cols < n_cols)
    rows, cols = rows[ok], cols[ok]
    i_lo, i_hi = np.maximum(rows - up, row_begin), np.minimum(rows + kh, row_end - 1)
    j_lo, j_hi = np.maximum(cols - left, 0), np.minimum(cols + kw, n_cols - 1)
    live = i_lo <= i_hi
    out = set()
    for a, b, c, d in zip(i_lo[live], i_hi[live], j_lo[live], j_hi[live]):
        for ty in range((a - row_begin) // TILE, (b - row_begin) // TILE + 1):
            for tx in range(c // TILE, d // TILE + 1):
                out.add(ty * tiles_x + tx)
    return np.array(sorted(out), dtype=np.int64)


def occupancy_brute(dense_ok, km, kn, row_begin, row_end):
    """The same from a boolean map of surviving pixels (all rows of the block): an output pixel is live when its window holds
    one; a tile is listed when one of its output pixels is live."""
    dense_ok = np.asarray(dense_ok, dtype=bool)
    n_r, n_c = dense_ok.shape
    kh, kw = (km - 1) // 2, (kn - 1) // 2
    pad = np.zeros((n_r + km, n_c + kn), dtype=np.int64)
    pad[kh:kh + n_r, kw:kw + n_c] = dense_ok
    c = np.zeros((pad.shape[0] + 1, pad.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = pad.cumsum(0).cumsum(1)
    # window of output (i, j): padded rows i .. i + km - 1, columns j .. j + kn - 1
    live = (c[km:km + n_r, kn:kn + n_c] - c[:n_r, kn:kn + n_c] - c[km:km + n_r, :n_c] + c[:n_r, :n_c]) > 0
    live = live[row_begin:row_end]
    tiles_x = -(-n_c // TILE)
    out = []
    for ty in range(-(-(row_end - row_begin) // TILE)):
        for tx in range(tiles_x):
            if live[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].any():
                out.append(ty * tiles_x + tx)
    return np.array(out, dtype=np.int64)


def trans_chrom_sizes(total_bins=310_000, n_chroms=24):
    """Chromosome sizes in bins of make_trans_cool's default genome: hg38 proportions, chrX last, chrY small."""
    mb = np.asarray(list(np.asarray(genome_sizes(1_000_000))[:23]) + [57 * 1_000_000 / 3_100], dtype=np.float64)[:n_chroms]
    return np.maximum((mb / mb.sum() * total_bins).astype(np.int64), 256)


def make_trans_cool(total_bins=310_000, n_chroms=24, intra_diags=200, n_trans=20_000_000, n_planted=40, template=None, binsize=10_000,
                    seed=5, chrom_sizes=None):
    """Decoded-.cool dictionary: chromosomes in hg38 proportions (chrX last, chrY small), an intra band of `intra_diags`
    diagonals (Poisson, 1/(d+1) law), ~n_trans sparse trans contacts (Poisson counts at uniform random pixels of the upper
    trans area) and n_planted trans patterns (the template, scaled, added around random trans pixels).  Weights are 1.0
    with 1 % missing bins.  Returns (cool, planted [(bin1, bin2)] genome-wide)."""
    rng = np.random.default_rng(seed)
    if chrom_sizes is None:
        chrom_sizes = trans_chrom_sizes(total_bins, n_chroms)
    sizes = np.asarray(chrom_sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    n = int(off[-1])
    chrom_of = np.repeat(np.arange(sizes.size), sizes)
    b1l, b2l, cl = [], [], []
    # intra band
    d = np.arange(intra_diags)
    for c, m in enumerate(sizes.tolist()):
        rows = np.repeat(np.arange(m), intra_diags)
        cols = rows + np.tile(d, m)
        cnt = rng.poisson(20.0 / (np.tile(d, m) + 1.0))
        ok = (cols < m) & (cnt > 0)
        b1l.append(rows[ok] + off[c])
        b2l.append(cols[ok] + off[c])
        cl.append(cnt[ok].astype(np.int32))
    # sparse trans contacts: pixels drawn uniformly over the upper trans area
    r = rng.integers(0, n, size=int(n_trans) * 2)
    q = rng.integers(0, n, size=int(n_trans) * 2)
    lo, hi = np.minimum(r, q), np.maximum(r, q)
    keep = chrom_of[lo] != chrom_of[hi]
    lo, hi = lo[keep][:int(n_trans)], hi[keep][:int(n_trans)]
    b1l.append(lo)
    b2l.append(hi)
    cl.append(rng.integers(1, 3, size=lo.size).astype(np.int32))
    planted = []
    if template is not None and n_planted:
        t = np.asarray(template, dtype=np.float64)
        t = np.round(8 * (t - t.min()) / (t.max() - t.min())).astype(np.int32)
        kh, kw = t.shape[0] // 2, t.shape[1] // 2
        ii, jj = np.nonzero(t > 0)
        while len(planted) < n_planted:
            ca, cb = np.sort(rng.choice(sizes.size, 2, replace=False))
            i = int(rng.integers(kh + 2, sizes[ca] - kh - 2))
            j = int(rng.integers(kw + 2, sizes[cb] - kw - 2))
            planted.append((int(off[ca] + i), int(off[cb] + j)))
            b1l.append(off[ca] + i - kh + ii)
            b2l.append(off[cb] + j - kw + jj)
            cl.append(t[ii, jj].astype(np.int32))
    b1 = np.concatenate(b1l).astype(np.int64)
    b2 = np.concatenate(b2l).astype(np.int64)
    cnt = np.concatenate(cl).astype(np.int64)
    # one pixel per (bin1, bin2): duplicates summed
    key = b1 * n + b2
    uk, inv = np.unique(key, return_inverse=True)
    cnt = np.bincount(inv, weights=cnt).astype(np.int32)
    b1, b2 = uk // n, uk % n
    weight = np.ones(n)
    weight[rng.choice(n, n // 100, replace=False)] = np.nan
    cool = {"binsize": binsize, "chrom_offset": off, "chrom_names": np.array([f"chr{c + 1}" for c in range(sizes.size)]),
            "bin1_id": b1, "bin2_id": b2, "count": cnt, "weight": weight,
            "bin_start": np.concatenate([np.arange(s) * binsize for s in sizes]),
            "bin_end": np.concatenate([(np.arange(s) + 1) * binsize for s in sizes])}
    return cool, planted
