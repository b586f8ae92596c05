"""Edge-case pixel tables for ICE balancing (chromosight_amd/balance.py -> cs_ice_balance, cs_balance.hip) and a second
reference to hold the yardstick to: small seeded upper-triangle tables of integer counts, without weights, as the dict
pipeline.DeviceCool takes; a table of cases (name, table, ice_balance keywords, what the case is for); and `dense_reference`,
ICE on the dense symmetric matrix of every span in extended precision, which shares nothing with ice_restatement
(tests/test_balance_host.py) but the definition of the operation.

tests/test_balance_cases_host.py pins the cases on the CPU (the two references agree, every case reaches the branch it is named
for, no variance sits near tol); tests/test_gpu_balance_cases.py holds the device to ice_restatement on them."""
import functools
import math

import numpy as np

from test_balance_host import ice_restatement

LONG_BINS = 16_449                # 258 chunks of 64 bins: the span kernel's 256 threads take a second trip


def make_table(sizes, band, density, seed, *, mean=40.0, trans=0, straddle=0, zeros=0.0, zero_bins=(), diag_only=(), empty=(),
               scaled=None, binsize=1000):
    """An upper-triangle pixel table, sorted by (bin1, bin2), integer counts, no weights.

    sizes: bins per chromosome (0 allowed).  band, density, mean: per chromosome or one for all -- the pixels (r, r + d),
    0 <= d <= band, are stored with probability `density`, count 1 + Poisson(mean / sqrt(1 + d)).  straddle: the band runs on
    over a chromosome's end into the first `straddle` bins behind it (trans pixels right behind a row's last cis pixel);
    trans: that many more trans pixels anywhere.  zeros: fraction of the stored counts set to 0; zero_bins: bins 90 % of whose
    pixels are set to 0.  diag_only: chromosomes that store their main diagonal, whole, and no other cis pixel; empty:
    chromosomes no pixel touches.  scaled: {bin: factor}, the counts of the bin's pixels multiplied (rounded, at least 1)."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, dtype=np.int64)
    n_chrom = sizes.size
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(off[-1])
    chrom = np.repeat(np.arange(n_chrom), sizes)
    band_c = np.broadcast_to(np.asarray(band, dtype=np.int64), (n_chrom,))
    dens_c = np.broadcast_to(np.asarray(density, dtype=np.float64), (n_chrom,))
    mean_c = np.broadcast_to(np.asarray(mean, dtype=np.float64), (n_chrom,))
    width = int(band_c.max()) + 1
    r = np.repeat(np.arange(n, dtype=np.int64), width)
    d = np.tile(np.arange(width, dtype=np.int64), n)
    inside = r + d < n
    r, d = r[inside], d[inside]
    c = r + d
    cr = chrom[r]
    end = off[cr + 1]
    only_diag = np.isin(cr, list(diag_only))
    keep = (d <= band_c[cr]) & (rng.random(r.size) < dens_c[cr]) & ((c < end) | (c - end < straddle))
    keep = np.where(only_diag & (c < end), d == 0, keep)
    r, c, d = r[keep], c[keep], d[keep]
    cnt = 1 + rng.poisson(mean_c[chrom[r]] / np.sqrt(1.0 + d))
    if trans:
        a, b = rng.integers(0, n, trans), rng.integers(0, n, trans)
        a, b = np.minimum(a, b), np.maximum(a, b)
        far = chrom[a] != chrom[b]
        r, c = np.concatenate([r, a[far]]), np.concatenate([c, b[far]])
        cnt = np.concatenate([cnt, 1 + rng.poisson(3.0, int(far.sum()))])
    _, first = np.unique(r * n + c, return_index=True)        # (sorted by (bin1, bin2); a pixel drawn twice stored once)
    r, c, cnt = r[first], c[first], cnt[first]
    touched = np.isin(chrom[r], list(empty)) | np.isin(chrom[c], list(empty))
    r, c, cnt = r[~touched], c[~touched], cnt[~touched]
    if scaled:
        f = np.ones(n)
        f[list(scaled)] = list(scaled.values())
        cnt = np.maximum(1, np.rint(cnt * f[r] * f[c])).astype(np.int64)
    cnt[rng.random(cnt.size) < zeros] = 0
    zb = np.isin(r, list(zero_bins)) | np.isin(c, list(zero_bins))
    cnt[zb & (rng.random(cnt.size) < 0.9)] = 0
    return {"binsize": binsize, "chrom_offset": off, "chrom_names": np.array([f"c{k}" for k in range(n_chrom)]),
            "bin1_id": r, "bin2_id": c, "count": cnt.astype(np.int32),
            "bin_start": np.concatenate([np.arange(s) * binsize for s in sizes]) if n_chrom else np.zeros(0, dtype=np.int64),
            "bin_end": np.concatenate([(np.arange(s) + 1) * binsize for s in sizes]) if n_chrom else np.zeros(0, dtype=np.int64)}


# ---------------------------------------------------------------------------------------------------------------------
# bins whose marginal is scaled down: far enough below the median for the MAD filter (mad), or slow to balance (timing)
MAD_BINS = [17, 64, 65, 130, 199, 200, 260, 349]
SLOW_BINS = list(range(5, 200, 9))
ZERO_BINS = [10, 63, 64, 120, 149, 150, 201]

TABLES = {
    # every chunk tail: a chromosome of 1, 63, 64, 65 bins, one of none, and 129 (three chunks, the last of one bin)
    "geometry": dict(sizes=[1, 63, 64, 65, 0, 129], band=12, density=0.8, mean=8.0, seed=9101, straddle=3, trans=40),
    # rows and CSC columns of up to 201 pixels (more than two trips of a wave's lane-strided loop), trans pixels, straddling rows
    "wide": dict(sizes=[400, 150], band=[200, 40], density=0.85, seed=9102, straddle=5, trans=3000),
    "trans": dict(sizes=[100, 80, 120], band=30, density=0.8, seed=9103, straddle=8, trans=600),
    "mad": dict(sizes=[200, 150], band=40, density=0.8, seed=9104, trans=80, scaled={b: 0.03 for b in MAD_BINS}),
    "zeros": dict(sizes=[150, 100], band=30, density=0.8, seed=9105, zeros=0.1, zero_bins=ZERO_BINS, trans=50),
    # chromosome 1: at most 8 pixels per bin; 3: its main diagonal only; 5: no pixel at all
    "nothing": dict(sizes=[120, 60, 90, 50, 70, 40], band=[30, 3, 30, 0, 30, 30], density=[0.8, 1.0, 0.8, 1.0, 0.8, 0.8],
                    seed=9106, diag_only=(3,), empty=(5,), trans=60),
    # chromosome 0 has bins five times below the rest and few counts, chromosome 1 is even and deep, chromosome 2 is one chunk
    "timing": dict(sizes=[200, 200, 64], band=[25, 60, 30], density=[0.6, 1.0, 0.9], mean=[4.0, 4000.0, 40.0], seed=9107,
                   scaled={b: 0.2 for b in SLOW_BINS}),
    "long": dict(sizes=[LONG_BINS, 70], band=[3, 20], density=0.9, mean=[6.0, 40.0], seed=9108, trans=200, straddle=2),
}


@functools.lru_cache(maxsize=None)
def table(name):
    """The table of that name, built once per process and read-only."""
    cool = make_table(**TABLES[name])
    for v in cool.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cool


class Case:
    def __init__(self, name, table_name, kw, purpose):
        self.name, self.table, self.kw, self.purpose = name, table_name, dict(kw), purpose

    @property
    def cool(self):
        return table(self.table)

    @property
    def dense(self):
        """Held to dense_reference as well (all but the long span: its dense matrix would take 2 GB)."""
        return self.table != "long"

    @property
    def reference(self):
        """ice_restatement's (weights, info) for the case: computed once, read-only."""
        return _reference(self.name)


CASES = [Case(*c) for c in [
    ("geometry_d0", "geometry", dict(ignore_diags=0, min_nnz=0), "chunks of 1, 63, 64, 65, 0 and 129 bins; the 1-bin chromosome keeps its diagonal pixel"),
    ("geometry_d2", "geometry", dict(min_nnz=4), "the same chunks; the 1-bin and the 0-bin chromosome are empty spans"),
    ("geometry_genome", "geometry", dict(cis_only=False, min_nnz=4), "one span over chromosomes that end inside chunks, trans pixels kept"),
    ("wide_d1", "wide", dict(ignore_diags=1), "rows and columns of more than 128 kept pixels; row and column filter agree at 1"),
    ("wide_d3", "wide", dict(ignore_diags=3), "... at 3"),
    ("wide_d7", "wide", dict(ignore_diags=7), "... at 7"),
    ("wide_genome_d3", "wide", dict(ignore_diags=3, cis_only=False), "long rows whose trans pixels count"),
    ("trans_cis", "trans", dict(), "trans pixels stored and dropped: rows that straddle their chromosome's last bin"),
    ("trans_loose_tol", "trans", dict(tol=1e-2), "a loose tol: few iterations"),
    ("trans_no_rescale", "trans", dict(rescale_marginals=False), "rescale_marginals=False"),
    ("trans_genome_no_rescale", "trans", dict(rescale_marginals=False, cis_only=False, ignore_diags=1, max_iters=400), "... genome-wide"),
    ("mad_default", "mad", dict(min_nnz=0), "the MAD filter removes bins"),
    ("mad_off", "mad", dict(min_nnz=0, mad_max=0), "mad_max=0 keeps them"),
    ("mad_min_count", "mad", dict(min_nnz=0, mad_max=0, min_count=302), "min_count removes them instead; the lowest of the other bins has exactly that marginal"),
    ("zeros_min_nnz", "zeros", dict(mad_max=0), "explicit zeros stored: bins fall below min_nnz although they have the pixels"),
    ("nothing_d2", "nothing", dict(), "an all-filtered chromosome, a diagonal-only one (an empty span) and one without pixels"),
    ("nothing_min_nnz4", "nothing", dict(min_nnz=4), "bins of exactly min_nnz pixels (kept) beside bins of one fewer (dropped)"),
    ("nothing_d0", "nothing", dict(ignore_diags=0, min_nnz=0, max_iters=100), "the diagonal-only chromosome oscillates up to max_iters; its neighbours converge"),
    ("timing", "timing", dict(ignore_diags=1, min_nnz=0, mad_max=0), "spans that stop at very different iterations: frozen chunks, the running-span counter reaching 0"),
    ("long_span", "long", dict(ignore_diags=1, min_nnz=2), "a cis span of 258 chunks"),
]]
BY_NAME = {c.name: c for c in CASES}
DENSE = [c.name for c in CASES if c.dense]


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = BY_NAME[name]
    w, info = ice_restatement(case.cool, **case.kw)
    w.setflags(write=False)
    return w, info


def unconverged(info):
    return [k for k, c in enumerate(info["converged"]) if not c]


# ---------------------------------------------------------------------------------------------------------------------
def relocate(cool, order, front=()):
    """The same chromosomes in another order, behind pixel-less chromosomes of `front` bins each.  Returns (table, new first
    bin of every old chromosome).  A trans pixel whose chromosomes change places is stored the other way round (upper triangle)."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    old = np.diff(off)
    sizes = np.concatenate([np.asarray(front, dtype=np.int64), old[list(order)]])
    new_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    start = np.zeros(old.size, dtype=np.int64)
    start[list(order)] = new_off[len(front):-1]
    chrom = np.repeat(np.arange(old.size), old)
    shift = (start - off[:-1])[chrom]
    a, b = cool["bin1_id"] + shift[cool["bin1_id"]], cool["bin2_id"] + shift[cool["bin2_id"]]
    a, b = np.minimum(a, b), np.maximum(a, b)
    srt = np.lexsort((b, a))
    names = [f"front{k}" for k in range(len(front))] + [str(cool["chrom_names"][k]) for k in order]
    return {"binsize": cool["binsize"], "chrom_offset": new_off, "chrom_names": np.array(names), "bin1_id": a[srt], "bin2_id": b[srt],
            "count": cool["count"][srt], "bin_start": np.concatenate([np.arange(s) * cool["binsize"] for s in sizes]),
            "bin_end": np.concatenate([(np.arange(s) + 1) * cool["binsize"] for s in sizes])}, start


def without_trans(cool):
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))
    cis = chrom[cool["bin1_id"]] == chrom[cool["bin2_id"]]
    out = dict(cool)
    for k in ("bin1_id", "bin2_id", "count"):
        out[k] = cool[k][cis]
    return out


# ---------------------------------------------------------------------------------------------------------------------
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def _row_sums(p):
    if WIDE:
        return p.sum(axis=1)
    return np.array([math.fsum(row) for row in p], dtype=np.longdouble)


def _total(x):
    return x.sum() if WIDE else np.longdouble(math.fsum(x))


def _median(values):
    v = sorted(values)
    if not v:
        return math.nan
    h = len(v) // 2
    return v[h] if len(v) % 2 else (v[h - 1] + v[h]) / 2.0


def dense_reference(cool, cis_only=True, mad_max=5, min_nnz=10, min_count=0, ignore_diags=2, tol=1e-5, max_iters=200,
                    rescale_marginals=True):
    """ICE as cooler.balance_cooler defines it, on dense matrices: per span the symmetric matrix U + U^T of the kept pixels (a
    diagonal pixel twice: it adds to the marginal of both of its bins, which are one), the filters as masks over bins, the
    marginals dense row sums in np.longdouble (math.fsum where that is no wider than float64).  Returns (weights, info)."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    n = int(off[-1])
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))
    upper = np.zeros((n, n))
    upper[cool["bin1_id"], cool["bin2_id"]] = cool["count"]
    i, j = np.indices((n, n))
    kept = j - i >= ignore_diags
    if cis_only:
        kept &= chrom[:, None] == chrom[None, :]
    upper[~kept] = 0.0
    sym = upper + upper.T
    stored = (upper != 0).astype(np.float64)
    total = sym.sum(axis=1)                                 # (integers: exact)
    nonzero = (stored + stored.T).sum(axis=1)
    alive = np.ones(n, dtype=bool)
    if min_nnz > 0:
        alive &= nonzero >= min_nnz
    if min_count > 0:
        alive &= total >= min_count
    if mad_max > 0:
        scaled = np.full(n, math.nan)
        for lo, hi in zip(off[:-1], off[1:]):
            med = _median([float(x) for x in total[lo:hi] if x > 0])
            if not math.isnan(med):
                scaled[lo:hi] = total[lo:hi] / med
        logs = [math.log(x) for x in scaled if x > 0]
        if logs:
            med = _median(logs)
            spread = _median([abs(x - med) for x in logs])
            alive &= ~(scaled < math.exp(med - mad_max * spread))
    weights = np.full(n, math.nan)
    info = {"iterations": [], "var": [], "scale": [], "converged": []}
    for lo, hi in (zip(off[:-1], off[1:]) if cis_only else [(0, n)]):
        a = sym[lo:hi, lo:hi].astype(np.longdouble)
        b = alive[lo:hi].astype(np.longdouble)
        done, conv, var, mean = 0, False, np.longdouble(0), np.longdouble(math.nan)
        some = False
        while done < max_iters:
            done += 1
            m = _row_sums(a * b[:, None] * b[None, :])
            on = m != 0
            some = bool(on.any())
            if not some:
                var, conv, mean = np.longdouble(0), True, np.longdouble(math.nan)
                break
            mean = _total(m[on]) / on.sum()
            var = _total((m[on] - mean) ** 2) / on.sum()
            b = np.where(on, b / np.where(on, m / mean, 1), b)
            if var < tol:
                conv = True
                break
        if some:
            w = np.where(b == 0, np.longdouble(math.nan), b)
            weights[lo:hi] = (w / np.sqrt(mean) if rescale_marginals else w).astype(np.float64)
        for k, x in zip(("iterations", "var", "scale", "converged"), (done, float(var), float(mean), conv)):
            info[k].append(x)
    return weights, info
