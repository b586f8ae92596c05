"""Adversarial pixel tables for the block staging (DeviceCool.stage_blocks / stage_intra / stage_inter) and what they must
stage to: decoded-cool dictionaries with the keys of tools.synthetic_genome.make_cool, built from seeds, each a genome of
several chromosomes with trans pixels stored (every block is a true view of a larger CSR), none above 3 000 bins.

The expectation of a block is oracle/detrend_oracle.py: balanced_band + prepare_band.  tests/test_staging_cases_host.py pins
these tables and expectations on the CPU (shapes present where the metadata says, the oracle's band route against a dense
restatement); tests/test_gpu_staging_oracle.py holds the device to them."""
import functools
from fractions import Fraction

import numpy as np

from oracle import detrend_oracle

MAX_VAL = 10.0
LARGEST = 17
SHAPES_KEEP = 60 + LARGEST            # the keep distance the row shapes of `row_shapes` are laid out for (max_dist 60)


class Case:
    """cool: the table; stagings: (max_dist, chromosomes or None for all) to stage with largest_kernel 17; smooth: the
    stagings also staged with smooth=True; exact: laws exact in any summation order (values held to 1e-13 relative, else
    1e-11 absolute); meta: where the shapes the case is about sit."""

    def __init__(self, name, cool, stagings, smooth=(), exact=False, val_dtype=np.float32, meta=None, symmetric=False):
        self.name, self.cool, self.stagings, self.smooth = name, cool, list(stagings), list(smooth)
        self.exact, self.val_dtype, self.meta, self.symmetric = exact, val_dtype, meta or {}, symmetric
        self._expected = {}

    @property
    def offsets(self):
        return np.asarray(self.cool["chrom_offset"], dtype=np.int64)

    def n(self, ci):
        return int(self.offsets[ci + 1] - self.offsets[ci])

    def chroms(self, staging):
        return list(range(len(self.offsets) - 1)) if staging[1] is None else list(staging[1])

    def expected(self, ci, keep, smooth=False):
        """(prepared band [n, keep + 1], law [keep + 1] with NaN on empty diagonals, detectable [n], uncapped ratio band)."""
        key = (ci, keep, bool(smooth))
        if key not in self._expected:
            band, det = detrend_oracle.balanced_band(self.cool, ci, keep)
            out, law = detrend_oracle.prepare_band(band, det, max_val=MAX_VAL, smooth=smooth)
            with np.errstate(all="ignore"):
                ratio = band / np.where(np.isnan(law), 0.0, law)[None, :]
            for a in (out, law, det, ratio):
                a.setflags(write=False)
            self._expected[key] = (out, law, det, ratio)
        return self._expected[key]


def keep_of(max_dist, n, largest=LARGEST):
    return min(max_dist, n) + largest


def geometry(max_dist, n, largest=LARGEST):
    """(keep, band?, band_w, ld) as the reference's keep distance and the project's layout rule give them: a band when it
    is less than half of the dense map; the pitch a multiple of 64 (band) / 16 (dense) that is no multiple of 4 KiB."""
    keep = keep_of(max_dist, n, largest)
    in_w = min(keep, n - 1) + 1
    out_w = min(max_dist, n - 1) + 1
    band = 2 * max(in_w, out_w) < n
    q = 64 if band else 16
    ld = ((in_w if band else n) + q - 1) // q * q
    if (ld * 8) % 4096 == 0:
        ld += q
    return keep, band, in_w if band else 0, ld


def expected_rows(case, ci, max_dist, smooth=False):
    """The staged buffer [n, ld] a block must equal, pitch included: band rows (slot = diagonal) or dense rows (slot =
    column, upper band only), zeros everywhere else.  Also returns the same array of uncapped ratios."""
    n = case.n(ci)
    keep, band, band_w, ld = geometry(max_dist, n)
    out, _, _, ratio = case.expected(ci, keep, smooth)
    rows, rat = np.zeros((n, ld)), np.zeros((n, ld))
    if band:
        rows[:, :band_w], rat[:, :band_w] = out[:, :band_w], ratio[:, :band_w]
        cols = np.arange(n)[:, None] + np.arange(band_w)[None, :]
        rat[:, :band_w][cols >= n] = 0.0
    else:
        for d in range(min(n, keep + 1)):
            i = np.arange(n - d)
            rows[i, i + d], rat[i, i + d] = out[i, d], ratio[i, d]
    return rows, rat


# ---------------------------------------------------------------------------------------------------------------------
def _finish(sizes, b1, b2, cnt, weight, binsize=1000, symmetric=False):
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)])
    b1, b2, cnt = np.asarray(b1, dtype=np.int64), np.asarray(b2, dtype=np.int64), np.asarray(cnt)
    key = b1 * int(off[-1]) + b2
    assert np.unique(key).size == key.size, "a pixel stored twice"
    assert np.all(b2 >= b1)
    if symmetric:                                           # the lower triangle stored as well (trans pixels mirrored too)
        offd = b2 > b1
        b1, b2, cnt = np.concatenate([b1, b2[offd]]), np.concatenate([b2, b1[offd]]), np.concatenate([cnt, cnt[offd]])
    order = np.lexsort((b2, b1))
    return {"binsize": binsize, "chrom_offset": off, "chrom_names": np.array([f"c{k}" for k in range(len(sizes))]),
            "bin1_id": b1[order], "bin2_id": b2[order], "count": cnt[order], "weight": np.asarray(weight, dtype=np.float64),
            "bin_start": np.concatenate([np.arange(s) * binsize for s in sizes]),
            "bin_end": np.concatenate([(np.arange(s) + 1) * binsize for s in sizes])}


class _Table:
    """Pixels by (bin1, bin2) in genome bins; a later set overwrites an earlier one."""

    def __init__(self, sizes):
        self.sizes = list(sizes)
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.px = {}

    def set(self, ci, r, c, v, cj=None):
        cj = ci if cj is None else cj
        assert 0 <= r < self.sizes[ci] and 0 <= c < self.sizes[cj]
        self.px[(int(self.off[ci] + r), int(self.off[cj] + c))] = v

    def clear_row(self, ci, r):
        g = int(self.off[ci] + r)
        for k in [k for k in self.px if k[0] == g]:
            del self.px[k]

    def background(self, rng, ci, reach, density, draw, zeros=0.0):
        n = self.sizes[ci]
        for r in range(n):
            for d in range(min(reach + 1, n - r)):
                if rng.random() < density:
                    self.set(ci, r, r + d, 0 if rng.random() < zeros else draw(d))

    def trans(self, rng, ca, cb, count, draw):
        for _ in range(count):
            self.set(ca, int(rng.integers(self.sizes[ca])), int(rng.integers(self.sizes[cb])), draw(0), cj=cb)

    def arrays(self, dtype):
        keys = sorted(self.px)
        b1 = np.array([k[0] for k in keys], dtype=np.int64)
        b2 = np.array([k[1] for k in keys], dtype=np.int64)
        return b1, b2, np.array([self.px[k] for k in keys], dtype=dtype)


def _log_weights(rng, n, lo=1e-3, hi=1e3):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _poisson(rng, scale=40.0):
    return lambda d: int(rng.poisson(scale / (d + 1.0)) + 1)


# ---------------------------------------------------------------------------------------------------------------------
def row_shapes(symmetric=False):
    """int32 counts, weights over 1e-3 .. 1e3; chromosome 1 (700 bins) carries every row shape, chromosome 2 is its dense
    twin: the same 700 bins with every pixel of the widest band stored and positive (what the poisoned-buffer stagings
    run first)."""
    rng = np.random.default_rng(7101)
    sizes = [40, 700, 700, 64]
    t = _Table(sizes)
    K = SHAPES_KEEP
    draw = _poisson(rng)
    t.background(rng, 0, 60, 0.6, draw, zeros=0.03)
    t.background(rng, 1, 230, 0.35, draw, zeros=0.03)
    t.background(rng, 3, 90, 0.6, draw)
    for r in range(700):                                    # the twin: nothing of its widest band is a gap
        for d in range(min(200 + LARGEST + 1, 700 - r)):
            t.set(2, r, r + d, draw(d))
    for ca, cb, k in [(0, 1, 150), (0, 2, 60), (0, 3, 40), (1, 2, 900), (1, 3, 300), (2, 3, 200)]:
        t.trans(rng, ca, cb, k, draw)
    ci = 1
    rows = {}
    nxt = iter(range(20, 600, 9))                           # the special rows, apart from one another

    def fresh():
        r = next(nxt)
        t.clear_row(ci, r)
        return r

    r = fresh()
    rows["empty"] = r
    r = fresh()
    rows["trans_only"] = r
    t.set(ci, r, 0, 5, cj=2)
    t.set(ci, r, 33, 2, cj=3)
    r = fresh()
    rows["beyond_keep"] = r
    for d in (K + 1, K + 2, K + 40):
        t.set(ci, r, r + d, draw(d))
    rows["first_d"] = {}
    for d0 in (0, 1, K - 1, K, K + 1):
        r = fresh()
        rows["first_d"][d0] = r
        for d in (d0, d0 + 1, d0 + 3):
            t.set(ci, r, r + d, draw(d))
        t.set(ci, r, 11, 3, cj=2)
    r = fresh()
    rows["single_last_diag"] = r
    t.set(ci, r, r + K, 4)
    rows["n_cis"] = {}
    for m in (1, 2, 63, 64, 65, 128, 129):
        r = fresh()
        rows["n_cis"][m] = r
        for d in range(m):
            t.set(ci, r, r + d, draw(d))
        t.set(ci, r, 5, 1, cj=3)
    rows["gaps"] = {}
    for gap in (1, 63, 64, 65, 136):                        # `gap` empty slots between two stored pixels
        r = fresh()
        rows["gaps"][gap] = (r, 2)
        for d in (0, 1, 2, 2 + gap + 1):
            t.set(ci, r, r + d, draw(d))
    rows["tail"] = list(range(700 - 12, 700))               # the band runs past the end; trans pixels follow at once
    for r in rows["tail"]:
        t.clear_row(ci, r)
        for d in range(700 - r):
            t.set(ci, r, r + d, draw(d))
        for c in range(0, 6):
            t.set(ci, r, c, 7, cj=2)
    b1, b2, cnt = t.arrays(np.int32)
    w = _log_weights(rng, sum(sizes))
    w[rng.choice(sum(sizes), 25, replace=False)] = np.nan
    special = [rows["empty"], rows["trans_only"], rows["beyond_keep"], rows["single_last_diag"], *rows["first_d"].values(),
               *rows["n_cis"].values(), *[g[0] for g in rows["gaps"].values()]]
    w[40 + np.array(special)] = np.where(np.isnan(w[40 + np.array(special)]), 1.0, w[40 + np.array(special)])
    w[740:1440] = np.where(np.isnan(w[740:1440]), 1.0, w[740:1440])        # the twin: every bin weighted, no pixel staged as 0
    cool = _finish(sizes, b1, b2, cnt, w, symmetric=symmetric)
    return Case("row_shapes" + ("_sym" if symmetric else ""), cool, [(60, None), (200, [1, 2]), (5, [0, 1, 3])],
                smooth=[(60, None)], val_dtype=np.float32, symmetric=symmetric,
                meta={"chrom": 1, "twin": 2, "keep": K, "rows": rows})


SIZES = [1, 2, 3, 16, 17, 18] + list(range(4, 41)) + [63, 64, 65, 255, 256, 257, 1031]


def sizes():
    """Every tail of the tiler's two-rows-per-wave loop, both sides of the band / dense choice and of keep = min(max_dist, n)
    + largest_kernel: float64 fractional counts."""
    rng = np.random.default_rng(7102)
    t = _Table(SIZES)
    draw = lambda d: float(rng.gamma(2.0, 8.0 / (d + 1.0)) + 0.01)          # noqa: E731
    for ci, n in enumerate(SIZES):
        t.background(rng, ci, 95, 0.7 if n < 300 else 0.4, draw, zeros=0.02)
    for ca in range(len(SIZES) - 1):
        t.trans(rng, ca, ca + 1, 3 + SIZES[ca] // 8, draw)
        t.set(ca, SIZES[ca] - 1, 0, 1.5, cj=ca + 1)         # a trans pixel right behind the last row's diagonal
    t.trans(rng, 0, len(SIZES) - 1, 1, draw)
    b1, b2, cnt = t.arrays(np.float64)
    w = _log_weights(rng, sum(SIZES), 0.05, 20.0)
    w[rng.choice(sum(SIZES), sum(SIZES) // 25, replace=False)] = np.nan
    stagings = [(1, None), (5, None), (60, None), (2000, None)]
    per_n = {}
    for ci, n in enumerate(SIZES):
        for md in (n - 1, n, n + 1):
            per_n.setdefault(md, []).append(ci)
    stagings += [(md, cs) for md, cs in sorted(per_n.items()) if md not in (1, 5, 60)]
    return Case("sizes", _finish(SIZES, b1, b2, cnt, w), stagings, smooth=[(5, None), (2000, None)], val_dtype=np.float64,
                meta={"sizes": SIZES})


def missing(symmetric=False):
    """NaN weights: isolated bins, runs of 1, 2, 17 and 64, the first and the last bin (chromosome 0); every second bin (1: its
    odd diagonals have an empty law although pixels are stored on them); a whole chromosome (2); one detectable bin (3)."""
    rng = np.random.default_rng(7103)
    sizes_ = [300, 200, 40, 120]
    t = _Table(sizes_)
    draw = _poisson(rng)
    for ci in range(4):
        t.background(rng, ci, 100, 0.8, draw, zeros=0.02)
    for ca, cb in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]:
        t.trans(rng, ca, cb, 80, draw)
    w = rng.normal(1.0, 0.2, sum(sizes_)).clip(0.3) * 0.05
    runs = {1: 20, 2: 30, 17: 50, 64: 100}
    gone = [0, 299, 10, 12, 85] + [s + k for m, s in runs.items() for k in range(m)]
    w[gone] = np.nan
    w[300 + np.arange(0, 200, 2)] = np.nan
    w[500:540] = np.nan
    w[540:660] = np.nan
    w[540 + 77] = 0.04
    b1, b2, cnt = t.arrays(np.int32)
    return Case("missing" + ("_sym" if symmetric else ""), _finish(sizes_, b1, b2, cnt, w, symmetric=symmetric),
                [(60, None), (5, None), (1, None)], smooth=[(60, None)], symmetric=symmetric,
                meta={"runs": runs, "isolated": [10, 12, 85], "ends": [0, 299], "alternate": 1, "all_nan": 2, "one_bin": (3, 77),
                      "empty_diags": {1: {"undetectable": list(range(1, 78, 2))}}})


def diagonals():
    """A kept diagonal with nothing stored (7), one whose stored pixels are all explicit zeros (9), one whose positive pixels
    all touch an undetectable bin (11), in chromosomes staged as a band (0) and dense (2)."""
    rng = np.random.default_rng(7104)
    sizes_ = [200, 150, 90]
    t = _Table(sizes_)
    draw = _poisson(rng)
    for ci in range(3):
        t.background(rng, ci, 80, 0.9, draw)
    t.trans(rng, 0, 1, 200, draw)
    t.trans(rng, 0, 2, 50, draw)
    t.trans(rng, 1, 2, 100, draw)
    w = rng.normal(1.0, 0.1, sum(sizes_)) * 0.1
    empty = {}
    for ci in (0, 2):
        n, s = sizes_[ci], int(t.off[ci])
        for r in range(n):
            t.px.pop((s + r, s + r + 7), None)
            if r + 9 < n:
                t.set(ci, r, r + 9, 0)
            t.px.pop((s + r, s + r + 11), None)
        bad = list(range(30, n - 11, 24))                   # bins apart by more than 11: the pixels (b, b + 11) touch one each
        for b in bad:
            t.set(ci, b, b + 11, 6)
            w[s + b] = np.nan
        empty[ci] = {"unstored": [7], "zeros": [9], "undetectable": [11]}
    b1, b2, cnt = t.arrays(np.int32)
    return Case("diagonals", _finish(sizes_, b1, b2, cnt, w), [(20, None), (60, None)], smooth=[(20, None)], meta={"empty_diags": empty})


def values_f32():
    """float32 fractional counts (staged as float64: they are not integers), explicit zeros, weights over 1e-3 .. 1e3."""
    rng = np.random.default_rng(7105)
    sizes_ = [120, 80, 30]
    t = _Table(sizes_)
    draw = lambda d: np.float32(rng.gamma(2.0, 5.0 / (d + 1.0)) + 0.01)     # noqa: E731
    for ci in range(3):
        t.background(rng, ci, 70, 0.7, draw, zeros=0.05)
    t.trans(rng, 0, 1, 90, draw)
    t.trans(rng, 0, 2, 30, draw)
    t.trans(rng, 1, 2, 30, draw)
    w = _log_weights(rng, sum(sizes_))
    w[[3, 60, 61, 150, 229]] = np.nan
    b1, b2, cnt = t.arrays(np.float32)
    return Case("values_f32", _finish(sizes_, b1, b2, cnt, w), [(10, None), (60, None)], smooth=[(10, None)], val_dtype=np.float64)


CAP_SETS = {"at": (10.0, 18), "below": (9.5, 17), "above": (10.5, 19)}    # (ratio, companions of 0.5): mean exactly 1.0


def cap_exact():
    """Unit weights, counts that are multiples of 0.5.  Every diagonal d has the law L = 1 (d even) or 2 (d odd), exactly and
    in any summation order: its positive pixels are sets of {10 L and eighteen 0.5 L}, {9.5 L, seventeen 0.5 L} and {10.5 L,
    nineteen 0.5 L} (each of mean L) and pixels of L itself -- all partial sums are small multiples of 0.25, exact in float64
    (and in float32).  So v / law is exactly 10 (capped), 9.5 (kept) or 10.5 (capped)."""
    rng = np.random.default_rng(7106)
    sizes_ = [150, 90, 40]
    t = _Table(sizes_)
    cap = []
    for ci, n in enumerate(sizes_):
        for d in range(min(n, 60 + LARGEST + 1)):
            law = 1.0 if d % 2 == 0 else 2.0
            slots = [int(r) for r in rng.permutation(n - d)]
            for kind, (ratio, mates) in CAP_SETS.items():
                if len(slots) < mates + 1:
                    continue
                r = slots.pop()
                t.set(ci, r, r + d, ratio * law)
                cap.append((ci, r, d, kind))
                for _ in range(mates):
                    r = slots.pop()
                    t.set(ci, r, r + d, 0.5 * law)
            for r in slots[:len(slots) // 2]:
                t.set(ci, r, r + d, law)
            for r in slots[len(slots) // 2:len(slots) // 2 + 2]:
                t.set(ci, r, r + d, 0.0)                    # explicit zeros: not part of the law
    t.trans(rng, 0, 1, 60, lambda d: 2.5)
    t.trans(rng, 0, 2, 20, lambda d: 0.5)
    t.trans(rng, 1, 2, 20, lambda d: 10.0)
    b1, b2, cnt = t.arrays(np.float64)
    return Case("cap_exact", _finish(sizes_, b1, b2, cnt, np.ones(sum(sizes_))), [(60, None), (10, None), (1, None)], exact=True,
                val_dtype=np.float64, meta={"cap": cap})


def exact_law(case, ci, keep):
    """The laws of a unit-weight case in exact rational arithmetic (None on an empty diagonal)."""
    off = case.offsets
    s, n = int(off[ci]), case.n(ci)
    sums, cnts = {}, {}
    for a, b, v in zip(case.cool["bin1_id"], case.cool["bin2_id"], case.cool["count"]):
        d = int(b - a)
        if s <= a < s + n and s <= b < s + n and 0 <= d <= keep and v > 0:
            sums[d] = sums.get(d, Fraction(0)) + Fraction(float(v))
            cnts[d] = cnts.get(d, 0) + 1
    return [sums[d] / cnts[d] if d in sums else None for d in range(min(n, keep + 1))]


BUILDERS = {
    "row_shapes": row_shapes, "row_shapes_sym": functools.partial(row_shapes, symmetric=True), "sizes": sizes,
    "missing": missing, "missing_sym": functools.partial(missing, symmetric=True), "diagonals": diagonals,
    "values_f32": values_f32, "cap_exact": cap_exact,
}
RANDOM_VALUED = [k for k in BUILDERS if k != "cap_exact"]


@functools.lru_cache(maxsize=None)
def get(name):
    """The case of that name, built once per process (its expectations are cached on it and read-only)."""
    return BUILDERS[name]()


# ---------------------------------------------------------------------------------------------------------------------
def trans_genome():
    """Trans blocks whose stored pixels number 0, 1, 2, odd and even, with tied middle values, explicit zeros, and a chromosome
    without any weight.  meta["pairs"]: (ca, cb) -> stored pixels."""
    rng = np.random.default_rng(7107)
    sizes_ = [50, 33, 70, 21, 40, 16]
    t = _Table(sizes_)
    draw = _poisson(rng)
    for ci in range(len(sizes_)):
        t.background(rng, ci, 20, 0.5, draw)

    def fill(ca, cb, values):
        cells = rng.choice(sizes_[ca] * sizes_[cb], len(values), replace=False)
        for cell, v in zip(cells, values):
            t.set(ca, int(cell) // sizes_[cb], int(cell) % sizes_[cb], v, cj=cb)

    plan = {(0, 1): [], (0, 2): [4], (0, 3): [3, 9], (1, 2): [int(v) for v in rng.integers(1, 30, 101)],
            (1, 3): [int(v) for v in rng.integers(1, 30, 64)], (2, 3): [5] * 20 + [1, 2, 3, 50, 60, 70, 80] + [0] * 4,     # tied middle
            (2, 5): [7, 7, 7, 7, 1, 2, 30, 40] + [0, 0], (0, 4): [int(v) for v in rng.integers(1, 9, 40)],
            (3, 4): [2, 8, 5], (3, 5): [int(v) for v in rng.integers(0, 4, 90)] + [6] * 100}
    for (ca, cb), values in plan.items():
        fill(ca, cb, values)
    w = rng.normal(1.0, 0.15, sum(sizes_)).clip(0.4)
    for ci in (2, 3, 5):                                    # unit weights: tied counts stay tied after balancing
        w[int(t.off[ci]):int(t.off[ci + 1])] = 1.0
    w[int(t.off[4]):int(t.off[5])] = np.nan                # chromosome 4: no weight at all
    w[[2, 60, 100, 160]] = np.nan
    b1, b2, cnt = t.arrays(np.int32)
    return Case("trans", _finish(sizes_, b1, b2, cnt, w), [], meta={"pairs": {k: len(v) for k, v in plan.items()}})


def trans_block(cool, ca, cb):
    """(dense block, median, stored pixels): count * w1 * w2, NaN -> 0, over the median of the stored values (numpy's: the mean
    of the two middle values of an even number; NaN when nothing is stored), NaN -> 0 again (0 / 0)."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    b1, b2 = np.asarray(cool["bin1_id"]), np.asarray(cool["bin2_id"])
    cnt, w = np.asarray(cool["count"], dtype=np.float64), np.asarray(cool["weight"], dtype=np.float64)
    s1, e1, s2, e2 = int(off[ca]), int(off[ca + 1]), int(off[cb]), int(off[cb + 1])
    sel = (b1 >= s1) & (b1 < e1) & (b2 >= s2) & (b2 < e2)
    with np.errstate(invalid="ignore"):
        vals = cnt[sel] * w[b1[sel]] * w[b2[sel]]
    vals = np.where(np.isnan(vals), 0.0, vals)
    med = float(np.median(vals)) if vals.size else float("nan")
    dense = np.zeros((e1 - s1, e2 - s2))
    with np.errstate(all="ignore"):
        dense[b1[sel] - s1, b2[sel] - s2] = vals / med
    dense[np.isnan(dense)] = 0.0
    return dense, med, int(sel.sum())
