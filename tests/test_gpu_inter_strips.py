"""Trans blocks in row strips on the device (pipeline.detect_inter_block / quantify_inter_block): the occupancy list of
cs_csr_tile_occupancy against its numpy restatement, cs_candidates_tiles on that list against the full tile list, and
detect / quantify --inter through strips against the per-block route of resident trans blocks."""
import copy
import time

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import engine, pipeline
from oracle import foci_oracle
from oracle import pearson_oracle as orc
from chromosight_amd.utils import detection as cid
from tools.synthetic_inter import make_trans_cool, occupancy_reference

pytestmark = pytest.mark.gpu

LOOPS = np.asarray(ck.loops["kernels"][0], dtype=np.float64)


@pytest.fixture(scope="module")
def small():
    cool, planted = make_trans_cool(n_chroms=4, intra_diags=30, n_trans=400, n_planted=8, template=LOOPS, binsize=1000, seed=11,
                                    chrom_sizes=[701, 853, 599, 947])          # (odd column counts)
    return cool, planted


def _block_pixels(cool, dcool, ca, cb, ra, rb):
    off = dcool.offsets
    b1, b2 = np.asarray(cool["bin1_id"]), np.asarray(cool["bin2_id"])
    cnt, w = np.asarray(cool["count"], dtype=np.float64), np.asarray(cool["weight"])
    sel = (b1 >= off[ca] + ra) & (b1 < off[ca] + rb) & (b2 >= off[cb]) & (b2 < off[cb + 1])
    return b1[sel] - off[ca], b2[sel] - off[cb], cnt[sel], w[b1[sel]], w[b2[sel]]


@pytest.mark.parametrize("tmpl", [(17, 17), (7, 17), (21, 9)])
def test_device_occupancy_matches_numpy(small, tmpl):
    cool, _ = small
    dcool = pipeline.DeviceCool(cool)
    km, kn = tmpl
    reach = pipeline._strip_reach([np.zeros(tmpl)])
    halo = (reach - 1) // 2
    checked = 0
    for ca, cb in [(0, 1), (0, 3), (2, 3)]:
        n_r, n_c = dcool.chrom_size(ca), dcool.chrom_size(cb)
        for rows in [(0, n_r), (0, 70), (n_r // 3, n_r // 3 + 200), (n_r - 90, n_r)]:
            blk = dcool.stage_inter(ca, cb, rows=rows, largest_kernel=reach)
            got = []
            for _ in range(2):
                tiles, nt = engine.run_tile_occupancy(dcool.dev, blk.view, blk.view_row0, km, kn, rows, n_c)
                got.append(tiles.download()[:nt].astype(np.int64))
            assert np.array_equal(got[0], got[1])                       # the same list from run to run
            ra, rb = max(0, rows[0] - halo), min(n_r, rows[1] + halo)
            r, c, v, wr, wc = _block_pixels(cool, dcool, ca, cb, ra, rb)
            want = occupancy_reference(r, c, v, wr, wc, n_c, km, kn, rows[0], rows[1])
            assert np.array_equal(got[0], want), (ca, cb, rows)
            checked += want.size
    assert checked > 0


KERNEL_MFMA_LIST = 8            # include/chromosight_hip.h CS_KERNEL_MFMA_LIST
ASYM = LOOPS + 0.05 * np.arange(17)[:, None]            # 17 x 17 whose rows do not mirror: the list instance without RSYM


@pytest.mark.parametrize("pearson", [0.3, 0.1, 0.0])
@pytest.mark.parametrize("tmpl", ["loops", "asym", "nonsquare"])
def test_candidates_on_the_occupancy_list_equal_the_full_list(small, pearson, tmpl):
    """pearson 0.3: float32 candidates from the list instance of the tile kernel (checked: cs_last_kernel), RSYM (the loops
    template, rows mirror) and not (asym); pearson <= 0.1: float64 maps filtered by the list.  Odd column counts, row windows
    that start and end off the 64-row grid."""
    cool, _ = small
    dcool = pipeline.DeviceCool(cool)
    kernel = {"loops": LOOPS, "asym": ASYM, "nonsquare": LOOPS[5:12, :]}[tmpl]
    assert (tmpl == "loops") == np.array_equal(kernel, kernel[::-1]) or tmpl == "nonsquare"
    kspec = engine.KernelSpec(kernel)
    reach = pipeline._strip_reach([kernel])
    cfg = dict(ck.loops, pearson=pearson)
    list_path = pearson > 0.1 and tmpl != "nonsquare"
    n_cand = skipped = 0
    for ca, cb in [(0, 1), (1, 2), (0, 3), (2, 3)]:
        n_r, n_c = dcool.chrom_size(ca), dcool.chrom_size(cb)
        assert n_c % 2 == 1
        for rows in [(0, n_r), (n_r // 4 + 3, n_r // 4 + 153), (n_r - 77, n_r)]:
            blk = dcool.stage_inter(ca, cb, rows=rows, largest_kernel=reach)
            tiles, nt = engine.run_tile_occupancy(dcool.dev, blk.view, blk.view_row0, kspec.km, kspec.kn, rows, n_c)
            n_all = -(-n_c // 64) * -(-(rows[1] - rows[0]) // 64)
            every = dcool.dev.to_device(np.arange(n_all, dtype=np.int32))
            common = pipeline._strip_common(blk, cfg)
            kw = dict(pearson=pearson, lo_diag=-(n_r - 1), hi_diag=n_c - 1, **common)
            got = engine.run_candidates_tiles(dcool.dev, blk.sig, (n_r, n_c), kspec, rows, tiles, nt, **kw)
            if list_path and nt:
                assert dcool.dev.lib.cs_last_kernel(dcool.dev.ctx) == KERNEL_MFMA_LIST
            ref = engine.run_candidates_tiles(dcool.dev, blk.sig, (n_r, n_c), kspec, rows, every, n_all, **kw)
            if list_path:
                assert dcool.dev.lib.cs_last_kernel(dcool.dev.ctx) == KERNEL_MFMA_LIST
            plain = engine.run_candidates(dcool.dev, blk.sig, (n_r, n_c), kspec, rows, **kw)
            for a, b in zip(got, ref):
                assert np.array_equal(a, b)
            for a, b in zip(got, plain):
                assert np.array_equal(a, b)
            assert np.array_equal(got[2].view(np.int64), ref[2].view(np.int64))      # bit-identical values
            n_cand += got[0].size
            skipped += n_all - nt
    assert n_cand > 0 and skipped > 0
    print(f"{tmpl}, pearson {pearson}: {n_cand} candidates, {skipped} tiles skipped")


def _oracle_block(cool, off, ca, cb, kernel, cfg, rows=None, halo=0):
    """foci_oracle.detect_table (inter=True) on the trans block (ca, cb) built on the host from the pixel table: count * w1 * w2,
    NaN -> 0, divided by the median of the block's stored values (NaN counted as 0).  rows = (a, b): only the rows a - halo ..
    b + halo - 1 (a crop; its records are block-local).  Returns (table (k, 3), windows, median)."""
    b1, b2 = np.asarray(cool["bin1_id"]), np.asarray(cool["bin2_id"])
    cnt, w = np.asarray(cool["count"], dtype=np.float64), np.asarray(cool["weight"], dtype=np.float64)
    s1, e1, s2, e2 = int(off[ca]), int(off[ca + 1]), int(off[cb]), int(off[cb + 1])
    sel = (b1 >= s1) & (b1 < e1) & (b2 >= s2) & (b2 < e2)
    with np.errstate(invalid="ignore"):
        vals = cnt[sel] * w[b1[sel]] * w[b2[sel]]
    vals = np.where(np.isnan(vals), 0.0, vals)
    med = float(np.median(vals))
    ra, rb = (0, e1 - s1) if rows is None else (max(0, rows[0] - halo), min(e1 - s1, rows[1] + halo))
    r, c = b1[sel] - s1, b2[sel] - s2
    keep = (r >= ra) & (r < rb)
    dense = np.zeros((rb - ra, e2 - s2))
    dense[r[keep] - ra, c[keep]] = vals[keep] / med
    miss_r, miss_c = ~np.isfinite(w[s1 + ra:s1 + rb]), ~np.isfinite(w[s2:e2])
    mtol, ztol = cfg["max_perc_undetected"] / 100, cfg["max_perc_zero"] / 100
    pred = orc.framed_missing_predicate(dense.shape, kernel.shape, miss_r, miss_c, False, None)
    corr, _ = orc.normxcorr2_oracle(dense, kernel, full=True, missing=pred, missing_tol=mtol)
    tab, wins = foci_oracle.detect_table(dense, corr, miss_r, miss_c, kernel.shape, cfg["pearson"], ztol, mtol, inter=True,
                                         return_windows=True)
    tab = np.asarray(tab, dtype=np.float64).reshape(-1, 3).copy()
    tab[:, 0] += ra
    return tab, np.asarray(wins).reshape(-1, *kernel.shape), med


def test_yeast_trans_blocks_against_the_oracle(golden):
    """Every trans block of the yeast map through detect_inter_block (float32 candidates from the list kernel: pearson 0.3),
    whole and cut into strips, against foci_oracle.detect_table on the host-built block: coordinates and order exact, scores
    within 1e-9, windows within 1e-9."""
    cool = golden("yeast_cool")
    cfg = copy.deepcopy(ck.loops)
    cfg["pearson"], cfg["max_perc_zero"] = 0.3, 100.0
    dcool = pipeline.DeviceCool(cool)
    budget = _cut_budget(dcool, 17)
    n_rec = n_blocks = 0
    for ca in range(dcool.n_chrom):
        for cb in range(ca + 1, dcool.n_chrom):
            want, wwin, med = _oracle_block(cool, dcool.offsets, ca, cb, LOOPS, cfg)
            assert dcool.inter_median(ca, cb) == med
            for bud in (1 << 34, budget):
                tab, win = pipeline.detect_inter_block(dcool, ca, cb, cfg, LOOPS, want_windows=True, inter_budget=bud)
                tab = np.zeros((0, 4)) if tab is None else tab
                assert np.array_equal(tab[:, :2], want[:, :2]), (ca, cb, bud)
                assert np.allclose(tab[:, 2], want[:, 2], rtol=0, atol=1e-9)
                if len(tab):
                    assert np.allclose(win, wwin, rtol=0, atol=1e-9, equal_nan=True)
            n_rec += len(want)
            n_blocks += 1
    assert n_rec > 0
    print(f"yeast: {n_blocks} trans blocks, {n_rec} records equal to the oracle, whole and in strips (budget {budget} B)")


def _detect_per_block(cool, cfg):
    """`detect(inter=True)` as it was before the strip route: every trans block staged whole (stage_inter(resident=True)) and
    scanned by detect_blocks -- the yardstick."""
    dcool = pipeline.DeviceCool(cool)
    off = dcool.offsets
    pairs = pipeline.sub_matrices(dcool, True)
    max_dist = max(cfg["max_dist"] // dcool.binsize, 1)
    largest = max(np.shape(k)[0] for k in cfg["kernels"])
    intra = dict(zip([a for a, b in pairs if a == b], dcool.stage_blocks([a for a, b in pairs if a == b], max_dist, largest)))
    blocks = [intra[a] if a == b else dcool.stage_inter(a, b, resident=True) for a, b in pairs]
    all_coords, all_windows = [], []
    for kernel_id, kernel in enumerate(cfg["kernels"]):
        for it in range(cfg["max_iterations"]):
            tables, windows = [], []
            results = pipeline.detect_blocks(dcool, blocks, cfg, kernel, raw=True, want_windows=True)
            for (ca, cb), (tab, win) in zip(pairs, results):
                if tab is None or len(tab) == 0:
                    continue
                tab[:, 0] += int(off[ca])
                tab[:, 1] += int(off[cb])
                tables.append(tab)
                windows.append(win)
            if not tables:
                break
            rec = np.concatenate(tables)
            all_coords.append({"bin1": rec[:, 0].astype(np.int64), "bin2": rec[:, 1].astype(np.int64), "score": rec[:, 2],
                               "pvalue": rec[:, 3], "kernel_id": np.full(len(rec), kernel_id), "iteration": np.full(len(rec), it)})
            kw = np.concatenate(windows)
            all_windows.append(kw)
            kernel = cid.pileup_patterns(kw)
    coords = {k: np.concatenate([c[k] for c in all_coords]) for k in all_coords[0]}
    return pipeline.postprocess(coords, cfg, dcool.binsize, off, dcool.names, dcool.bin_start, dcool.bin_end,
                                windows=np.concatenate(all_windows))


def _same(a, b):
    (ta, wa), (tb, wb) = a, b
    assert len(ta) == len(tb)
    for col in ("bin1", "bin2", "kernel_id", "iteration"):
        assert np.array_equal(ta[col].to_numpy(), tb[col].to_numpy()), col
    assert np.allclose(ta.score.to_numpy(dtype=float), tb.score.to_numpy(dtype=float), rtol=0, atol=1e-9)
    assert np.allclose(ta.pvalue.to_numpy(dtype=float), tb.pvalue.to_numpy(dtype=float), rtol=1e-9, atol=0, equal_nan=True)
    assert np.allclose(wa, wb, rtol=0, atol=1e-9, equal_nan=True)


def _cut_budget(dcool, reach, own=8):
    """The smallest budget that holds `own` rows and their halo of every trans block of the map: the widest blocks are cut into
    strips of `own` rows, the narrowest into fewer, wider ones."""
    sizes = np.diff(dcool.offsets)
    halo = (reach - 1) // 2
    return max((own + 2 * halo) * ((int(n_c) + 15) // 16 * 16) * 8 for n_c in sizes[1:])


@pytest.mark.parametrize("iterations,pearson", [(1, 0.3), (1, 0.1), (2, 0.3), (2, 0.1)])
def test_yeast_detect_inter_strips_equal_the_per_block_route(golden, iterations, pearson):
    """pearson 0.3: float32 candidates (the list kernel); 0.1: float64 maps.  Two iterations: every strip staged again, the
    second template is the pileup of the windows of every block.  Same table, same order, windows within 1e-9."""
    cool = golden("yeast_cool")
    cfg = copy.deepcopy(ck.loops)
    cfg["max_iterations"] = iterations
    cfg["pearson"], cfg["max_perc_zero"] = pearson, 100.0      # (sparse trans windows: keep the ones with zeros)
    want = _detect_per_block(cool, cfg)
    dcool = pipeline.DeviceCool(cool)
    whole = pipeline.detect(dcool, cfg, inter=True, return_windows=True, inter_budget=1 << 34)
    _same(whole, want)
    inter_rows = whole[0][whole[0].chrom1 != whole[0].chrom2]
    assert len(inter_rows) > 0
    reach = pipeline._strip_reach(cfg["kernels"])
    budget = _cut_budget(dcool, reach)
    dcool = pipeline.DeviceCool(cool)                   # (a fresh pool: its high-water is this run's)
    cut = pipeline.detect(dcool, cfg, inter=True, return_windows=True, inter_budget=budget)
    assert 0 < dcool.inter_high_water <= budget
    _same(cut, want)
    # foci whose best pixel is on the row next to a cut: their windows (and, for foci of more than one row, their pixels)
    # straddle it
    sizes = np.diff(dcool.offsets)
    on_cut = 0
    halo = (reach - 1) // 2
    for _, r in inter_rows.iterrows():
        ca, cb = int(np.searchsorted(dcool.offsets, r.bin1, "right") - 1), int(np.searchsorted(dcool.offsets, r.bin2, "right") - 1)
        strips = pipeline.plan_inter_strips(sizes[ca], sizes[cb], budget, halo)
        local = int(r.bin1 - dcool.offsets[ca])
        on_cut += any(local in (a - 1, a) for a, _ in strips[1:])
    assert on_cut > 0, "no detected focus next to a cut"
    n_strips = [len(pipeline.plan_inter_strips(sizes[a], sizes[b], budget, halo)) for a in range(len(sizes)) for b in range(a + 1, len(sizes))]
    assert np.mean(np.array(n_strips) >= 3) > 0.5
    print(f"detect --inter, {iterations} iteration(s), pearson {pearson}: {len(whole[0])} patterns, {len(inter_rows)} trans, "
          f"{on_cut} next to a cut, budget {budget} B, pool high-water {dcool.inter_high_water} B")


def test_yeast_quantify_inter_strips_equal_the_whole_blocks(golden):
    cool = golden("yeast_cool")
    cfg = copy.deepcopy(ck.loops)
    cfg["pearson"], cfg["max_perc_zero"] = 0.1, 100.0
    dcool = pipeline.DeviceCool(cool)
    table = pipeline.detect(dcool, cfg, inter=True, inter_budget=1 << 34)
    rng = np.random.default_rng(4)
    pos = table[["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].copy()
    names, sizes = dcool.names, np.diff(dcool.offsets)
    extra = []
    for _ in range(300):
        ca, cb = np.sort(rng.choice(len(names), 2, replace=False))
        s1, s2 = int(rng.integers(0, sizes[ca])) * dcool.binsize, int(rng.integers(0, sizes[cb])) * dcool.binsize
        extra.append((names[ca], s1, s1 + dcool.binsize, names[cb], s2, s2 + dcool.binsize))
    pos = pd.concat([pos, pd.DataFrame(extra, columns=pos.columns)], ignore_index=True)
    want_t, want_w = pipeline.quantify(dcool, pos, cfg, inter=True, inter_budget=1 << 34)
    budget = _cut_budget(dcool, pipeline._strip_reach(cfg["kernels"]))
    dcool = pipeline.DeviceCool(cool)
    got_t, got_w = pipeline.quantify(dcool, pos, cfg, inter=True, inter_budget=budget)
    assert 0 < dcool.inter_high_water <= budget
    pd.testing.assert_frame_equal(got_t, want_t)
    # (the windows of a trans position differ by up to 4e-15 between two runs of the SAME budget on fresh DeviceCools -- measured
    # on an MI355X, not caused by the strips: DESIGN.md)
    assert np.array_equal(np.isnan(got_w), np.isnan(want_w))
    assert np.allclose(got_w, want_w, rtol=0, atol=1e-12, equal_nan=True)
    # against the resident blocks of the batched path (cs_quantify_blocks on stage_inter_many): the route of the parent
    dcool2 = pipeline.DeviceCool(cool)
    shard_free = _quantify_resident(dcool2, pos, cfg)
    assert np.allclose(got_t.score.to_numpy(dtype=float), shard_free.score.to_numpy(dtype=float), rtol=0, atol=1e-9, equal_nan=True)


def _quantify_resident(dcool, pos, cfg):
    """quantify with every sub-matrix resident: one shard that holds everything (the parallel path keeps the resident route)."""
    class One:
        def select(self, todo, dcool, max_dist):
            return todo

        def merge(self, score_out, pval_out, win_out, sels):
            return score_out, pval_out, win_out
    t, _ = pipeline.quantify(dcool, pos, cfg, inter=True, shard=One())
    return t


def test_scale_trans_genome_in_strips():
    """24 chromosomes in hg38 proportions, ~310 000 bins (~360 GB of dense float64 trans area: more than an MI355X holds), a
    200-diagonal intra band and 2e7 sparse trans contacts with 40 planted trans patterns: detect --inter in strips within a
    2 GiB budget (the largest blocks in 3 strips)."""
    t0 = time.perf_counter()
    cool, planted = make_trans_cool(total_bins=310_000, n_chroms=24, intra_diags=200, n_trans=20_000_000, n_planted=40,
                                    template=LOOPS, binsize=10_000, seed=5)
    t_make = time.perf_counter() - t0
    dcool = pipeline.DeviceCool(cool)
    n = dcool.n_bins
    sizes = np.diff(dcool.offsets)
    area = (float(sizes.sum()) ** 2 - float((sizes.astype(np.float64) ** 2).sum())) / 2
    cfg = copy.deepcopy(ck.loops)
    cfg["max_perc_zero"] = 100.0            # (a planted pattern on an empty background: windows with zeros are kept)
    budget = 2 << 30
    stats = []
    orig = pipeline.detect_inter_block

    def spy(*a, **k):
        st = {}
        k["stats"] = st
        out = orig(*a, **k)
        stats.append(st)
        return out
    pipeline.detect_inter_block = spy
    try:
        t1 = time.perf_counter()
        table = pipeline.detect(dcool, cfg, inter=True, inter_budget=budget)
        wall = time.perf_counter() - t1
    finally:
        pipeline.detect_inter_block = orig
    assert dcool.inter_high_water <= budget
    trans = table[table.chrom1 != table.chrom2]
    found = set(zip(trans.bin1.astype(int), trans.bin2.astype(int)))
    hit = sum(any((abs(i - a) <= 1 and abs(j - b) <= 1) for a, b in found) for i, j in planted)
    strips = [s["strips"] for s in stats if s]
    tiles = sum(s["tiles"] for s in stats if s)
    listed = sum(s["tiles_listed"] for s in stats if s)
    print(f"scale: {n} bins, trans area {area:.3g} pixels ({area * 8 / 1e9:.0f} GB dense float64), {dcool.nnz} pixels "
          f"(generated in {t_make:.1f} s); detect --inter {wall:.1f} s, {len(trans)} trans patterns, {hit}/{len(planted)} planted found; "
          f"strips per block max {max(strips)} mean {np.mean(strips):.2f}, tiles skipped {1 - listed / max(tiles, 1):.4f}; "
          f"pool high-water {dcool.inter_high_water} B of {budget}")
    assert n > 300_000 and area * 8 > 3.5e11
    assert hit >= 0.9 * len(planted)
    assert max(strips) >= 2
    # oracle crops: the rows around three planted patterns of different blocks (plus the halo), built on the host and scaled by
    # the WHOLE block's median; every record of the block in the crop's inner rows equals the oracle's
    off = dcool.offsets
    chrom_of = np.repeat(np.arange(dcool.n_chrom), np.diff(off))
    seen, n_cmp = set(), 0
    for i, j in planted:
        ca, cb = int(chrom_of[i]), int(chrom_of[j])
        if (ca, cb) in seen or len(seen) == 3:
            continue
        seen.add((ca, cb))
        r = i - int(off[ca])
        lo, hi = max(0, r - 40), min(dcool.chrom_size(ca), r + 40)
        want, wwin, med = _oracle_block(cool, off, ca, cb, LOOPS, cfg, rows=(lo, hi), halo=8)
        assert dcool.inter_median(ca, cb) == med
        tab, win = pipeline.detect_inter_block(dcool, ca, cb, cfg, LOOPS, want_windows=True, inter_budget=budget)
        inner_lo, inner_hi = lo + 8 * (lo > 0), hi - 8 * (hi < dcool.chrom_size(ca))
        g = (tab[:, 0] >= inner_lo) & (tab[:, 0] < inner_hi)
        o = (want[:, 0] >= inner_lo) & (want[:, 0] < inner_hi)
        assert np.array_equal(tab[g, :2], want[o, :2]), (ca, cb)
        assert np.allclose(tab[g, 2], want[o, 2], rtol=0, atol=1e-9)
        assert np.allclose(win[g], wwin[o], rtol=0, atol=1e-9, equal_nan=True)
        n_cmp += int(g.sum())
    assert len(seen) == 3 and n_cmp >= 3
    print(f"scale oracle crops: {n_cmp} records in 3 blocks equal to the oracle")
