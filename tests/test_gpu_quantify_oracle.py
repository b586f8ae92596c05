"""`quantify` on the device against an independent CPU restatement (tests/quantify_oracle_util.py: the pinned oracles of
oracle/ -- block preparation, coefficients, the quantify rules of foci_oracle.quantify_table(_band), cmd_quantify's selection),
never against another device route.  Positions are built class by class (corners and edges around the strict window bounds,
missing-bin clusters, the diagonal and below it, max_dist - 1 .. + 1 and beyond, empty and nearly-too-empty regions, runs of
neighbours, duplicates, wide intervals, unknown chromosomes) and every class is asserted non-empty.

Asserted per case: the rows and their order, the NaN pattern of score / p-value / q-value, scores <= 1e-9, p-values to 1e-6
relative, and -- from the raw device records and windows -- inside / n_zero / n_missing exactly and the windows (NaN pattern
exact, values <= 1e-12).  A position whose oracle cond is below parity_util.COND_EPS, or one of whose oracle sums lies within
1e-9 relative of a zeroing threshold, is held to tol * COND_EPS / cond instead; such positions are at most 1 % of the finite
scores of a case and their count is printed.

A coefficient that is 0 by rule -- fewer present pixels than the cut, or a two-valued template (borders, stripes) whose
present entries are all equal -- is no exclusion: the oracle reports it well defined and it is held to 1e-9 like any other.
The returned windows (selection order: ascending score, NaN last) are compared row by row with the oracle's windows of the
picked template, groups of equal scores as multisets."""
import copy
import time

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
import quantify_oracle_util as qo
from chromosight_amd import engine, pipeline
from parity_util import COND_EPS
from tools.synthetic_genome import make_cool
from tools.synthetic_inter import make_trans_cool

pytestmark = pytest.mark.gpu

BIN = 2000
SIZES = [12, 19, 36, 400, 900, 3000]
LOOPS = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
_genomes = {}


def _with_clusters(cool, rng):
    """Missing-bin clusters at both ends and inside every chromosome of 36 bins and more; an emptied square and a thinned one
    (about a tenth of its pixels removed: zero shares on either side of max_perc_zero = 10) in the longer ones."""
    off = cool["chrom_offset"]
    w = cool["weight"]
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    drop = np.zeros(b1.size, dtype=bool)
    marks = {}
    for ci in range(len(off) - 1):
        s, n = int(off[ci]), int(off[ci + 1] - off[ci])
        if n < 36:
            continue
        w[s:s + 2] = np.nan
        w[s + n - 3:s + n] = np.nan
        inner = [n // 2] if n < 400 else [n // 3, n // 2, 2 * n // 3]
        for k, m in enumerate(inner):
            w[s + m:s + m + (3, 9, 6)[k % 3]] = np.nan
        marks[ci] = dict(clusters=[0, n - 3] + inner)
        if n >= 400:
            e0, t0 = n // 6, n // 6 + 80
            marks[ci].update(empty=(e0, e0 + 40), thin=(t0, t0 + 40))
            r, c = b1 - s, b2 - s
            drop |= (r >= e0 - 12) & (r < e0 + 12) & (c >= e0 + 28) & (c < e0 + 52)
            thin = (r >= t0 - 20) & (r < t0 + 20) & (c >= t0 + 20) & (c < t0 + 60)
            drop |= thin & (rng.random(b1.size) < 0.07)
    for k in ("bin1_id", "bin2_id", "count"):
        cool[k] = cool[k][~drop]
    return marks


def genome(md, seed=41, sizes=SIZES):
    key = (md, seed, tuple(sizes))
    if key not in _genomes:
        cool, planted = make_cool(sum(sizes), md, BIN, seed=seed, template=LOOPS, chrom_sizes=sizes, largest_kernel=40)
        marks = _with_clusters(cool, np.random.default_rng(seed))
        _genomes[key] = (cool, planted, marks)
    return _genomes[key]


def build_positions(cool, planted, marks, md, k, seed=3, n_uniform=5000, long_run=300):
    """DataFrame of positions and {class: row indices}.  k: template side (kh = (k - 1) // 2)."""
    rng = np.random.default_rng(seed)
    off = np.asarray(cool["chrom_offset"])
    names = [str(x) for x in cool["chrom_names"]]
    kh = (k - 1) // 2
    rows, cls = [], {}

    def add(name, ci, r, c, w1=1, w2=1):
        r, c = np.atleast_1d(r).astype(np.int64), np.atleast_1d(c).astype(np.int64)
        n = int(off[ci + 1] - off[ci])
        ok = (r >= 0) & (r < n) & (c >= 0) & (c < n)
        for a, b in zip(r[ok], c[ok]):
            cls.setdefault(name, []).append(len(rows))
            rows.append((names[ci], int(a) * BIN, int(a + w1) * BIN, names[ci], int(b) * BIN, int(b + w2) * BIN))
    chrom_of = np.searchsorted(off, np.array([p[0] for p in planted]), side="right") - 1 if planted else []
    for (g1, g2), ci in zip(planted, chrom_of):
        add("planted", ci, g1 - off[ci], g2 - off[ci])
    for ci in range(len(names)):
        n = int(off[ci + 1] - off[ci])
        if n <= 19:
            add("below_template_size", ci, [0, n // 2, n - 1, 3], [n // 2, n // 2, n - 1, 1])
            continue
        r = rng.integers(0, n, n_uniform if n >= 400 else 40)
        add("uniform_in_band", ci, r, r + rng.integers(0, md + 1, r.size))
        edge = np.concatenate([np.arange(0, kh + 2), np.arange(n - kh - 2, n)])
        near = np.unique(np.clip(np.concatenate([edge, edge[:kh + 2] + md // 2, edge[kh + 2:] - md // 2]), 0, n - 1))
        rr, cc = np.meshgrid(edge, near, indexing="ij")
        add("corners_edges", ci, rr.ravel(), cc.ravel())
        add("corners_edges", ci, cc.ravel(), rr.ravel())
        m = marks.get(ci, {})
        for cl in m.get("clusters", []):
            for dr in range(-kh - 2, kh + 12, 3):
                add("missing_clusters", ci, np.full(8, cl + dr), cl + dr + np.array([0, 1, 2, kh - 1, kh, kh + 3, 2 * kh + 2, md // 2]))
        d0 = np.arange(kh, n, max(n // 25, 1))
        add("main_diagonal", ci, d0, d0)
        for d in (1, 2, k - 1, k, k + 1, 3 * k):
            add("below_diag_within" if d <= k else "below_diag_beyond", ci, d0, d0 - d)
        for d, name in ((md - 1, "max_dist-1"), (md, "max_dist"), (md + 1, "max_dist+1"), (md + 40, "beyond_max_dist"), (n - 1 - kh - 3, "beyond_max_dist")):
            if d > md - 2 and d < n:
                add(name, ci, d0, d0 + d)
        if "empty" in m:
            e0, t0 = m["empty"][0], m["thin"][0]
            add("empty_region", ci, [e0, e0 + 1, e0 - 1], [e0 + 40, e0 + 40, e0 + 41])
            tr, tc = np.meshgrid(np.arange(t0 - 8, t0 + 9, 2), np.arange(t0 + 30, t0 + 50, 2), indexing="ij")
            add("thinned_region", ci, tr.ravel(), tc.ravel())
        if n >= 400:
            cl = m["clusters"][2]
            for length in (1, 2, 63, 64, 65, long_run):
                add(f"run_{length if length < long_run else 'long'}", ci, np.full(length, n // 5), n // 5 + 3 + np.arange(length))
            add("run_across_missing", ci, np.full(70, cl - 20), cl - 10 + np.arange(70))
            add("run_across_band_edge", ci, np.full(66, n // 4), n // 4 + md - 30 + np.arange(66))
            add("run_to_chrom_end", ci, np.full(65, n - 50), n - 65 + np.arange(65))
            add("duplicates", ci, [n // 5, n // 5, n // 5, 40], [n // 5 + 3, n // 5 + 3, n // 5 + 4, 60])
            add("wide_intervals", ci, [50, 51, n // 2, n - 6], [80, 90, n // 2 + 30, n - 4], w1=3, w2=5)
    cls["unknown_chromosome"] = [len(rows), len(rows) + 1]
    rows += [("chrZ", 10 * BIN, 11 * BIN, "chrZ", 20 * BIN, 21 * BIN), (names[-1], 10 * BIN, 11 * BIN, "nowhere", 20 * BIN, 21 * BIN)]
    n_last = int(off[-1] - off[-2])
    cls["past_chromosome_end"] = [len(rows), len(rows) + 1]
    rows += [(names[-1], 10 * BIN, 11 * BIN, names[-1], (n_last + 5) * BIN, (n_last + 6) * BIN),
             (names[-1], (n_last + 50) * BIN, (n_last + 51) * BIN, names[-1], (n_last + 70) * BIN, (n_last + 71) * BIN)]
    return pd.DataFrame(rows, columns=["chrom1", "start1", "end1", "chrom2", "start2", "end2"]), {k: np.array(v) for k, v in cls.items()}


class _Capture:
    """The raw records and windows of every native quantify call, keyed by (block name, row, column)."""

    def __init__(self, monkeypatch):
        self.rec, self.block = {}, [None]
        blocks_fn, pixels_fn, detect_block = engine.run_quantify_blocks, engine.run_quantify_pixels, pipeline.detect_block

        def run_blocks(dev, blocks, kspec, blk, rows, cols, **kw):
            rec, win = blocks_fn(dev, blocks, kspec, blk, rows, cols, **kw)
            self.keep([blocks[b].name for b in np.asarray(blk)], rows, cols, rec, win)
            return rec, win

        def run_pixels(dev, sig, shape, kspec, rows, cols, **kw):
            rec, win = pixels_fn(dev, sig, shape, kspec, rows, cols, **kw)
            if self.block[0] is not None:
                self.keep([self.block[0]] * len(rec), rows, cols, rec, win)
            return rec, win

        def one_block(dcool, block, *a, **kw):
            self.block[0] = block.name
            try:
                return detect_block(dcool, block, *a, **kw)
            finally:
                self.block[0] = None
        monkeypatch.setattr(engine, "run_quantify_blocks", run_blocks)
        monkeypatch.setattr(engine, "run_quantify_pixels", run_pixels)
        monkeypatch.setattr(pipeline, "detect_block", one_block)

    def keep(self, names, rows, cols, rec, win):
        for t, (nm, r, c) in enumerate(zip(names, np.asarray(rows), np.asarray(cols))):
            self.rec.setdefault((nm, int(r), int(c)), []).append(
                (int(rec["inside"][t]), int(rec["n_zero"][t]), int(rec["n_missing"][t]), None if win is None else win[t].copy(),
                 float(rec["n_obs"][t]), float(rec["pval"][t])))


def check_case(monkeypatch, what, cool, positions, classes, cfg, inter=False, max_dist_bp=None, env=(), **opts):
    for name, idx in classes.items():
        assert len(idx) > 0, (what, name)
    cfg = pipeline.with_win_size(cfg, opts.get("win_size"))
    t0 = time.time()
    res, want = qo.quantify_genome(cool, positions, dict(cfg, kernels=[np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]),
                                   inter=inter, max_dist_bp=max_dist_bp, smooth=bool(opts.get("smooth")), tsvd=opts.get("tsvd"))
    _assert_straddles(what, res[0], cfg, classes)
    t_oracle = time.time() - t0
    for e in env:
        monkeypatch.setenv(e, "1")
    cap = _Capture(monkeypatch)
    table, windows = pipeline.quantify(pipeline.DeviceCool(copy.deepcopy(cool)), positions, cfg, inter=inter, max_dist_bp=max_dist_bp, **opts)
    for e in env:
        monkeypatch.delenv(e)
    # ---- rows and order (the rows without a bin come last in both; among themselves they are compared as a set)
    assert len(table) == len(want), what
    has_bin = ~np.isnan(want.bin1.to_numpy(dtype=np.float64)) & ~np.isnan(want.bin2.to_numpy(dtype=np.float64))
    for col in ("chrom1", "start1", "end1", "chrom2", "start2", "end2"):
        assert (table[col].to_numpy()[has_bin] == want[col].to_numpy()[has_bin]).all(), (what, col)
    cols6 = ["chrom1", "start1", "end1", "chrom2", "start2", "end2"]
    assert sorted(map(tuple, table[cols6].to_numpy()[~has_bin].tolist())) == sorted(map(tuple, want[cols6].to_numpy()[~has_bin].tolist())), what
    for col in ("bin1", "bin2"):
        assert np.array_equal(table[col].to_numpy(dtype=np.float64), want[col].to_numpy(dtype=np.float64), equal_nan=True), (what, col)
    got_s, want_s = table["score"].to_numpy(dtype=np.float64), want["score"].to_numpy(dtype=np.float64)
    got_p, want_p = table["pvalue"].to_numpy(dtype=np.float64), want["pvalue"].to_numpy(dtype=np.float64)
    assert np.isnan(got_s[~has_bin]).all() and np.isnan(want_s[~has_bin]).all(), what
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s)), what
    assert np.array_equal(np.isnan(got_p), np.isnan(want_p)), what
    assert np.array_equal(np.isnan(table["qvalue"].to_numpy(dtype=np.float64)), want["qvalue_nan"].to_numpy()), what
    # ---- scores: 1e-9; the ill-conditioned and the threshold-straddling ones by parity_util's rule, at most 1 % of them
    src, kid = want.src.to_numpy(), want.kernel_id.to_numpy()
    cond = np.array([res[k]["cond"][s] for s, k in zip(src, kid)])
    near = np.array([bool(res[k]["near"][s]) for s, k in zip(src, kid)])
    fin = ~np.isnan(want_s)
    soft = fin & (near | (cond < COND_EPS))
    err = np.abs(got_s - want_s)
    worst = float(err[fin & ~soft].max()) if (fin & ~soft).any() else 0.0
    assert soft.sum() <= 0.01 * fin.sum(), (what, int(soft.sum()), int(fin.sum()))
    assert worst < 1e-9, (what, worst)
    if soft.any():            # (tol * COND_EPS / cond, never below the bound of an ordinary position)
        assert (err[soft] <= 1e-9 * np.maximum(1.0, COND_EPS / np.maximum(cond[soft], 1e-300))).all(), (what, float(err[soft].max()))
    assert np.allclose(got_p[fin], want_p[fin], rtol=1e-6, atol=1e-300), what
    # ---- raw records and windows of every scanned position, every template
    n_raw, worst_w = 0, 0.0
    kspecific, kk = len(res) == 1, int(np.prod(np.shape(cfg["kernels"][0])))
    names = [str(x) for x in cool["chrom_names"]]
    for ki, d in enumerate(res):
        for t in np.flatnonzero(d["scanned"]):
            ca, cb = int(d["chrom1"][t]), int(d["chrom2"][t])
            key = (names[ca] if ca == cb else f"{names[ca]}-{names[cb]}", int(d["bin1"][t]), int(d["bin2"][t]))
            assert key in cap.rec, (what, key)
            for inside, n_zero, n_missing, win, n_obs, pval in cap.rec[key]:
                assert inside == int(d["inside"][t]), (what, key, "inside")
                if inside:
                    assert (n_zero, n_missing) == (int(d["n_zero"][t]), int(d["n_missing"][t])), (what, key, n_zero, n_missing)
                if d["valid"][t] and win is not None:
                    assert np.array_equal(np.isnan(win), np.isnan(d["windows"][t])), (what, key, "window NaN pattern")
                    worst_w = max(worst_w, float(np.nanmax(np.abs(win - d["windows"][t]), initial=0.0)))
                if kspecific and not np.isnan(d["pvalue"][t]):
                    # (cs_focus.n_obs / pval, which cs_accept_records trusts: 0 stands for "every pixel present"; records are
                    # keyed by position, so these two are checked where one template makes the calls)
                    if d["pvalue"][t] != 1.0:
                        assert (n_obs or float(kk)) == d["n_obs"][t], (what, key, n_obs, d["n_obs"][t])
                    assert np.isclose(pval, d["pvalue"][t], rtol=1e-6, atol=1e-300), (what, key, pval, d["pvalue"][t])
                n_raw += 1
    assert worst_w < 1e-12, (what, worst_w)
    assert n_raw >= int(sum(d["scanned"].sum() for d in res)), what
    # ---- the returned windows: selection order = ascending score, NaN scores last (cli/chromosight.py:434-441)
    exp_w = np.stack([res[k]["windows"][s_] for s_, k in zip(src, kid)]) if len(src) else windows
    order = np.argsort(np.where(fin, got_s, np.inf), kind="stable")
    n_fin = int(fin.sum())
    assert np.isnan(windows[n_fin:]).all() and np.isnan(exp_w[~fin]).all(), what
    got_w, exp_w, s_sorted = windows[:n_fin], exp_w[order[:n_fin]], got_s[order[:n_fin]]

    def canon(w, group):                                # rows of equal score: the same multiset of windows
        key = np.lexsort((np.round(np.nansum(w * np.arange(1, w[0].size + 1).reshape(w[0].shape), axis=(1, 2)), 6),
                          np.round(np.nansum(w, axis=(1, 2)), 6), np.isnan(w).sum(axis=(1, 2)), group))
        return w[key]
    group = np.concatenate([[0], np.cumsum(s_sorted[1:] != s_sorted[:-1])]) if n_fin else np.zeros(0, dtype=int)
    if n_fin:
        a, b = canon(got_w, group), canon(exp_w, group)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "returned windows: NaN placement")
        assert float(np.nanmax(np.abs(a - b), initial=0.0)) < 1e-12, (what, "returned windows")
    sizes = ", ".join(f"{k} {len(v)}" for k, v in classes.items())
    print(f"[quantify-oracle] {what}: {len(positions)} positions -> {len(table)} rows, {int(fin.sum())} finite scores, "
          f"{int(soft.sum())} excluded (cond < {COND_EPS:g} or near a threshold), worst |score err| {worst:.2e}, worst |window err| "
          f"{worst_w:.2e}, {n_raw} raw records checked, oracle {t_oracle:.1f} s; classes: {sizes}")
    # chromosomes not larger than the template (12 bins always, 19 from 19 x 19 on): all NaN
    n_bins = np.diff(np.asarray(cool["chrom_offset"]))
    tiny = [nm for nm, n in zip(names, n_bins) if n <= max(np.shape(cfg["kernels"][0]))]
    if tiny:
        assert np.isnan(got_s[np.isin(table.chrom1.to_numpy(), tiny)]).all(), what
    return want


def _assert_straddles(what, d, cfg, classes):
    """The classes the issue defines by their outcome, from the oracle's own statistics: max_perc_undetected met from both
    sides next to the missing clusters, a zero share just under and just over max_perc_zero, an empty window."""
    if "missing_clusters" not in classes:
        return
    tot = int(np.prod(np.shape(cfg["kernels"][0])))
    mtol, ztol = cfg["max_perc_undetected"] / 100, cfg["max_perc_zero"] / 100
    ins = d["inside"].astype(bool)
    with np.errstate(all="ignore"):
        pu, pz = d["n_missing"] / tot, d["n_zero"] / (tot - d["n_missing"])
    mc = np.zeros(ins.size, dtype=bool)
    mc[classes["missing_clusters"]] = True
    assert (mc & ins & (pu < mtol) & (pu >= mtol - 0.15)).any() and (mc & ins & (pu >= mtol) & (pu < mtol + 0.15)).any(), (what, "undetected")
    assert (ins & (pu < mtol) & (pz < ztol) & (pz >= ztol - 0.05)).any() and (ins & (pu < mtol) & (pz >= ztol) & (pz < ztol + 0.05)).any(), (what, "zero share")
    assert (ins & (pz == 1.0)).any(), (what, "empty window")


def _cfg(name):
    return copy.deepcopy(getattr(ck, name))


def _nonsquare_cfg(golden):
    cfg = _cfg("loops")
    cfg["kernels"] = [np.asarray(golden("nonsquare")["d2_59_kernel"], dtype=np.float64)]
    return cfg


INTRA = [("loops 17x17", "loops", {}), ("borders x3, best of templates", "borders", {}), ("hairpins 15x15", "hairpins", {}),
         ("loops_small 7x7", "loops_small", {}), ("stripes_left 31x31", "stripes_left", {}),
         ("loops 17x17 smooth", "loops", dict(smooth=True)), ("loops 17x17 tsvd", "loops", dict(tsvd=0.999)),
         ("--win-size 9", "loops", dict(win_size=9)), ("--win-size 23", "loops", dict(win_size=23)),
         ("--win-size 33", "loops", dict(win_size=33))]


@pytest.mark.parametrize("what,pattern,opts", INTRA, ids=[c[0] for c in INTRA])
def test_intra_quantify_vs_oracle(monkeypatch, what, pattern, opts):
    """pipeline.quantify end to end (cs_quantify_blocks) on chromosomes of 12 .. 3000 bins, max_dist pinned."""
    md = 120
    cool, planted, marks = genome(md)
    cfg = _cfg(pattern)
    k = opts.get("win_size") or np.shape(cfg["kernels"][0])[0]
    positions, classes = build_positions(cool, planted, marks, md, k)
    check_case(monkeypatch, what, cool, positions, classes, cfg, max_dist_bp=md * BIN, **opts)


@pytest.mark.parametrize("env", [(), ("CHROMOSIGHT_HIP_NO_RUN_RESCORE",), ("CHROMOSIGHT_HIP_NO_QUANTIFY_BATCH",)],
                         ids=["derived max_dist", "no run rescore", "cs_quantify_pixels"])
def test_loops_routes_vs_oracle(monkeypatch, env):
    """loops 17 x 17 with max_dist derived from the furthest position (the reference's rule), without the run-scoring kernel,
    and block by block (cs_quantify_pixels)."""
    md = 120
    cool, planted, marks = genome(md)
    positions, classes = build_positions(cool, planted, marks, md, 17)
    check_case(monkeypatch, f"loops 17x17 {env or 'derived max_dist'}", cool, positions, classes, _cfg("loops"),
               max_dist_bp=None if not env else md * BIN, env=env)


def test_every_position_located_qvalues_vs_oracle(monkeypatch):
    """Chromosomes larger than the template only, no position outside the genome: every p-value is finite, so the q-values
    are NaN exactly where the score is (elsewhere in this file one unlocated position makes them all NaN, as the reference does)."""
    md = 120
    cool, planted, marks = genome(md, sizes=[36, 400, 900])
    positions, classes = build_positions(cool, planted, marks, md, 17)
    drop = np.concatenate([classes.pop("unknown_chromosome"), classes.pop("past_chromosome_end")])
    keep = np.setdiff1d(np.arange(len(positions)), drop)
    remap = np.full(len(positions), -1)
    remap[keep] = np.arange(keep.size)
    classes = {k: remap[v] for k, v in classes.items()}
    positions = positions.iloc[keep].reset_index(drop=True)
    want = check_case(monkeypatch, "loops 17x17, every position located", cool, positions, classes, _cfg("loops"), max_dist_bp=md * BIN)
    assert not want["qvalue_nan"].all() and want["qvalue_nan"].any()


def test_nonsquare_template_per_block_path_vs_oracle(monkeypatch, golden):
    """A 5 x 9 template: the batch does not apply, every block takes the per-block path with the (kh, kw) shift mismatch."""
    md = 120
    cool, planted, marks = genome(md)
    positions, classes = build_positions(cool, planted, marks, md, 9)
    check_case(monkeypatch, "non-square 5x9, per-block path", cool, positions, classes, _nonsquare_cfg(golden), max_dist_bp=md * BIN)


def _trans_positions(cool, k, rng, n_uniform=150):
    off = np.asarray(cool["chrom_offset"])
    names = [str(x) for x in cool["chrom_names"]]
    kh = (k - 1) // 2
    rows, cls = [], {}
    for ca in range(len(names)):
        for cb in range(ca + 1, len(names)):
            nr, nc = int(off[ca + 1] - off[ca]), int(off[cb + 1] - off[cb])

            def add(name, r, c):
                for a, b in zip(np.atleast_1d(r), np.atleast_1d(c)):
                    if 0 <= a < nr and 0 <= b < nc:
                        cls.setdefault(name, []).append(len(rows))
                        rows.append((names[ca], int(a) * BIN, int(a + 1) * BIN, names[cb], int(b) * BIN, int(b + 1) * BIN))
            add("uniform", rng.integers(0, nr, n_uniform), rng.integers(0, nc, n_uniform))
            er = np.concatenate([np.arange(0, kh + 2, 3), np.arange(nr - kh - 2, nr, 3), [0, kh, kh + 1, nr - kh - 2, nr - kh - 1, nr - 2, nr - 1]])
            ec = np.concatenate([np.arange(0, kh + 2, 3), np.arange(nc - kh - 2, nc, 3), [0, kh, kh + 1, nc - kh - 2, nc - kh - 1, nc - 2, nc - 1]])
            rr, cc = np.meshgrid(er, ec, indexing="ij")
            add("corners_edges", rr.ravel(), cc.ravel())
            add("run_65", np.full(65, nr // 2), nc // 3 + np.arange(65))
            add("run_to_edge", np.full(70, nr // 3), nc - 70 + np.arange(70))
            add("duplicates", [nr // 2, nr // 2], [nc // 3, nc // 3])
    return pd.DataFrame(rows, columns=["chrom1", "start1", "end1", "chrom2", "start2", "end2"]), {k: np.array(v) for k, v in cls.items()}


def test_centromeres_trans_block_through_strips_vs_oracle(monkeypatch):
    """centromeres 81 x 81 on modest trans blocks through quantify_inter_block, inter_budget small enough for several row groups."""
    tmpl = np.asarray(ck.centromeres["kernels"][0], dtype=np.float64)
    sizes = [300, 260, 90]
    cool, _ = make_trans_cool(chrom_sizes=sizes, intra_diags=40, n_trans=60_000, n_planted=6, template=tmpl, binsize=BIN, seed=9)
    w = cool["weight"]
    for s in (0, 140, 296, 300, 430, 555):
        w[s:s + 4] = np.nan
    positions, classes = _trans_positions(cool, 81, np.random.default_rng(4))
    ld = pipeline._inter_ld(260)
    budget = ld * 8 * 130                                 # 130 rows of the widest block (halo 40 each side): several groups of its 300 rows
    groups = []
    real = pipeline._row_groups
    monkeypatch.setattr(pipeline, "_row_groups", lambda *a: groups.append(real(*a)) or groups[-1])
    check_case(monkeypatch, "centromeres 81x81 --inter in strips", cool, positions, classes, _cfg("centromeres"), inter=True,
               max_dist_bp=40 * BIN, inter_budget=budget)
    assert max(len(g) for g in groups) >= 3, groups


def test_c4_genome_200k_quantify_vs_oracle(monkeypatch):
    """The 200 000-bin, 23-block genome of test_c4_genome_200k_vs_oracle_pipeline (same generator call, the oracle bands built
    the same way) with more than 10^5 positions of every class, long runs included: grid sizing and the batched chain's block
    table at size."""
    md = 1000
    cool, planted = make_cool(200_000, md, BIN, seed=2, template=LOOPS)
    marks = _with_clusters(cool, np.random.default_rng(2))
    positions, classes = build_positions(cool, planted, marks, md, 17, n_uniform=2400, long_run=700)
    assert len(positions) >= 100_000, len(positions)
    t0 = time.time()
    check_case(monkeypatch, "C4 genome 200k, loops 17x17", cool, positions, classes, _cfg("loops"), max_dist_bp=md * BIN)
    print(f"[quantify-oracle] C4 genome case: {time.time() - t0:.1f} s")
