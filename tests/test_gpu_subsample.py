"""--subsample on the device (cs_subsample, chromosight_amd/subsample.py; DeviceCool.subsampled(sampler="device")): exact pool
totals, identity and empty cases, bitwise determinism, the distribution of the draws against the exact pmf and numpy's
sampler, and detect / quantify end to end against an upload of the same subsampled table."""
import copy

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import pipeline
from chromosight_amd import subsample as css
from chromosight_amd._lib import Device
from tests.subsample_util import block_pmf, chi2_against_pmf, two_sample_chi2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def yeast_dcool(golden):
    return pipeline.DeviceCool(golden("yeast_cool"))


def _host_table(dcool):
    h = dcool.host
    return np.asarray(h["bin1_id"], dtype=np.int64), np.asarray(h["bin2_id"], dtype=np.int64), np.asarray(h["count"])


def _chroms(dcool, b1, b2):
    chrom_of = np.repeat(np.arange(dcool.n_chrom), np.diff(dcool.offsets))
    return chrom_of[b1], chrom_of[b2]


def _csr_host(res):
    n = res["nnz"]
    indptr = res["indptr"].download()
    return indptr, res["indices"].download()[:n].copy(), res["data"].download().view(np.uint8)[:n * np.dtype(res["val_dtype"]).itemsize]


def _new_counts(dcool, res):
    """The drawn table's counts on the parent's pixels (0 where a pixel was dropped)."""
    b1, b2, _ = _host_table(dcool)
    n = res["nnz"]
    indptr = res["indptr"].download()
    nb1 = np.repeat(np.arange(dcool.n_bins, dtype=np.int64), np.diff(indptr))
    nb2 = res["indices"].download()[:n].astype(np.int64)
    data = res["data"].download().view(res["val_dtype"])[:n]
    key = b1 * dcool.n_bins + b2
    at = np.searchsorted(key, nb1 * dcool.n_bins + nb2)
    assert np.all(key[at] == nb1 * dcool.n_bins + nb2), "a drawn pixel is not a pixel of the parent"
    new = np.zeros(b1.size, dtype=np.int64)
    new[at] = data.astype(np.int64)
    assert np.all(data > 0) and np.all(data == np.rint(data))
    return new


@pytest.mark.parametrize("inter", [False, True])
@pytest.mark.parametrize("sample", [0.1, 0.5, 0.9])
def test_pool_totals_are_exact(yeast_dcool, inter, sample):
    dc = yeast_dcool
    assert dc.nnz > 2_000_000 and dc.n_chrom == 17
    res = css.subsample_csr(dc, sample, seed=11, inter=inter, drawn=True)
    b1, b2, cnt = _host_table(dc)
    cnt = cnt.astype(np.int64)
    c1, c2 = _chroms(dc, b1, b2)
    new, drawn = _new_counts(dc, res), res["drawn"]
    mirrored = (c1 == c2) & (b1 != b2)
    blocks = res["blocks"]
    assert len(blocks) == (17 * 18 // 2 if inter else 17)
    want_pairs = sorted((a, b) for a, b in pipeline.sub_matrices(dc, inter))
    assert [(int(b["chrom1"]), int(b["chrom2"])) for b in blocks] == want_pairs
    sampled = np.zeros(b1.size, dtype=bool)
    for blk in blocks:
        ca, cb = int(blk["chrom1"]), int(blk["chrom2"])
        sel = (c1 == ca) & (c2 == cb)
        sampled |= sel
        total = int(cnt[sel].sum() + cnt[sel & mirrored].sum())
        assert int(blk["total"]) == total
        assert int(blk["keep"]) == int(sample * total)
        assert int(drawn[sel].sum()) == int(blk["keep"])
    assert np.all((new >= 0) & (new <= cnt))
    assert np.all(drawn[~sampled] == 0) and np.all(new[~sampled] == 0)
    assert np.all(new[~mirrored] == drawn[~mirrored])
    assert np.all((new[mirrored] <= drawn[mirrored]) & (drawn[mirrored] - new[mirrored] <= cnt[mirrored]))
    if inter:
        # a trans block stores its whole draw: its total is the numpy path's, exactly
        ref = dc.subsampled(sample, seed=11, inter=True)
        rb1, rb2, rcnt = _host_table(ref)
        r1, r2 = _chroms(ref, rb1, rb2)
        for blk in blocks:
            ca, cb = int(blk["chrom1"]), int(blk["chrom2"])
            if ca != cb:
                assert int(new[(c1 == ca) & (c2 == cb)].sum()) == int(rcnt[(r1 == ca) & (r2 == cb)].sum()) == int(blk["keep"])


def test_sample_one_returns_the_parent_and_zero_an_empty_table(yeast_dcool):
    dc = yeast_dcool
    b1, b2, cnt = _host_table(dc)
    sub = dc.subsampled(1.0, seed=2, inter=True, sampler="device")
    keep = cnt.astype(np.int64) > 0
    assert sub.nnz == int(keep.sum())
    assert np.array_equal(sub.host["bin1_id"], b1[keep]) and np.array_equal(sub.host["bin2_id"], b2[keep])
    assert np.array_equal(sub.host["count"], cnt.astype(np.int64)[keep])
    up = pipeline.DeviceCool(sub.host)
    assert sub.val_dtype is up.val_dtype and sub.counts_ok == up.counts_ok and sub.upper == up.upper
    assert np.array_equal(sub.indptr.download(), up.indptr.download())
    assert np.array_equal(sub.indices.download()[:sub.nnz], up.indices.download())
    assert np.array_equal(sub.data.download().view(up.val_dtype)[:sub.nnz], up.data.download())
    assert np.array_equal(sub.host["weight"], dc.host["weight"], equal_nan=True)
    empty = dc.subsampled(0.0, seed=2, inter=True, sampler="device")
    assert empty.nnz == 0 and empty.host["count"].size == 0 and np.all(empty.indptr.download() == 0)


def test_fractional_counts_truncate_like_the_host_path(golden):
    cool = dict(golden("yeast_cool"))
    cool["count"] = np.asarray(cool["count"], dtype=np.float64) + 0.75
    dc = pipeline.DeviceCool(cool)
    assert dc.val_dtype is np.float64
    got = dc.subsampled(1.0, seed=0, inter=True, sampler="device")
    want = dc.subsampled(1.0, seed=0, inter=True)
    for k in ("bin1_id", "bin2_id", "count"):
        assert np.array_equal(np.asarray(got.host[k], dtype=np.int64), np.asarray(want.host[k], dtype=np.int64)), k
    assert got.val_dtype is pipeline.DeviceCool(got.host).val_dtype is np.float32


def test_invalid_counts_and_samples_raise(golden, yeast_dcool):
    cool = dict(golden("yeast_cool"))
    bad = np.asarray(cool["count"], dtype=np.float64).copy()
    bad[1234] = -3.0
    with pytest.raises(ValueError):
        pipeline.DeviceCool(dict(cool, count=bad)).subsampled(0.5, sampler="device")
    bad[1234] = np.nan
    with pytest.raises(ValueError):
        pipeline.DeviceCool(dict(cool, count=bad)).subsampled(0.5, sampler="device")
    with pytest.raises(ValueError, match="Subsample must be strictly positive."):
        yeast_dcool.subsampled(-0.1, sampler="device")
    with pytest.raises(ValueError, match="Subsample cannot be above 1"):
        yeast_dcool.subsampled(1.5, sampler="device")
    with pytest.raises(ValueError, match="sampler"):
        yeast_dcool.subsampled(0.5, sampler="gpu")


def test_draws_are_bitwise_reproducible(golden, yeast_dcool):
    dc = yeast_dcool
    a = css.subsample_csr(dc, 0.4, seed=5, inter=True)
    b = css.subsample_csr(dc, 0.4, seed=5, inter=True)
    other = pipeline.DeviceCool(golden("yeast_cool"), dev=Device(0))
    c = css.subsample_csr(other, 0.4, seed=5, inter=True)
    ha = _csr_host(a)
    for r in (b, c):
        assert r["nnz"] == a["nnz"] and r["val_dtype"] is a["val_dtype"]
        for x, y in zip(ha, _csr_host(r)):
            assert np.array_equal(x, y)
    d = css.subsample_csr(dc, 0.4, seed=6, inter=True)
    assert not np.array_equal(_new_counts(dc, a), _new_counts(dc, d))
    # an intra block draws the same whichever other blocks are sampled
    b1, b2, _ = _host_table(dc)
    c1, c2 = _chroms(dc, b1, b2)
    intra = c1 == c2
    off = css.subsample_csr(dc, 0.4, seed=5, inter=False)
    assert np.array_equal(_new_counts(dc, a)[intra], _new_counts(dc, off)[intra])


def _many_chromosomes(n_chrom, size, pixels, trans=()):
    """n_chrom identical chromosomes of `size` bins: intra pixels [(i, j, count)] in every chromosome, trans pixels
    [(i, j, count)] (bin i of chromosome a, bin j of chromosome b) in every pair a < b."""
    off = np.arange(n_chrom + 1, dtype=np.int64) * size
    rows = []
    for a in range(n_chrom):
        for i, j, c in pixels:
            rows.append((off[a] + i, off[a] + j, c))
        for b in range(a + 1, n_chrom):
            for i, j, c in trans:
                rows.append((off[a] + i, off[b] + j, c))
    t = np.array(sorted(rows), dtype=np.int64)
    n = int(off[-1])
    return {"binsize": 1000, "chrom_offset": off, "chrom_names": np.array([f"c{a}" for a in range(n_chrom)]),
            "bin1_id": t[:, 0], "bin2_id": t[:, 1], "count": t[:, 2], "weight": np.ones(n),
            "bin_start": np.tile(np.arange(size) * 1000, n_chrom), "bin_end": np.tile(np.arange(1, size + 1) * 1000, n_chrom)}


def test_small_draws_follow_the_exact_pmf():
    """300 identical chromosomes: every block is one independent draw.  Intra blocks (with mirror copies) and trans blocks
    against the enumerated multivariate hypergeometric pmf, over three fixed seeds."""
    intra = [(0, 0, 2), (0, 1, 1), (1, 2, 2), (2, 2, 1)]
    trans = [(0, 1, 2), (1, 0, 1), (2, 2, 1)]
    n_chrom = 300
    dc = pipeline.DeviceCool(_many_chromosomes(n_chrom, 3, intra, trans))
    b1, b2, _ = _host_table(dc)
    c1, c2 = _chroms(dc, b1, b2)
    for sample in (0.5, 0.3):
        got_intra, got_trans = [], []
        for seed in (1, 2, 3):
            new = _new_counts(dc, css.subsample_csr(dc, sample, seed=seed, inter=True))
            sel = c1 == c2
            got_intra += [tuple(r) for r in new[sel].reshape(n_chrom, len(intra))]
            # a trans block's pixels are spread over its rows: group them by block, table order kept inside a block
            order = np.lexsort((np.flatnonzero(~sel), c2[~sel], c1[~sel]))
            got_trans += [tuple(r) for r in new[~sel][order].reshape(-1, len(trans))]
        p_intra = chi2_against_pmf(got_intra, block_pmf([c for _, _, c in intra], [i != j for i, j, _ in intra], sample))
        p_trans = chi2_against_pmf(got_trans, block_pmf([c for _, _, c in trans], [False] * len(trans), sample))
        print(f"sample {sample}: intra p = {p_intra:.3g} ({len(got_intra)} draws), trans p = {p_trans:.3g} ({len(got_trans)} draws)")
        assert p_intra >= 1e-3 and p_trans >= 1e-3


@pytest.mark.parametrize("good,bad", [(10 ** 6, 3 * 10 ** 6), (4 * 10 ** 8, 5 * 10 ** 8), (999_999_937, 3 * 10 ** 8)])
def test_large_draws_match_the_hypergeometric_moments_and_numpy(good, bad):
    """Blocks of two diagonal pixels (good, bad) keeping about half: the left pixel's draw is Hypergeometric(good, bad, keep)
    from the rejection branch.  Moments within 5 sigma; two-sample chi-square against numpy's sampler."""
    n_chrom = 3000
    dc = pipeline.DeviceCool(_many_chromosomes(n_chrom, 2, [(0, 0, good), (1, 1, bad)]))
    assert dc.val_dtype is (np.float64 if max(good, bad) >= 1 << 24 else np.float32)
    draws = []
    for seed in (7, 8, 9, 10):
        res = css.subsample_csr(dc, 0.5, seed=seed, drawn=True)
        keep = int(0.5 * (good + bad))
        assert np.all(res["blocks"]["keep"] == keep)
        draws.append(res["drawn"][0::2])
    x = np.concatenate(draws).astype(np.float64)
    N = good + bad
    mean = keep * good / N
    var = keep * (good / N) * (bad / N) * (N - keep) / (N - 1)
    n = x.size
    assert abs(x.mean() - mean) < 5 * np.sqrt(var / n), (x.mean(), mean)
    assert abs(x.var(ddof=1) - var) < 5 * var * np.sqrt(2.0 / (n - 1)), (x.var(ddof=1), var)
    ref = np.random.default_rng(1).hypergeometric(good, bad, keep, size=n)
    p = two_sample_chi2(x.astype(np.int64), ref)
    print(f"({good}, {bad}): mean {x.mean():.6g} / {mean:.6g}, var {x.var(ddof=1):.6g} / {var:.6g}, two-sample p = {p:.3g}")
    assert p >= 1e-3


def _yeast_cfgs():
    # half of the yeast map's pixels hold a single contact: after subsampling most windows exceed the default 10 % of zeros,
    # so the zero filter is opened to leave patterns to compare
    loops = dict(copy.deepcopy(ck.loops), max_perc_zero=100.0)
    borders = dict(copy.deepcopy(ck.borders), max_perc_zero=100.0)
    return loops, borders


def _same_tables(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for col in a.columns:
        x, y = a[col].to_numpy(), b[col].to_numpy()
        if col in ("score", "pvalue", "qvalue"):
            assert np.allclose(x.astype(float), y.astype(float), rtol=1e-9, atol=1e-12, equal_nan=True), col
        else:
            assert np.array_equal(x, y), col


@pytest.mark.parametrize("inter", [False, True])
def test_detect_with_device_subsample_equals_an_upload_of_the_table(golden, inter):
    cool = golden("yeast_cool")
    dc = pipeline.DeviceCool(cool)
    sub = dc.subsampled(0.5, seed=3, inter=inter, sampler="device")
    up = pipeline.DeviceCool(sub.host)
    loops, borders = _yeast_cfgs()
    got = pipeline.detect(dc, loops, inter=inter, subsample=0.5, seed=3, sampler="device", return_windows=True)
    want = pipeline.detect(up, loops, inter=inter, return_windows=True)
    _same_tables(got[0], want[0])
    assert np.allclose(got[1], want[1], rtol=0, atol=1e-12, equal_nan=True)
    assert len(got[0]) > 0
    if not inter:
        # the genome-step route (no windows) and borders
        _same_tables(pipeline.detect(dc, loops, subsample=0.5, seed=3, sampler="device"), pipeline.detect(up, loops))
        _same_tables(pipeline.detect(dc, borders, subsample=0.5, seed=3, sampler="device"), pipeline.detect(up, borders))


def test_quantify_with_device_subsample_equals_an_upload_of_the_table(golden):
    cool = golden("yeast_cool")
    g = golden("yeast_quantify")
    names = [str(n) for n in cool["chrom_names"]]
    binsize = int(cool["binsize"])
    rows = []
    for bi in range(int(g["n_blocks"])):
        ca, cb = (int(x) for x in g[f"b{bi}_chroms"])
        for r, c in g[f"b{bi}_coords"]:
            rows.append((names[ca], int(r) * binsize, (int(r) + 1) * binsize, names[cb], int(c) * binsize, (int(c) + 1) * binsize))
    positions = pd.DataFrame(rows, columns=["chrom1", "start1", "end1", "chrom2", "start2", "end2"])
    cfg = dict(pearson=0.15, max_perc_undetected=75.0, max_perc_zero=100.0, max_dist=0, min_dist=0,
               kernels=[g[f"kernel{ki}"] for ki in range(3)], max_iterations=1, min_separation=5000)
    md = int(g["cfg_max_dist_bp"])
    dc = pipeline.DeviceCool(cool)
    up = pipeline.DeviceCool(dc.subsampled(0.5, seed=3, inter=True, sampler="device").host)
    got, got_w = pipeline.quantify(dc, positions, cfg, inter=True, max_dist_bp=md, subsample=0.5, seed=3, sampler="device")
    want, want_w = pipeline.quantify(up, positions, cfg, inter=True, max_dist_bp=md)
    _same_tables(got, want)
    assert np.isfinite(got.score.to_numpy(dtype=float)).sum() > 100
    assert np.array_equal(np.isnan(got_w), np.isnan(want_w))
    assert np.allclose(got_w, want_w, rtol=0, atol=1e-12, equal_nan=True)


def test_hg38_scale_table_subsamples_and_runs_detect_inter():
    """A synthetic hg38-proportioned table (24 chromosomes, 300 blocks with --inter) of more than 30 M pixels: exact block
    totals, then `detect --inter` of the subsampled table under a 2 GiB strip budget."""
    from tools.synthetic_inter import make_trans_cool
    cool, planted = make_trans_cool(seed=5, template=ck.loops["kernels"][0])
    dc = pipeline.DeviceCool(cool)
    assert dc.nnz >= 30_000_000
    res = css.subsample_csr(dc, 0.5, seed=9, inter=True, drawn=True)
    b1, b2, cnt = _host_table(dc)
    c1, c2 = _chroms(dc, b1, b2)
    cnt = cnt.astype(np.int64)
    bid = c1 * dc.n_chrom + c2
    mult = np.where((c1 == c2) & (b1 != b2), 2, 1)
    totals = np.bincount(bid, weights=(cnt * mult).astype(np.float64), minlength=dc.n_chrom ** 2).astype(np.int64)
    drawn = np.bincount(bid, weights=res["drawn"].astype(np.float64), minlength=dc.n_chrom ** 2).astype(np.int64)
    assert len(res["blocks"]) == 300
    for blk in res["blocks"]:
        k = int(blk["chrom1"]) * dc.n_chrom + int(blk["chrom2"])
        assert int(blk["total"]) == totals[k] and int(blk["keep"]) == int(0.5 * totals[k]) == drawn[k]
    sub = pipeline.DeviceCool.from_device_csr(dc, res["indptr"], res["indices"], res["data"], res["nnz"], res["val_dtype"])
    cfg = dict(copy.deepcopy(ck.loops), max_perc_zero=100.0)         # trans counts are 1 or 2: half of them drop to 0
    table = pipeline.detect(sub, cfg, inter=True, inter_budget=2 << 30)
    assert sub.inter_high_water <= 2 << 30
    assert len(table) > 0
    print(f"hg38-scale: {dc.nnz} pixels -> {sub.nnz}; detect --inter: {len(table)} patterns, "
          f"{int((table.chrom1 != table.chrom2).sum())} trans")
