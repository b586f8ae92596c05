"""The matrix-core kernel of the templates with a side of 34 .. 81 (chromosight_amd/csrc/cs_corr_large.hip, cs_last_kernel() ==
CS_KERNEL_MFMA_LARGE): candidate calls reach it by default and give the lists the runtime-size kernel gives
(CHROMOSIGHT_HIP_NO_LARGE=1); its coefficients (maps under CHROMOSIGHT_HIP_LARGE=1) against the C oracle; the candidate screen
loses no pixel at or above pearson; detect / quantify --inter with the `centromeres` preset equal the runtime-size route."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd import engine, pipeline
from chromosight_amd._lib import get_device
from chromosight_amd.utils import detection as cud
from chromosight_amd.utils import preprocessing as cup
from oracle import c_oracle
from tools.synthetic_inter import make_trans_cool

pytestmark = pytest.mark.gpu

KERNEL_GENERIC, KERNEL_MFMA_LARGE = 1, 9          # include/chromosight_hip.h
CENTRO = np.asarray(ck.centromeres["kernels"][0], dtype=np.float64)
# float32 sums of up to 6561 terms (what the runtime-size kernel reaches on 81 x 81: 2e-4).  The candidate screen only needs the
# float32 value to fall within its margin (engine.rescore_margin, >= 1e-4 at pearson 0.5 ... ) of the float64 one on
# well-conditioned windows -- everything else is re-scored in float64 -- so the maps are held to that bound.
TOL = 2e-4
COND_EPS = 1e-3


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


def last_kernel():
    dev = get_device()
    return dev.lib.cs_last_kernel(dev.ctx)


def template(shape, seed=0):
    """A full-rank template with structure (a blob on a gradient plus noise)."""
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + seed)
    i, j = np.indices(shape)
    ci, cj = (shape[0] - 1) / 2, (shape[1] - 1) / 2
    blob = np.exp(-((i - ci) ** 2 + (j - cj) ** 2) / (0.08 * shape[0] * shape[1] + 1))
    return 0.4 + blob + 0.02 * (i - j) + 0.15 * rng.normal(size=shape)


def _check(got, want, cond, what):
    got = got.toarray() if sp.issparse(got) else np.asarray(got, dtype=np.float64)
    well = cond >= COND_EPS
    err = float(np.abs(got - want)[well].max())
    print(f"[large] {what}: max|err| {err:.2e} on {int(well.sum())} well-conditioned pixels")
    assert err < TOL, (what, err)
    assert np.all(np.abs(got) <= 1.0 + 1e-6), what


# ---------------------------------------------------------------------------------------------------------------------------
# coefficients (maps under CHROMOSIGHT_HIP_LARGE=1) against the oracle

# (the API takes odd sides only; 49 is the last side of two Toeplitz passes, 51 the first of three)
@pytest.mark.parametrize("kshape", [(35, 35), (41, 41), (49, 49), (51, 51), (65, 65), (81, 81), (35, 81), (81, 41), (21, 71)])
@pytest.mark.parametrize("full", [True, False])
def test_dense_maps_match_oracle(kshape, full, monkeypatch):
    monkeypatch.setenv("CHROMOSIGHT_HIP_LARGE", "1")
    rng = np.random.default_rng(kshape[0] * 100 + kshape[1])
    sig = rng.gamma(2.0, 1.0, size=(300, 333)).astype(np.float32)
    kern = template(kshape)
    got, _ = cud.normxcorr2(sig, kern, full=full)
    assert last_kernel() == KERNEL_MFMA_LARGE
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), kern, 0, sig.shape[0], full=full)
    _check(got, want, cond, f"dense {kshape} full={full}")


def test_map_calls_stay_on_the_runtime_size_kernel_by_default():
    sig = np.random.default_rng(1).gamma(2.0, 1.0, size=(200, 200)).astype(np.float32)
    cud.normxcorr2(sig, template((41, 41)), full=True)
    assert last_kernel() == KERNEL_GENERIC


@pytest.mark.parametrize("full", [True, False])
def test_centromeres_on_a_masked_inter_block(full, monkeypatch):
    """The shipped 81 x 81 template on a trans block with missing bins (test_gpu_parity's block), float64 container."""
    monkeypatch.setenv("CHROMOSIGHT_HIP_LARGE", "1")
    rng = np.random.default_rng(81)
    ms, ns = 600, 520
    a = rng.gamma(4, 0.25, size=(ms, ns)) * (rng.random((ms, ns)) > 0.3)
    a[200:281, 300:381] = CENTRO / CENTRO.mean() * rng.gamma(50, 0.02, size=CENTRO.shape)
    mr, mc = np.zeros(ms, bool), np.zeros(ns, bool)
    mr[[7, 100, 101, 433, 599]] = True
    mc[[0, 250, 251, 252, 519]] = True
    a[mr, :] = 0
    a[:, mc] = 0
    mask = cup.make_missing_mask((ms, ns), np.flatnonzero(~mr), np.flatnonzero(~mc), sym_upper=False)
    got, _ = cud.normxcorr2(sp.csr_matrix(a), CENTRO, full=full, missing_mask=mask, missing_tol=0.5)
    assert last_kernel() == KERNEL_MFMA_LARGE
    want, cond = c_oracle.normxcorr2_rows(a, CENTRO, 0, ms, full=full, miss_row=mr, miss_col=mc, missing_tol=0.5)
    _check(got, want, cond, f"centromeres inter full={full}")
    assert np.nanmax(want) > 0.5


@pytest.mark.parametrize("kshape,md", [((81, 81), 300), ((49, 49), 150), ((35, 81), 200)])
def test_banded_maps_with_bin_masks(kshape, md, monkeypatch):
    """The intra configuration: CSR in, band in / band out, per-bin masks, sym_upper, full."""
    monkeypatch.setenv("CHROMOSIGHT_HIP_LARGE", "1")
    n = 700
    rng = np.random.default_rng(n + md)
    ii, jj = np.indices((n, n))
    sig = np.triu(np.minimum(rng.gamma(20, 0.05, size=(n, n)), 10.0))
    sig[jj - ii > md + max(kshape)] = 0
    miss = rng.random(n) < 0.04
    sig[miss, :] = 0
    sig[:, miss] = 0
    valid = np.flatnonzero(~miss)
    band = (jj - ii >= 0) & (jj - ii <= md)
    kern = template(kshape)
    mask = cup.make_missing_mask((n, n), valid, valid, max_dist=md, sym_upper=True)
    c, _ = cud.normxcorr2(sp.csr_matrix(sig.astype(np.float32)), kern, max_dist=md, sym_upper=True, full=True, missing_mask=mask,
                          missing_tol=0.75)
    assert last_kernel() == KERNEL_MFMA_LARGE
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float32).astype(np.float64), kern, 0, n, max_dist=md, sym_upper=True,
                                          full=True, miss_row=miss, miss_col=miss, missing_tol=0.75)
    _check(c.toarray()[band], want[band], cond[band], f"band {kshape} md={md}")


def test_explicit_mask_and_f64_dense(monkeypatch):
    monkeypatch.setenv("CHROMOSIGHT_HIP_LARGE", "1")
    rng = np.random.default_rng(3)
    sig = rng.gamma(2.0, 1.0, size=(260, 300))                  # float64 container
    m = rng.random(sig.shape) < 0.03
    sig[m] = 0
    kern = template((45, 45))
    got, _ = cud.normxcorr2(sig, kern, full=False, missing_mask=sp.csr_matrix(m), missing_tol=0.75)
    assert last_kernel() == KERNEL_MFMA_LARGE
    monkeypatch.setenv("CHROMOSIGHT_HIP_NO_LARGE", "1")
    ref, _ = cud.normxcorr2(sig, kern, full=False, missing_mask=sp.csr_matrix(m), missing_tol=0.75)
    assert last_kernel() == KERNEL_GENERIC
    assert np.abs(np.asarray(got) - np.asarray(ref)).max() < TOL
    monkeypatch.delenv("CHROMOSIGHT_HIP_NO_LARGE")
    got, _ = cud.normxcorr2(sig, kern, full=True)
    assert last_kernel() == KERNEL_MFMA_LARGE
    want, cond = c_oracle.normxcorr2_rows(sig, kern, 0, sig.shape[0], full=True)
    _check(got, want, cond, "f64 dense full")


# ---------------------------------------------------------------------------------------------------------------------------
# candidate calls: the new kernel by default, the same lists as the runtime-size kernel

@pytest.fixture(scope="module")
def trans():
    cool, planted = make_trans_cool(n_chroms=3, intra_diags=30, n_trans=300_000, n_planted=6, template=CENTRO, binsize=2000, seed=3,
                                    chrom_sizes=[701, 853, 599])
    return cool, planted


def _candidates(dcool, ca, cb, rows, kspec, pearson, tiles_of=None):
    n_r, n_c = dcool.chrom_size(ca), dcool.chrom_size(cb)
    cfg = dict(ck.centromeres, pearson=pearson)
    reach = pipeline._strip_reach([kspec.kernel if hasattr(kspec, "kernel") else CENTRO])
    blk = dcool.stage_inter(ca, cb, rows=rows, largest_kernel=reach)
    kw = dict(pearson=pearson, lo_diag=-(n_r - 1), hi_diag=n_c - 1, **pipeline._strip_common(blk, cfg))
    if tiles_of is None:
        return engine.run_candidates(dcool.dev, blk.sig, (n_r, n_c), kspec, rows, **kw)
    tiles, nt = engine.run_tile_occupancy(dcool.dev, blk.view, blk.view_row0, kspec.km, kspec.kn, rows, n_c)
    return engine.run_candidates_tiles(dcool.dev, blk.sig, (n_r, n_c), kspec, rows, tiles, nt, **kw), nt


@pytest.mark.parametrize("pearson", [0.5, 0.2])
def test_inter_block_candidates_equal_the_runtime_size_kernel(trans, pearson, monkeypatch):
    cool, _ = trans
    dcool = pipeline.DeviceCool(cool)
    kspec = engine.KernelSpec(CENTRO)
    n = 0
    for ca, cb in [(0, 1), (1, 2), (0, 2)]:
        n_r = dcool.chrom_size(ca)
        for rows in [(0, n_r), (n_r // 3 + 5, n_r // 3 + 170)]:
            monkeypatch.delenv("CHROMOSIGHT_HIP_NO_LARGE", raising=False)
            got = _candidates(dcool, ca, cb, rows, kspec, pearson)
            assert last_kernel() == KERNEL_MFMA_LARGE
            (lst, nt) = _candidates(dcool, ca, cb, rows, kspec, pearson, tiles_of=True)
            if nt:
                assert last_kernel() == KERNEL_MFMA_LARGE
            monkeypatch.setenv("CHROMOSIGHT_HIP_NO_LARGE", "1")
            ref = _candidates(dcool, ca, cb, rows, kspec, pearson)
            assert last_kernel() == KERNEL_GENERIC
            for a, b, c in zip(got, ref, lst):
                assert np.array_equal(a, b)
                assert np.array_equal(a, c)
            n += got[0].size
    assert n > 0
    print(f"pearson {pearson}: {n} candidates")


def _dense_candidates(a, kern, pearson, miss, *, sym_upper=False, max_dist=None):
    from chromosight_amd._lib import CsMatrix, LAYOUT_DENSE, MASK_BINS, np_dtype_code
    dev = get_device()
    ms, ns = a.shape
    ld = (ns + 15) // 16 * 16
    host = np.zeros((ms, ld))
    host[:, :ns] = a
    buf = dev.to_device(host)
    sig = CsMatrix(buf.ptr, np_dtype_code(np.float64), LAYOUT_DENSE, ld, 0, 0)
    fr, fc = dev.to_device(miss[0].astype(np.uint8)), dev.to_device(miss[1].astype(np.uint8))
    md = -1 if max_dist is None else max_dist
    out = engine.run_candidates(dev, sig, (ms, ns), engine.KernelSpec(kern), (0, ms), pearson=pearson,
                                lo_diag=0 if sym_upper else -(ms - 1), hi_diag=md if sym_upper else ns - 1, inter=not sym_upper,
                                full=True, sym_upper=sym_upper, max_dist=md, mask_mode=1, miss_row=fr, miss_col=fc,
                                missing_tol=0.5)
    del buf
    return out


@pytest.mark.parametrize("pearson", [0.5, 0.15])
@pytest.mark.parametrize("sym_upper", [False, True])
def test_the_screen_loses_no_passing_pixel(pearson, sym_upper):
    """Plateau maps (value 5 +- a few 1e-3) carrying faint 81 x 81 copies, so that the float64 coefficients straddle pearson while
    float32 sums of 6561 terms evaluate them with large relative errors: the candidates (re-scored in float64) are exactly the
    pixels whose float64 coefficient passes, at the preset's 0.5 and at 0.15.  A dense trans-style block and a masked band."""
    n = 420
    kz = (CENTRO - CENTRO.mean()) / CENTRO.std()
    passing = 0
    for amp in (0.2, 0.35, 0.5, 0.7, 0.9, 1.5):
        rng = np.random.default_rng(int(amp * 100) + 7 * sym_upper)
        a = 5.0 * (1.0 + 2e-3 * rng.standard_normal((n, n)))
        centres = [(120, 200), (300, 330)] if sym_upper else [(120, 200), (300, 90)]
        for i0, j0 in centres:
            a[i0 - 40:i0 + 41, j0 - 40:j0 + 41] += 5.0 * 2e-3 * amp * kz
        miss = np.zeros(n, bool)
        miss[rng.choice(n, size=8, replace=False)] = True
        md = 260 if sym_upper else None
        ii, jj = np.indices((n, n))
        if sym_upper:
            a[(jj - ii < 0) | (jj - ii > md + 81)] = 0
        a[miss, :] = 0
        a[:, miss] = 0
        want, _ = c_oracle.normxcorr2_rows(a, CENTRO, 0, n, max_dist=md, sym_upper=sym_upper, full=True, miss_row=miss,
                                           miss_col=miss, missing_tol=0.5)
        rows, cols, vals = _dense_candidates(a, CENTRO, pearson, (miss, miss), sym_upper=sym_upper, max_dist=md)
        assert last_kernel() == KERNEL_MFMA_LARGE
        got = np.zeros((n, n), dtype=bool)
        got[rows, cols] = True
        exp = (want >= pearson) & (want != 0)
        if sym_upper:
            exp &= (jj - ii >= 0) & (jj - ii <= md)
        edge = np.abs(want - pearson) < 1e-9
        assert np.array_equal(got & ~edge, exp & ~edge), (amp, int(got.sum()), int(exp.sum()))
        if rows.size:
            assert np.abs(vals - want[rows, cols]).max() < 1e-7
        passing += int(exp.sum())
        print(f"amp {amp} pearson {pearson} sym_upper {sym_upper}: {int(exp.sum())} passing pixels")
    assert passing > 0


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: detect / quantify --inter with the centromeres preset

def _same_tables(a, b):
    """Same table (coordinates, order, scores) and windows; the windows of trans positions may differ by a few 1e-15 between two
    runs whatever the kernel (test_gpu_inter_strips.py), hence 1e-12 there."""
    import pandas as pd
    ta, wa = a
    tb, wb = b
    pd.testing.assert_frame_equal(ta, tb)
    wa, wb = np.asarray(wa, dtype=np.float64), np.asarray(wb, dtype=np.float64)
    assert wa.shape == wb.shape
    assert np.array_equal(np.isnan(wa), np.isnan(wb))
    assert np.allclose(wa, wb, rtol=0, atol=1e-12, equal_nan=True)


def test_yeast_centromeres_detect_and_quantify_equal_the_runtime_size_route(golden, monkeypatch):
    """detect --inter (intra blocks whole: the preset's max_dist = 0; trans blocks in strips through their tile lists) and
    quantify --inter on the detected positions plus 200 random trans ones: the same tables and windows on both kernels."""
    import pandas as pd
    cool = golden("yeast_cool")
    cfg = copy.deepcopy(ck.centromeres)
    cfg["max_perc_zero"] = 100.0
    cfg["pearson"] = 0.15
    res = {}
    pos = None
    for large in (True, False):
        if large:
            monkeypatch.delenv("CHROMOSIGHT_HIP_NO_LARGE", raising=False)
        else:
            monkeypatch.setenv("CHROMOSIGHT_HIP_NO_LARGE", "1")
        dcool = pipeline.DeviceCool(cool)
        det = pipeline.detect(dcool, cfg, inter=True, return_windows=True)
        assert last_kernel() == (KERNEL_MFMA_LARGE if large else KERNEL_GENERIC)
        if pos is None:
            rng = np.random.default_rng(4)
            pos = det[0][["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].copy()
            names, sizes = dcool.names, np.diff(dcool.offsets)
            extra = []
            for _ in range(200):
                ca, cb = np.sort(rng.choice(len(names), 2, replace=False))
                s1, s2 = int(rng.integers(0, sizes[ca])) * dcool.binsize, int(rng.integers(0, sizes[cb])) * dcool.binsize
                extra.append((names[ca], s1, s1 + dcool.binsize, names[cb], s2, s2 + dcool.binsize))
            pos = pd.concat([pos, pd.DataFrame(extra, columns=pos.columns)], ignore_index=True)
        q = pipeline.quantify(dcool, pos, cfg, inter=True)
        res[large] = (det, q)
    _same_tables(res[True][0], res[False][0])
    _same_tables(res[True][1], res[False][1])
    assert len(res[True][0][0]) > 0 and len(res[True][1][0]) > 0
    print(f"centromeres --inter: {len(res[True][0][0])} patterns, {len(res[True][1][0])} quantified")


def test_synthetic_genome_planted_centromeres_are_found():
    """A 309 988-bin genome with planted 81 x 81 trans patterns, detect --inter in strips under a 2 GiB budget."""
    cool, planted = make_trans_cool(total_bins=310_000, n_chroms=24, intra_diags=200, n_trans=20_000_000, n_planted=40,
                                    template=CENTRO, binsize=10_000, seed=5)
    dcool = pipeline.DeviceCool(cool)
    assert dcool.n_bins > 300_000
    cfg = copy.deepcopy(ck.centromeres)
    cfg["max_perc_zero"] = 100.0
    budget = 2 << 30
    table = pipeline.detect(dcool, cfg, inter=True, inter_budget=budget)
    assert last_kernel() == KERNEL_MFMA_LARGE
    assert dcool.inter_high_water <= budget
    trans = table[table.chrom1 != table.chrom2]
    found = set(zip(trans.bin1.astype(int), trans.bin2.astype(int)))
    hit = sum(any((abs(i - a) <= 1 and abs(j - b) <= 1) for a, b in found) for i, j in planted)
    print(f"synthetic genome: {hit}/{len(planted)} planted found, {len(trans)} trans patterns, high-water {dcool.inter_high_water}")
    assert hit == len(planted)
