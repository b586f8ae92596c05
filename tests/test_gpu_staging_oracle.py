"""Block staging on the device against oracle/detrend_oracle.py on the adversarial pixel tables of tests/staging_cases.py
(pinned on the CPU by tests/test_staging_cases_host.py): every staged block is downloaded WHOLE -- every row up to its pitch
-- and compared element by element.

Routes: (1) DeviceCool.stage_blocks served by the one-call entry (cs_stage_blocks / cs_stage_blocks_opt; checked: sig32 is
set only there): float64 band, its float32 copy, float32-only staging, smooth=True; (2) stage_intra block by block
(cs_csr_band_extent, cs_distance_law_csr / _finish, cs_csr_to_band), which is also what a table with a stored lower triangle
takes; (3) counts=True: bands of raw counts; (4) the short chromosomes either route stages dense.  Then stage_inter /
stage_inter_many against a block built on the host.

Bounds: 1e-11 absolute on random-valued tables (what the suite holds staging to against the reference's captures), 1e-13
relative where the laws are exact in any summation order, zero pattern and capped set identical everywhere, float32 == the
float64 band rounded once.  A law is a mean of fewer than n positive terms (n: bins of the chromosome), so two summation
orders differ by less than n * 2^-52 relative; a fitted law pools fewer than n such means: 2 n * 2^-52.

Lazily evaluated float64 bands (lazy64=True) are read through their descriptor by the batched kernels only; no entry writes
them out, so they are not compared here (test_lazy_float64_bands_equal_the_stored_ones holds them to the stored ones)."""
import ctypes as C

import numpy as np
import pytest

import staging_cases as sc
from chromosight_amd import pipeline
from chromosight_amd._lib import COUNTS_HEADER_BYTES, LAYOUT_BAND, LAYOUT_BAND_COUNTS, LAYOUT_BAND_PADDED, LAYOUT_DENSE

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _d2h(dev, ptr, shape, dtype):
    host = np.empty(shape, dtype=dtype)
    if host.nbytes:
        dev._check(dev.lib.cs_memcpy_d2h(dev.ctx, host.ctypes.data, C.c_void_p(ptr), host.nbytes, None))
    return host


def download_rows(dcool, sig, n):
    """Every element of a staged map: n rows of sig.ld (download_block of test_gpu_device_pipeline.py crops the pitch)."""
    return _d2h(dcool.dev, sig.d_ptr, (n, int(sig.ld)), np.float64 if sig.dtype == 1 else np.float32)


def _want(case, ci, max_dist, smooth=False):
    cache = case.__dict__.setdefault("_rows", {})
    key = (ci, max_dist, smooth)
    if key not in cache:
        cache[key] = sc.expected_rows(case, ci, max_dist, smooth)
    return cache[key]


class Tally:
    def __init__(self, case, route):
        self.head, self.n, self.abs, self.rel, self.capped, self.blocks, self.dense = f"{case.name} / {route}", 0, 0.0, 0.0, 0, 0, 0

    def report(self):
        if not self.blocks:
            return
        print(f"{self.head}: {self.blocks} blocks ({self.dense} dense), {self.n} elements compared, worst error {self.abs:.2e} absolute "
              f"{self.rel:.2e} relative, {self.capped} capped pixels, excluded: 0")


def check_geometry(case, dcool, ci, max_dist, blk, only32=False, fast=False, counts=False):
    n = case.n(ci)
    keep, band, band_w, ld = sc.geometry(max_dist, n)
    assert keep == min(max_dist, n) + sc.LARGEST and band_w == (min(keep, n - 1) + 1 if band else 0)
    where = (case.name, ci, max_dist)
    assert blk.keep == keep and blk.shape == (n, n) and not blk.inter, where
    s = blk.sig32 if (only32 and fast) else blk.sig
    if counts and band:
        assert s.layout == LAYOUT_BAND_COUNTS and s.band_w == band_w and s.ld >= band_w + 4 and s.ld % 64 == 0, where
    else:
        padded = fast and only32 and band and ld >= band_w + 4
        assert s.layout == (LAYOUT_BAND_PADDED if padded else LAYOUT_BAND if band else LAYOUT_DENSE), where
        assert (s.ld, s.band_w, s.band_lo, s.row0) == (ld, band_w, 0, 0), where
        assert s.dtype == (0 if only32 else 1), where
    if fast and not only32:
        t = blk.sig32
        assert t.layout == (LAYOUT_BAND_PADDED if band and ld >= band_w + 4 else LAYOUT_BAND if band else LAYOUT_DENSE), where
        assert (t.ld, t.band_w, t.band_lo, t.dtype) == (ld, band_w, 0, 0), where
    det = case.expected(ci, keep)[2]
    for flags in (blk.miss_row, blk.miss_col):
        assert np.array_equal(_d2h(dcool.dev, flags.ptr, (n,), np.uint8), (~det).astype(np.uint8)), where
    assert np.array_equal(dcool.block_bins(ci), np.flatnonzero(det)), where
    return band, band_w, ld


def check_values(case, ci, max_dist, got, tally, smooth=False, band_w=0):
    """got: the downloaded float64 rows [n, ld]."""
    where = (case.name, ci, max_dist, smooth)
    want, ratio = _want(case, ci, max_dist, smooth)
    assert got.shape == want.shape, where
    n = case.n(ci)
    if band_w:
        assert not got[:, band_w:].any(), where                                        # band_w .. ld
        cols = np.arange(n)[:, None] + np.arange(band_w)[None, :]
        assert not got[:, :band_w][cols >= n].any(), where                             # columns at or beyond n
    else:
        assert not got[:, n:].any() and not np.tril(got[:, :n], -1).any(), where
    assert np.all(np.isfinite(got)), where
    assert np.array_equal(got == 0, want == 0), (where, np.argwhere((got == 0) != (want == 0))[:5])
    with np.errstate(invalid="ignore"):
        over = np.nan_to_num(ratio, nan=0.0, posinf=np.inf) >= sc.MAX_VAL
    assert np.array_equal((got == 1.0) & over, (want == 1.0) & over) and np.all(want[over] == 1.0), where
    err = np.abs(got - want)
    nz = want != 0
    rel = float((err[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
    tally.n += got.size
    tally.abs, tally.rel = max(tally.abs, float(err.max()) if err.size else 0.0), max(tally.rel, rel)
    tally.capped += int(((got == 1.0) & over).sum())
    tally.blocks += 1
    tally.dense += 0 if band_w else 1
    if case.exact:
        assert np.all(err <= 1e-13 * np.abs(want)), (where, rel)
    else:
        assert err.max(initial=0.0) <= 1e-11, (where, float(err.max()))


def check_law(case, dcool, ci, max_dist, blk, smooth=False):
    n = case.n(ci)
    keep = sc.keep_of(max_dist, n)
    nd = min(n, keep + 1)
    assert blk.n_diags == nd
    got = _d2h(dcool.dev, blk.d_law, (nd,), np.float64)
    want = np.nan_to_num(case.expected(ci, keep, smooth)[1][:nd], nan=0.0)
    assert np.array_equal(got == 0, want == 0), (case.name, ci, max_dist, smooth)
    bound = 0.0 if case.exact else (2 if smooth else 1) * n * EPS
    assert np.all(np.abs(got - want) <= bound * np.abs(want)), (case.name, ci, max_dist, smooth, np.abs(got - want).max())


def check_inputs(case, dcool):
    cool = case.cool
    assert dcool.val_dtype is case.val_dtype and dcool.upper == (not case.symmetric)
    assert np.array_equal(dcool.indptr.download(), np.searchsorted(cool["bin1_id"], np.arange(dcool.n_bins + 1)))
    assert np.array_equal(dcool.indices.download(), cool["bin2_id"].astype(np.int32))
    assert np.array_equal(dcool.data.download(), cool["count"].astype(case.val_dtype))
    assert np.array_equal(dcool.weight.download(), cool["weight"], equal_nan=True)
    assert np.array_equal(dcool.miss.download(), np.isnan(cool["weight"]).astype(np.uint8))


UPPER = [k for k in sc.BUILDERS if not k.endswith("_sym")]


@pytest.mark.parametrize("name", UPPER)
def test_one_call_staging_equals_the_oracle(name):
    """Route 1: float64 band + float32 copy, float32-only, smooth."""
    case = sc.get(name)
    dcool = pipeline.DeviceCool(case.cool)
    t64, tsm = Tally(case, "stage_blocks float64 + float32 copy"), Tally(case, "stage_blocks smooth")
    n32 = b32s = 0
    for st in case.stagings:
        md, chroms = st[0], case.chroms(st)
        fast = dcool.stage_blocks(chroms, md, sc.LARGEST)
        only = dcool.stage_blocks(chroms, md, sc.LARGEST, band_dtype=np.float32)
        assert all(b.sig32 is not None for b in fast + only), "the one-call entry did not serve the call"
        for ci, blk, b32 in zip(chroms, fast, only):
            n = case.n(ci)
            band, band_w, ld = check_geometry(case, dcool, ci, md, blk, fast=True)
            check_geometry(case, dcool, ci, md, b32, only32=True, fast=True)
            got = download_rows(dcool, blk.sig, n)
            check_values(case, ci, md, got, t64, band_w=band_w)
            check_law(case, dcool, ci, md, blk)
            assert np.array_equal(download_rows(dcool, blk.sig32, n), got.astype(np.float32)), (name, ci, md)
            got32 = download_rows(dcool, b32.sig32, n)
            assert b32.sig is b32.sig32 or b32.sig.d_ptr == b32.sig32.d_ptr
            assert np.array_equal(got32, got.astype(np.float32)), (name, ci, md)
            n32, b32s = n32 + got32.size, b32s + 1
    for st in case.smooth:
        md, chroms = st[0], case.chroms(st)
        fast = dcool.stage_blocks(chroms, md, sc.LARGEST, smooth=True)
        assert all(b.sig32 is not None for b in fast), "the one-call entry did not serve the smoothed call"
        for ci, blk in zip(chroms, fast):
            band, band_w, ld = check_geometry(case, dcool, ci, md, blk, fast=True)
            got = download_rows(dcool, blk.sig, case.n(ci))
            check_values(case, ci, md, got, tsm, smooth=True, band_w=band_w)
            check_law(case, dcool, ci, md, blk, smooth=True)
            assert np.array_equal(download_rows(dcool, blk.sig32, case.n(ci)), got.astype(np.float32)), (name, ci, md)
    check_inputs(case, dcool)
    if name == "sizes":
        assert t64.dense > 50 and t64.blocks - t64.dense > 10          # route 4: both layouts staged
    for t in (t64, tsm):
        t.report()
    print(f"{name} / stage_blocks float32 only: {b32s} blocks, {n32} elements equal to the float64 band rounded once, excluded: 0")


@pytest.mark.parametrize("name", list(sc.BUILDERS))
def test_block_by_block_staging_equals_the_oracle(name):
    """Route 2, on the upper tables and on the tables with a stored lower triangle (which stage_blocks hands to it as well)."""
    case = sc.get(name)
    dcool = pipeline.DeviceCool(case.cool)
    tally, tsm, tres = Tally(case, "stage_intra"), Tally(case, "stage_intra smooth"), Tally(case, "stage_blocks -> block by block")
    for st in case.stagings:
        md = st[0]
        for ci in case.chroms(st):
            blk = dcool.stage_intra(ci, md, sc.LARGEST)
            assert blk.sig32 is None
            band, band_w, ld = check_geometry(case, dcool, ci, md, blk)
            got = download_rows(dcool, blk.sig, case.n(ci))
            check_values(case, ci, md, got, tally, band_w=band_w)
            b32 = dcool.stage_intra(ci, md, sc.LARGEST, band_dtype=np.float32)
            check_geometry(case, dcool, ci, md, b32, only32=True)
            assert np.array_equal(download_rows(dcool, b32.sig, case.n(ci)), got.astype(np.float32)), (name, ci, md)
    for st in case.smooth:
        for ci in case.chroms(st):
            blk = dcool.stage_intra(ci, st[0], sc.LARGEST, smooth=True)
            band, band_w, ld = check_geometry(case, dcool, ci, st[0], blk)
            check_values(case, ci, st[0], download_rows(dcool, blk.sig, case.n(ci)), tsm, smooth=True, band_w=band_w)
    if case.symmetric:
        st = case.stagings[0]
        blocks = dcool.stage_blocks(case.chroms(st), st[0], sc.LARGEST)
        assert all(b.sig32 is None for b in blocks), "a table with a lower triangle went through the one-call entry"
        for ci, blk in zip(case.chroms(st), blocks):
            band, band_w, ld = check_geometry(case, dcool, ci, st[0], blk)
            check_values(case, ci, st[0], download_rows(dcool, blk.sig, case.n(ci)), tres, band_w=band_w)
    check_inputs(case, dcool)
    for t in (tally, tsm, tres):
        t.report()


def counts_rows(case, ci, band_w, ld):
    """The band of raw counts a block must hold: slot d of row r = the stored count of (r, r + d), 0 elsewhere."""
    off = case.offsets
    s, n = int(off[ci]), case.n(ci)
    b1, b2, cnt = case.cool["bin1_id"], case.cool["bin2_id"], case.cool["count"]
    sel = (b1 >= s) & (b1 < s + n) & (b2 >= b1) & (b2 < s + n) & (b2 - b1 < band_w)
    rows = np.zeros((n, ld), dtype=np.float32)
    rows[b1[sel] - s, b2[sel] - b1[sel]] = cnt[sel]
    return rows


@pytest.mark.parametrize("name", ["row_shapes", "missing", "diagonals"])
def test_bands_of_raw_counts_equal_the_pixel_table(name):
    """Route 3: counts=True with float32-only staging -- banded blocks hold the pixel table's counts exactly (their law is the
    oracle's; the detrended values are those of the same call with counts off, held to the oracle above); blocks staged
    dense by the same call are detrended as ever."""
    case = sc.get(name)
    dcool = pipeline.DeviceCool(case.cool)
    assert dcool.counts_ok
    n_counts = n_elem = 0
    for st in case.stagings:
        md, chroms = st[0], case.chroms(st)
        blocks = dcool.stage_blocks(chroms, md, sc.LARGEST, band_dtype=np.float32, counts=True)
        plain = dcool.stage_blocks(chroms, md, sc.LARGEST)
        assert all(b.sig32 is not None for b in blocks + plain), "the one-call entry did not serve the call"
        for ci, blk, ref in zip(chroms, blocks, plain):
            n = case.n(ci)
            band, band_w, ld = check_geometry(case, dcool, ci, md, blk, only32=True, fast=True, counts=True)
            check_law(case, dcool, ci, md, blk)
            got = download_rows(dcool, blk.sig32, n)
            if band:
                assert blk.buffer.ptr + COUNTS_HEADER_BYTES == blk.sig32.d_ptr
                assert np.array_equal(got, counts_rows(case, ci, band_w, int(blk.sig32.ld))), (name, ci, md)
                n_counts += 1
                n_elem += got.size
            else:
                assert np.array_equal(got, download_rows(dcool, ref.sig, n).astype(np.float32)), (name, ci, md)
    assert n_counts > 0
    check_inputs(case, dcool)
    print(f"{name} / stage_blocks counts: {n_counts} bands of raw counts, {n_elem} elements equal to the pixel table, excluded: 0")


@pytest.mark.parametrize("name", ["row_shapes", "row_shapes_sym"])
def test_staging_into_poisoned_buffers_equals_the_oracle(name):
    """Every element of a block is written exactly once, with no zero-fill pass: a block staged into buffers that just held the
    dense twin chromosome (same bins, every slot of the band positive; released to the genome's pool and taken again -- checked
    on the pointers) must equal the oracle like the first staging into fresh memory."""
    case = sc.get(name)
    ci, twin = case.meta["chrom"], case.meta["twin"]
    n = case.n(ci)
    dcool = pipeline.DeviceCool(case.cool)
    tally = Tally(case, "poisoned buffers")
    routes = {"float64 + float32": dict(), "float32 only": dict(band_dtype=np.float32), "smooth": dict(smooth=True),
              "counts": dict(band_dtype=np.float32, counts=True)}
    if case.symmetric:
        routes = {"block by block": dict(), "block by block float32": dict(band_dtype=np.float32)}
    reused = 0
    for md in (60, 200):
        for route, opt in routes.items():
            if route == "smooth" and md != 60:
                continue
            results = []
            for poisoned in (False, True):
                held = set()
                if poisoned:
                    before = dcool.stage_blocks([twin], md, sc.LARGEST, **opt)[0]
                    dcool.dev.sync()
                    filled = download_rows(dcool, before.sig32 if before.sig32 is not None else before.sig, n)
                    band_w = sc.geometry(md, n)[2]
                    cols = np.arange(n)[:, None] + np.arange(band_w)[None, :]
                    assert np.all(filled[:, :band_w][cols < n] != 0)               # the twin left no zero in the band
                    held = {int(p) for p in (before.sig.d_ptr, before.sig32.d_ptr if before.sig32 is not None else None) if p}
                    del before
                blk = dcool.stage_blocks([ci], md, sc.LARGEST, **opt)[0]
                if poisoned:
                    mine = {int(p) for p in (blk.sig.d_ptr, blk.sig32.d_ptr if blk.sig32 is not None else None) if p}
                    assert mine <= held, "the block did not take the buffers the twin released"
                    reused += len(mine)
                assert (blk.sig32 is not None) == (not case.symmetric)
                sig = blk.sig32 if opt.get("band_dtype") is np.float32 and blk.sig32 is not None else blk.sig
                rows = download_rows(dcool, sig, n)
                results.append(rows)
                band_w = sc.geometry(md, n)[2]
                if opt.get("counts"):
                    assert np.array_equal(rows, counts_rows(case, ci, band_w, int(sig.ld))), (route, md, poisoned)
                elif opt.get("band_dtype") is np.float32:
                    want = _want(case, ci, md)[0]
                    assert np.array_equal(rows == 0, want == 0) and np.abs(rows - want).max() <= 1e-11 + 2.0 ** -24 * 10, (route, md, poisoned)
                else:
                    check_values(case, ci, md, rows, tally, smooth=bool(opt.get("smooth")), band_w=band_w)
                    if blk.sig32 is not None:
                        assert np.array_equal(download_rows(dcool, blk.sig32, n), rows.astype(np.float32))
                del blk
            # (the law pass adds a group's pixels with LDS atomics: two stagings may differ in a law's last bit, so the two
            # results are each held to the oracle, not to one another)
            assert np.array_equal(results[0] == 0, results[1] == 0), (route, md)
    assert reused > 0
    tally.report()
    print(f"{name} / poisoned buffers: {reused} buffers taken over from the dense twin")


def test_trans_blocks_equal_the_host_built_block():
    """stage_inter and stage_inter_many against count * w1 * w2 over the block's median, NaN -> 0 (the median numpy's: of an
    even number of stored values the mean of the two middle ones; of none, NaN and an all-zero map): one division of the same
    operands, 1e-12 relative; zero pattern exact; the two entries bit for bit."""
    case = sc.trans_genome()
    dcool = pipeline.DeviceCool(case.cool)
    pairs = list(case.meta["pairs"])
    many = dcool.stage_inter_many(pairs)
    n_elem, worst = 0, 0.0
    for (ca, cb), blk in zip(pairs, many):
        want, med, stored = sc.trans_block(case.cool, ca, cb)
        n_r, n_c = want.shape
        got_med = dcool.inter_median(ca, cb)
        assert got_med == med or (np.isnan(got_med) and np.isnan(med)), (ca, cb, got_med, med)
        one = dcool.stage_inter(ca, cb, resident=True)
        a, b = download_rows(dcool, blk.sig, n_r), download_rows(dcool, one.sig, n_r)
        assert blk.shape == one.shape == (n_r, n_c) and blk.inter and one.inter
        assert blk.sig.layout == LAYOUT_DENSE and blk.sig.ld == (n_c + 15) // 16 * 16 == one.sig.ld
        assert np.array_equal(a, b), (ca, cb)
        assert not a[:, n_c:].any() and np.all(np.isfinite(a))
        got = a[:, :n_c]
        assert np.array_equal(got == 0, want == 0), (ca, cb)
        err = np.abs(got - want)
        assert np.all(err <= 1e-12 * np.abs(want)), (ca, cb, err.max())
        nz = want != 0
        worst = max(worst, float((err[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0)
        n_elem += a.size
        for flags, ch in ((blk.miss_row, ca), (blk.miss_col, cb)):
            s, e = int(case.offsets[ch]), int(case.offsets[ch + 1])
            assert np.array_equal(_d2h(dcool.dev, flags.ptr, (e - s,), np.uint8), np.isnan(case.cool["weight"][s:e]).astype(np.uint8))
    check_inputs(case, dcool)
    print(f"trans / stage_inter, stage_inter_many: {len(pairs)} blocks, {n_elem} elements compared, worst error {worst:.2e} relative, excluded: 0")


RECORDED = ("cs_csr_band_extent", "cs_csr_median", "cs_csr_median_many", "cs_memcpy_h2d", "cs_memcpy_d2h", "cs_distance_law_csr",
            "cs_distance_law_finish", "cs_csr_to_band", "cs_stage_blocks", "cs_stage_blocks_opt")


def test_staging_routes_issue_their_native_call_sequences(monkeypatch):
    """Which native entries every staging route calls, in order (plan.StepPlan replays recorded calls, and stage_inter_many
    exists for its synchronisation count): literal sequences, on `diagonals` at max_dist 60 -- chromosome 0 banded, 1 and 2
    staged dense.  Then a row strip against those rows of the unsplit trans block, and the width of a view_for view."""
    case = sc.get("diagonals")
    dcool = pipeline.DeviceCool(case.cool)
    md, big = 60, sc.LARGEST
    assert [pipeline.intra_geometry(case.n(ci), md, big).band for ci in range(3)] == [True, False, False] and dcool.upper
    log, lib = [], dcool.dev.lib

    def recorder(name, fn):
        def call(*args):
            log.append(name[3:])
            return fn(*args)
        return call

    for name in RECORDED:
        monkeypatch.setattr(lib, name, recorder(name, getattr(lib, name)))

    def calls(fn):
        del log[:]
        out = fn()
        return out, list(log)

    extent, median, to_band = "csr_band_extent", "csr_median", "csr_to_band"
    h2d, d2h = "memcpy_h2d", "memcpy_d2h"
    ca, cb, rows = 0, 1, (30, 90)
    whole, seq = calls(lambda: dcool.stage_inter(ca, cb, resident=True))
    assert seq == [extent, median, h2d, to_band]
    med, seq = calls(lambda: dcool.inter_median(ca, cb))
    assert seq == [extent, median] and med > 0
    _, seq = calls(lambda: dcool.stage_inter(ca, cb, rows=rows, largest_kernel=big, median=None))
    assert seq == [extent, median, extent, h2d, to_band]
    strip, seq = calls(lambda: dcool.stage_inter(ca, cb, rows=rows, largest_kernel=big, median=med))
    assert seq == [extent, h2d, to_band]
    many, seq = calls(lambda: dcool.stage_inter_many([(0, 1), (0, 2), (1, 2)]))
    assert seq == [extent] * 3 + ["csr_median_many", h2d] + [to_band] * 3 and len(many) == 3
    plain = [extent, "distance_law_csr", "distance_law_finish", to_band]
    fitted = [extent, "distance_law_csr", d2h, d2h, h2d, to_band]
    for ci in range(3):
        assert calls(lambda: dcool.stage_intra(ci, md, big))[1] == plain, ci
        assert case.n(ci) > 2 and calls(lambda: dcool.stage_intra(ci, md, big, smooth=True))[1] == fitted, ci
    part, seq = calls(lambda: dcool.stage_intra(0, md, big, rows=(50, 120), reduce=lambda x: x))
    assert seq == fitted and part.row_window == (50, 120)
    blocks, seq = calls(lambda: dcool.stage_blocks([0, 1, 2], md, big))
    assert seq == ["stage_blocks"] and all(b.shared is blocks[0].shared is not None for b in blocks)
    smoothed, seq = calls(lambda: dcool.stage_blocks([0, 1, 2], md, big, smooth=True))
    assert seq == ["stage_blocks_opt"] and all(b.smooth for b in smoothed) and not any(b.smooth for b in blocks)
    monkeypatch.undo()

    # a strip staged with the whole block's median holds those rows of the unsplit block, bit for bit, row0 respected
    n_r, n_c = whole.shape
    ra, rb = pipeline._strip_rows(n_r, rows, (big - 1) // 2)
    assert (ra, rb) == (22, 98) and strip.row_window == rows and strip.sig.row0 == ra == strip.view_row0 and strip.inter
    assert strip.shape == whole.shape and strip.sig.ld == whole.sig.ld == pipeline._inter_ld(n_c) and whole.sig.row0 == 0
    assert strip.strip_pool is not None and dcool.inter_high_water >= (rb - ra) * strip.sig.ld * 8 and strip.buffer is None
    got, want = download_rows(dcool, strip.sig, rb - ra), download_rows(dcool, whole.sig, n_r)
    assert want.any() and np.array_equal(got, want[ra:rb])
    assert np.array_equal(download_rows(dcool, many[0].sig, n_r), want)

    # a view of a banded block carries the band width the geometry gives for the shorter distance; a dense block has no view
    geo = pipeline.intra_geometry(case.n(0), 20, big)
    view = dcool.view_for(blocks[0], 20, big)
    assert geo.band and view.sig.band_w == geo.in_w == 38 and view.sig32.band_w == geo.in_w and view.keep == geo.keep
    assert view.sig.ld == blocks[0].sig.ld and view.sig.d_ptr == blocks[0].sig.d_ptr and view.parent is blocks[0] and view.buffer is None
    assert blocks[0].is_band and view.is_band and not blocks[1].is_band and not whole.is_band and not part.is_band
    assert dcool.view_for(blocks[1], 20, big) is None and dcool.view_for(smoothed[0], 20, big) is None
    assert dcool.view_for(blocks[0], md + 1, big) is None
    print(f"diagonals / call sequences: 9 routes as the parent's, strip of rows {ra}..{rb - 1} of {n_r} x {n_c} bit for bit, "
          f"view band_w {view.sig.band_w}")
