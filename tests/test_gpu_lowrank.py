"""--tsvd templates as rank-r separable passes (chromosight_amd/csrc/cs_corr_lowrank.hip, cs_last_kernel() == CS_KERNEL_LOWRANK):
maps and plain cross-correlations against the C oracle fed the same K' and Q', the golden tsvd captures again on the new kernel, the
default rule's routes, seeded sweeps (ranks, sizes, masks, band widths, n_obs), the candidate sink against the oracle's passing set,
and detect / quantify --tsvd tables identical to the full-template route."""
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
from oracle import pearson_oracle as orc
from parity_util import assert_parity

pytestmark = pytest.mark.gpu

KERNEL_LOWRANK = 10                  # include/chromosight_hip.h
TOL_LARGE = 2e-4                     # float32 sums of more than 33 x 33 terms (tests/test_gpu_large_templates.py)


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


@pytest.fixture
def lowrank(monkeypatch):
    monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", "1")


def last_kernel():
    dev = get_device()
    return dev.lib.cs_last_kernel(dev.ctx)


def worker_kernels():
    """cs_last_kernel() of the contexts pipeline.detect / quantify run their blocks on: the worker threads' own (pipeline._Workers)."""
    import threading
    import time
    seen = set()
    lock = threading.Lock()

    def probe(w):
        d = getattr(w.local, "dev", None)
        time.sleep(0.02)                         # (keeps every thread of the pool busy once)
        if d is not None:
            with lock:
                seen.add(d.lib.cs_last_kernel(d.ctx))
    for w in list(pipeline._WORKER_POOLS.values()):
        list(w.pool.map(lambda _: probe(w), range(8 * w.pool._max_workers)))
    return seen


def tsvd_pair(kernel, prop=0.999):
    u, v = cup.factorise_kernel(kernel.copy(), prop_info=prop)
    u2, v2 = cup.factorise_kernel(kernel ** 2, prop_info=prop)
    return u @ v, u2 @ v2, u.shape[1], u2.shape[1]


def preset(name, k=0):
    return np.asarray(getattr(ck, name)["kernels"][k], dtype=np.float64)


def low_rank_template(shape, rank, seed):
    rng = np.random.default_rng(seed)
    u, v = rng.normal(size=(shape[0], rank)), rng.normal(size=(rank, shape[1]))
    u[:, 0], v[0] = 1.0 + 0.3 * rng.normal(size=shape[0]), 2.0          # (a positive mean inside the rank)
    return u @ v


def cases():
    loops = preset("loops")
    out = [("loops", loops), ("borders0", preset("borders", 0)), ("stripes", preset("stripes_left"))]
    out += [(f"loops{s}", cup.resize_kernel(loops, factor=s / 17, quiet=True)) for s in (33, 41, 61)]
    out.append(("rank3_9x13", low_rank_template((9, 13), 3, 7)))
    return out


def _parity(got, want, cond, km, what, two_level, masked=False, ill=0.0):
    got = got.toarray() if sp.issparse(got) else np.asarray(got, dtype=np.float64)
    # (masked windows: float32 sums over the staged plane in another order than the tile kernels', up to 3.3e-5 measured at 17 .. 33)
    tol = (5e-5 if masked else 1e-5) if km <= 33 else TOL_LARGE
    # (windows whose present pixels of a 0 / 1 template are all equal: ill-defined in any order of additions)
    assert_parity(got, want, cond, "f32", what, tol=tol, max_ill_frac=0.3 if two_level else ill)


# ---------------------------------------------------------------------------------------------------------------------------
# maps against the oracle

@pytest.mark.parametrize("name,kern", cases(), ids=[c[0] for c in cases()])
@pytest.mark.parametrize("mode", ["dense", "dense_full", "bins_band"])
def test_maps_match_oracle(name, kern, mode, lowrank):
    km = kern.shape[0]
    kconv, ksq, _, _ = tsvd_pair(kern)
    two_level = len(np.unique(kern)) <= 2
    n = max(160, 3 * km)
    rng = np.random.default_rng(km + len(mode))
    if mode.startswith("dense"):
        sig = rng.gamma(2.0, 1.0, size=(n, n + 13)).astype(np.float32)
        full = mode == "dense_full"
        got, _ = cud.normxcorr2(sig, kern, full=full, tsvd=0.999)
        assert last_kernel() == KERNEL_LOWRANK
        want, _ = c_oracle.normxcorr2(sig.astype(np.float64), kern, full=full, kernel_conv=kconv, kernel_sq=ksq)
        cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), kern, 0, n, full=full)[1]
        _parity(got, want, cond, km, f"{name} {mode}", two_level)
        return
    md = 60
    ii, jj = np.indices((n, n))
    sig = np.triu(np.minimum(rng.gamma(20, 0.05, size=(n, n)), 10.0))
    sig[jj - ii > md + km] = 0
    miss = rng.random(n) < 0.05
    sig[miss, :] = 0
    sig[:, miss] = 0
    valid = np.flatnonzero(~miss)
    band = (jj - ii >= 0) & (jj - ii <= md)
    mask = cup.make_missing_mask((n, n), valid, valid, max_dist=md, sym_upper=True)
    s32 = sig.astype(np.float32)
    got, _ = cud.normxcorr2(sp.csr_matrix(s32), kern, max_dist=md, sym_upper=True, full=True, missing_mask=mask, tsvd=0.999)
    assert last_kernel() == KERNEL_LOWRANK
    kw = dict(max_dist=md, sym_upper=True, full=True, miss_row=miss, miss_col=miss)
    want, _ = c_oracle.normxcorr2(s32.astype(np.float64), kern, kernel_conv=kconv, kernel_sq=ksq, **kw)
    cond = c_oracle.normxcorr2_rows(s32.astype(np.float64), kern, 0, n, **kw)[1]
    _parity(got.toarray()[band], want[band], cond[band], km, f"{name} {mode}", two_level, masked=True)


@pytest.mark.parametrize("shape,rank", [((17, 17), 2), ((9, 13), 3), ((15, 11), 2), ((41, 41), 5)])
def test_xcorr2_matches_oracle(shape, rank, lowrank):
    """Plain cross-correlations: the factors of the weights as passed."""
    kern = low_rank_template(shape, rank, shape[0])
    rng = np.random.default_rng(shape[1])
    sig = rng.gamma(2.0, 1.0, size=(150, 170))
    got = cud.xcorr2(sig, kern, tsvd=0.999)
    assert last_kernel() == KERNEL_LOWRANK
    kconv, _, _, _ = tsvd_pair(kern)
    want = orc.xcorr2_oracle(sig, kconv, threshold=1e-4)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"xcorr2 {shape} rank {rank}: max relative err {err:.2e}")
    assert err < 2e-6


def test_switch_off_keeps_todays_route(monkeypatch):
    monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", "0")
    sig = np.random.default_rng(2).gamma(2.0, 1.0, size=(200, 200)).astype(np.float32)
    cud.normxcorr2(sig, preset("stripes_left"), tsvd=0.999)
    assert last_kernel() != KERNEL_LOWRANK
    cud.xcorr2(sig, preset("loops"), tsvd=0.999)
    assert last_kernel() != KERNEL_LOWRANK


def test_default_rule_routes(monkeypatch):
    """Without the switch (the rule measured in profiles/lowrank_time.json): loops at 41 and 61 on the new kernel; loops / borders
    at 17, loops_small at 7, stripes 31 and loops 33 on the matrix-core kernels, which are faster there; never without tsvd."""
    monkeypatch.delenv("CHROMOSIGHT_HIP_LOWRANK", raising=False)
    sig = np.random.default_rng(3).gamma(2.0, 1.0, size=(256, 256)).astype(np.float32)
    loops = preset("loops")
    for kern in (cup.resize_kernel(loops, factor=41 / 17, quiet=True), cup.resize_kernel(loops, factor=61 / 17, quiet=True)):
        cud.normxcorr2(sig, kern, tsvd=0.999)
        assert last_kernel() == KERNEL_LOWRANK
        cud.normxcorr2(sig, kern)
        assert last_kernel() != KERNEL_LOWRANK
    for kern in (loops, preset("borders"), preset("loops_small"), preset("stripes_left"), cup.resize_kernel(loops, factor=33 / 17, quiet=True)):
        cud.normxcorr2(sig, kern, tsvd=0.999)
        assert last_kernel() != KERNEL_LOWRANK


# ---------------------------------------------------------------------------------------------------------------------------
# the golden tsvd captures on the new kernel

def test_golden_xcorr2_and_normxcorr2_tsvd(golden, templates, lowrank):
    g = golden("xcorr2")
    t = cud.xcorr2(sp.csr_matrix(g["rand"]), templates["loops"], tsvd=0.999)
    assert last_kernel() == KERNEL_LOWRANK
    ref = g["rand_loops_tsvd999"]
    assert np.abs(t.toarray() - ref).max() < 2e-6 * np.abs(ref).max()
    g = golden("normxcorr2_dense")
    c, _ = cud.normxcorr2(sp.csr_matrix(g["sig_a"]), templates["loops"], full=True, tsvd=0.999)
    assert last_kernel() == KERNEL_LOWRANK
    assert np.abs(c.toarray() - g["sparse_a_loops_full_tsvd999_corr"]).max() < 1e-5


def test_golden_detect_tsvd_tables(golden, lowrank):
    """tests/golden/options.npz loops_tsvd_* / borders_tsvd_*: per-block raw tables of the reference, the candidates from the new
    kernel's sink."""
    g = golden("options")
    dcool = pipeline.DeviceCool(golden("example_cool"))
    total = 0
    for name in ("loops", "borders"):
        cfg = copy.deepcopy(getattr(ck, name))
        max_dist = max(cfg["max_dist"] // dcool.binsize, 1)
        kernels = [np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]
        largest = max(k.shape[0] for k in kernels)
        for ci in range(dcool.n_chrom):
            plain = dcool.stage_intra(ci, max_dist, largest, resident=True)
            for ki, kern in enumerate(kernels):
                want = g[f"{name}_tsvd_c{ci}_k{ki}"]
                tab, _ = pipeline.detect_block(dcool, plain, cfg, kern, tsvd=0.999, raw=True)
                assert dcool.dev.lib.cs_last_kernel(dcool.dev.ctx) == KERNEL_LOWRANK, (name, ci, ki)
                got = np.zeros((0, 4)) if tab is None else tab
                assert got.shape == want.shape, (name, ci, ki, got.shape, want.shape)
                if len(want):
                    assert np.array_equal(got[:, :2], want[:, :2]), (name, ci, ki)
                    assert np.abs(got[:, 2] - want[:, 2]).max() < 1e-9, (name, ci, ki)
                total += len(want)
    assert total > 200


# ---------------------------------------------------------------------------------------------------------------------------
# the candidate sink: detect / quantify --tsvd tables identical to the full-template route

def _same(a, b):
    import pandas as pd
    pd.testing.assert_frame_equal(a[0], b[0])
    # (windows: a few 1e-15 between two runs whatever the kernel, as in tests/test_gpu_large_templates.py)
    wa, wb = np.asarray(a[1], dtype=np.float64), np.asarray(b[1], dtype=np.float64)
    assert wa.shape == wb.shape and np.array_equal(np.isnan(wa), np.isnan(wb))
    assert np.allclose(wa, wb, rtol=0, atol=1e-12, equal_nan=True)


@pytest.fixture(scope="module")
def genome():
    from tools.synthetic_genome import make_cool
    return make_cool(total_bins=24_000, max_dist_bins=300, seed=5, largest_kernel=41)[0]


@pytest.mark.parametrize("name,switch,win", [("loops", "1", None), ("borders", "1", None), ("loops", None, 41)])
def test_detect_tables_equal_todays_route(genome, name, switch, win, monkeypatch):
    cfg = copy.deepcopy(getattr(ck, name))
    res = {}
    for route in (switch, "0"):
        if route is None:
            monkeypatch.delenv("CHROMOSIGHT_HIP_LOWRANK", raising=False)
        else:
            monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", route)
        dcool = pipeline.DeviceCool(genome)
        res[route] = pipeline.detect(dcool, cfg, tsvd=0.999, win_size=win, return_windows=True)
        if route != "0":
            assert KERNEL_LOWRANK in worker_kernels() | {last_kernel(), dcool.dev.lib.cs_last_kernel(dcool.dev.ctx)}
    _same(res[switch], res["0"])
    if win is None:
        assert len(res["0"][0]) > 0
    print(f"{name} win={win}: {len(res['0'][0])} patterns")


def test_yeast_quantify_equals_todays_route(golden, monkeypatch):
    cool = golden("yeast_cool")
    cfg = copy.deepcopy(ck.loops)
    dcool = pipeline.DeviceCool(cool)
    monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", "0")
    det = pipeline.detect(dcool, cfg, tsvd=0.999)
    pos = det[["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].copy()
    out = {}
    for route in ("1", "0"):
        monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", route)
        dq = pipeline.DeviceCool(cool)
        out[route] = pipeline.quantify(dq, pos, cfg, tsvd=0.999)
        if route == "1":
            assert KERNEL_LOWRANK in worker_kernels() | {last_kernel(), dq.dev.lib.cs_last_kernel(dq.dev.ctx)}
    _same(out["1"], out["0"])
    assert len(out["1"][0]) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# seeded sweeps: ranks 1 .. 8, sizes 3 .. 81 (odd, square or not; normxcorr2 takes odd sides only, xcorr2 even ones too), masks,
# band widths, n_obs, candidate lists

def test_random_sweep(lowrank):
    """Random templates of rank 1 .. 8 with sides of 3 .. 81 on dense maps with a constant offset (the cross term must not cancel
    against it): the new kernel wherever K' and Q' are of rank 8 or less, the C oracle's coefficients within the kernel tests'
    tolerances."""
    rng = np.random.default_rng(2026)
    served = 0
    for case in range(16):
        rank = 1 + case % 8
        km, kn = (int(x) * 2 + 1 for x in rng.integers(1, 41, size=2))
        kern = low_rank_template((km, kn), rank, 100 + case)
        kconv, ksq, r, r2 = tsvd_pair(kern)
        n = max(120, 2 * max(km, kn) + 20)
        a = 5.0 * (1.0 + 0.05 * rng.standard_normal((n, n)))
        i0, j0 = n // 2, n // 2
        a[i0 - km // 2:i0 + km // 2 + 1, j0 - kn // 2:j0 + kn // 2 + 1] += 0.25 * (kern - kern.mean()) / kern.std()
        a32 = a.astype(np.float32)
        c, _ = cud.normxcorr2(a32, kern, full=True, tsvd=0.999)
        on_kernel = r <= 8 and r2 <= 8
        assert (last_kernel() == KERNEL_LOWRANK) == on_kernel, (case, r, r2)
        want, _ = c_oracle.normxcorr2(a32.astype(np.float64), kern, kernel_conv=kconv, kernel_sq=ksq, full=True)
        cond = c_oracle.normxcorr2_rows(a32.astype(np.float64), kern, 0, n, full=True)[1]
        # (a signal at 5 +- 0.25: its variance is 1e-3 of its mean square, so every float32 kernel is held to the 81 x 81 bound here)
        assert_parity(c, want, cond, "f32", f"sweep {case} {km}x{kn} r={r},{r2}", tol=TOL_LARGE)
        served += on_kernel
        print(f"sweep {case}: {km}x{kn} rank {rank} -> {r}/{r2}, kernel {last_kernel()}")
    assert served >= 4


def _device_map(dev, a):
    from chromosight_amd._lib import CsMatrix, LAYOUT_DENSE, np_dtype_code
    d, ld = engine.to_device_map(dev, a)
    return d, ld, CsMatrix(d.ptr, np_dtype_code(a.dtype), LAYOUT_DENSE, ld, 0, 0)


@pytest.mark.parametrize("case", range(8))
def test_random_masked_sweep_nobs_and_candidates(case, monkeypatch):
    """Banded maps with per-bin masks (sym_upper, full, random max_dist): coefficients and n_obs of the new kernel against the C oracle,
    and the candidates of its sink, re-scored in float64, exactly the pixels whose float64 coefficient passes."""
    from chromosight_amd._lib import CS_F32, LAYOUT_DENSE, MASK_BINS, CsMatrix
    rng = np.random.default_rng(500 + case)
    rank = 1 + case % 3                          # (rank 4 templates have squares of rank 10 at 0.999: not low rank)
    km, kn = (int(x) * 2 + 1 for x in rng.integers(1, 31, size=2))
    kern = low_rank_template((km, kn), rank, 300 + case)
    kconv, ksq, r, r2 = tsvd_pair(kern)
    assert r <= 8 and r2 <= 8
    n = 2 * max(km, kn) + 120
    md = int(rng.integers(max(km, kn), n - max(km, kn)))
    ii, jj = np.indices((n, n))
    a = np.triu(np.minimum(rng.gamma(20, 0.05, size=(n, n)), 10.0))
    i0 = n // 2
    a[i0 - km // 2:i0 + km // 2 + 1, i0 + 5 - kn // 2:i0 + 5 + kn // 2 + 1] += 0.5 * (kern - kern.mean()) / kern.std()
    a[(jj - ii < 0) | (jj - ii > md + max(km, kn))] = 0
    miss = rng.random(n) < 0.05
    a[miss, :] = 0
    a[:, miss] = 0
    a32 = a.astype(np.float32)
    dev = get_device()
    d_sig, ld, sig = _device_map(dev, a32)
    d_out, d_nobs = dev.empty(n * ld, np.float32), dev.empty(n * ld, np.float32)
    out = CsMatrix(d_out.ptr, CS_F32, LAYOUT_DENSE, ld, 0, 0)
    nobs = CsMatrix(d_nobs.ptr, CS_F32, LAYOUT_DENSE, ld, 0, 0)
    fr = dev.to_device(miss.astype(np.uint8))
    spec = engine.KernelSpec(kern, 0.999)
    monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", "1")
    engine.run_normxcorr2(dev, sig, (n, n), spec, out, full=True, sym_upper=True, max_dist=md, mask_mode=MASK_BINS, miss_row=fr,
                          miss_col=fr, missing_tol=0.5, nobs=nobs, precision="f32")
    assert last_kernel() == KERNEL_LOWRANK
    got = d_out.download().reshape(n, ld)[:, :n].astype(np.float64)
    got_n = d_nobs.download().reshape(n, ld)[:, :n].astype(np.float64)
    kw = dict(max_dist=md, sym_upper=True, full=True, miss_row=miss, miss_col=miss, missing_tol=0.5)
    want, want_n = c_oracle.normxcorr2(a32.astype(np.float64), kern, kernel_conv=kconv, kernel_sq=ksq, **kw)
    cond = c_oracle.normxcorr2_rows(a32.astype(np.float64), kern, 0, n, **kw)[1]
    band = (jj - ii >= 0) & (jj - ii <= md)
    # (random templates with half a window missing: many windows whose present template pixels barely vary; as in
    # tests/test_gpu_large_templates.py the coefficients are held to the bound on the well-conditioned ones)
    well = band & (cond >= 1e-3)
    err = float(np.abs(got - want)[well].max())
    print(f"masked sweep {case} {km}x{kn} r={r},{r2} md={md}: max|err| {err:.2e} on {int(well.sum())} well-conditioned pixels")
    assert err < (5e-5 if max(km, kn) <= 33 else TOL_LARGE), (case, err)
    assert np.all(np.abs(got[band]) <= 1.0 + 1e-6)
    assert np.array_equal(got_n[band], want_n[band])
    # candidate sink: exactly the pixels whose float64 coefficient (C oracle, float64 signal) passes
    a64 = a32.astype(np.float64)
    d64, ld64, sig64 = _device_map(dev, a64)
    rows, cols, vals = engine.run_candidates(dev, sig64, (n, n), spec, (0, n), pearson=0.3, lo_diag=0, hi_diag=md, inter=False, full=True,
                                             sym_upper=True, max_dist=md, mask_mode=MASK_BINS, miss_row=fr, miss_col=fr, missing_tol=0.5)
    assert last_kernel() == KERNEL_LOWRANK
    gotc = np.zeros((n, n), dtype=bool)
    gotc[rows, cols] = True
    exp = band & (want >= 0.3) & (want != 0)
    edge = np.abs(want - 0.3) < 1e-9
    assert np.array_equal(gotc & ~edge, exp & ~edge), (case, int(gotc.sum()), int(exp.sum()))
    if rows.size:
        assert np.abs(vals - want[rows, cols]).max() < 1e-7
    print(f"masked sweep {case}: {km}x{kn} rank {rank} -> {r}/{r2}, md {md}: {rows.size} candidates")


@pytest.mark.parametrize("shape", [(8, 10), (12, 7), (40, 34)])
def test_xcorr2_even_sizes_equal_the_runtime_size_kernel(shape, monkeypatch):
    """Even sides (xcorr2 takes them): the new kernel against the runtime-size kernel on the same weights."""
    kern = low_rank_template(shape, 2, sum(shape))
    sig = np.random.default_rng(shape[0]).gamma(2.0, 1.0, size=(150, 170))
    res = {}
    for route in ("1", "0"):
        monkeypatch.setenv("CHROMOSIGHT_HIP_LOWRANK", route)
        res[route] = cud.xcorr2(sig, kern, tsvd=0.999)
        assert (last_kernel() == KERNEL_LOWRANK) == (route == "1"), route
    assert res["1"].shape == res["0"].shape
    assert np.abs(res["1"] - res["0"]).max() < 2e-6 * np.abs(res["0"]).max()


@pytest.mark.parametrize("pearson", [0.5, 0.15])
def test_the_screen_loses_no_passing_pixel(pearson, lowrank):
    """Plateau maps (value 5 +- a few 1e-3) carrying faint copies of loops resized to 41 (tsvd 0.999): float64 coefficients straddle
    pearson while float32 sums evaluate them with large relative errors.  The candidates of the new kernel's sink, re-scored in float64,
    are exactly the pixels whose float64 coefficient (C oracle, K' and Q') passes."""
    from chromosight_amd._lib import MASK_BINS
    kern = cup.resize_kernel(preset("loops"), factor=41 / 17, quiet=True)
    kconv, ksq, _, _ = tsvd_pair(kern)
    kz = (kern - kern.mean()) / kern.std()
    n, md = 300, 200
    ii, jj = np.indices((n, n))
    dev = get_device()
    passing = 0
    for amp in (0.2, 0.5, 0.9, 1.5):
        rng = np.random.default_rng(int(amp * 100))
        a = 5.0 * (1.0 + 2e-3 * rng.standard_normal((n, n)))
        for i0, j0 in ((100, 150), (200, 260)):
            a[i0 - 20:i0 + 21, j0 - 20:j0 + 21] += 5.0 * 2e-3 * amp * kz
        a[(jj - ii < 0) | (jj - ii > md + 41)] = 0
        miss = np.zeros(n, bool)
        miss[rng.choice(n, size=6, replace=False)] = True
        a[miss, :] = 0
        a[:, miss] = 0
        want, _ = c_oracle.normxcorr2(a, kern, kernel_conv=kconv, kernel_sq=ksq, max_dist=md, sym_upper=True, full=True, miss_row=miss,
                                      miss_col=miss, missing_tol=0.5)
        d_sig, ld, sig = _device_map(dev, a)
        fr = dev.to_device(miss.astype(np.uint8))
        rows, cols, vals = engine.run_candidates(dev, sig, (n, n), engine.KernelSpec(kern, 0.999), (0, n), pearson=pearson, lo_diag=0,
                                                 hi_diag=md, inter=False, full=True, sym_upper=True, max_dist=md, mask_mode=MASK_BINS,
                                                 miss_row=fr, miss_col=fr, missing_tol=0.5)
        assert last_kernel() == KERNEL_LOWRANK
        got = np.zeros((n, n), dtype=bool)
        got[rows, cols] = True
        exp = (want >= pearson) & (want != 0) & (jj - ii >= 0) & (jj - ii <= md)
        edge = np.abs(want - pearson) < 1e-9
        assert np.array_equal(got & ~edge, exp & ~edge), (amp, int(got.sum()), int(exp.sum()))
        if rows.size:
            assert np.abs(vals - want[rows, cols]).max() < 1e-7
        passing += int(exp.sum())
        print(f"amp {amp} pearson {pearson}: {int(exp.sum())} passing pixels")
    assert passing > 0
