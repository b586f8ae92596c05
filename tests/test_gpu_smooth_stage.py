"""--smooth-trend in the one-call staging: cs_stage_blocks_opt(CS_STAGE_SMOOTH) fits every block's distance law on the device
(stage_smooth_kernel, csrc/cs_stage.hip) between the laws' finish and the detrend / tiler pass.

Yardsticks, all committed before this path existed: the host fit utils/preprocessing._isotonic_non_increasing (pinned to
scikit-learn at 1e-12 by the CPU suite), the reference's own `detect --smooth-trend` tables (tests/golden/options.npz), and the
block-by-block staging DeviceCool.stage_intra(smooth=True) with its host fit, which this path does not touch.

Every map of the pipeline tests must have a law the fit really changes: each asserts that at least 10 % of the kept diagonals
of one block differ between the unsmoothed law and its fit (`assert_fit_matters`)."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd import parallel, pipeline
from chromosight_amd._lib import LAYOUT_BAND, LAYOUT_BAND_COUNTS
from chromosight_amd.utils.preprocessing import _isotonic_non_increasing
from tools.synthetic_genome import make_cool

pytestmark = pytest.mark.gpu

RTOL_FIT = 1e-12          # the project's bound for this fit (a float64 mean of at most 4096 terms is good to ~4.5e-13)


def d2h(dcool, ptr, count, dtype=np.float64):
    out = np.empty(count, dtype=dtype)
    dcool.dev.sync()
    dcool.dev._check(dcool.dev.lib.cs_memcpy_d2h(dcool.dev.ctx, out.ctypes.data, ptr, out.nbytes, None))
    return out


def law_of(dcool, block):
    return d2h(dcool, block.d_law, block.n_diags)


def download_block(dcool, block):
    """Staged float64 block -> dense numpy."""
    n, sig = block.shape[0], block.sig
    host = d2h(dcool, sig.d_ptr, n * sig.ld).reshape(n, sig.ld)
    if sig.layout in (LAYOUT_BAND, 3):
        out = np.zeros((n, n))
        for d in range(sig.band_w):
            idx = np.arange(0, n - d)
            out[idx, idx + d] = host[idx, d]
        return out
    return host[:, :n].copy()


def one_call(blocks):
    """The blocks came from ONE native staging call: they hold the same law buffer (a block of the block-by-block path has none)."""
    shared = {id(b.shared) for b in blocks}
    return len(shared) == 1 and blocks[0].shared is not None


def assert_fit_matters(dcool, chroms, max_dist, largest):
    """At least 10 % of the kept diagonals of at least one block change under the fit (else a test of the smoothed path
    would pass on the unsmoothed one)."""
    best = 0.0
    for blk in dcool.stage_blocks(chroms, max_dist, largest):
        law = law_of(dcool, blk)
        if blk.shape[0] > 2:
            best = max(best, float(np.mean(_isotonic_non_increasing(law) != law)))
    assert best >= 0.10, best
    return best


def cool_of_laws(laws, integer=False):
    """A pixel table whose chromosome c has the distance law laws[c] when every diagonal is kept: one stored pixel (0, d) per
    non-empty diagonal, weights 1."""
    sizes = [len(law) for law in laws]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    b1, b2, cnt = [], [], []
    for c, law in enumerate(laws):
        d = np.nonzero(np.asarray(law) > 0)[0]
        b1.append(np.full(d.size, off[c]))
        b2.append(off[c] + d)
        cnt.append(np.asarray(law)[d])
    cnt = np.concatenate(cnt)
    return {"binsize": 1000, "chrom_offset": off, "chrom_names": np.asarray([f"c{i}" for i in range(len(sizes))]),
            "bin1_id": np.concatenate(b1).astype(np.int64), "bin2_id": np.concatenate(b2).astype(np.int64),
            "count": cnt.astype(np.int64) if integer else cnt, "weight": np.ones(int(off[-1]))}


def make_laws(rng, n):
    noisy = rng.random(n) * np.linspace(3.0, 0.05, n) ** 2 + 1e-3
    monotone = np.sort(noisy)[::-1].copy()
    increasing = np.sort(noisy + np.arange(n) * 1e-6).copy()
    holes = noisy.copy()
    holes[rng.random(n) < 0.2] = 0.0
    holes[n - max(n // 5, 1):] = 0.0
    if n > 4:
        holes[n // 2] = 0.0
    return {"noisy": noisy, "monotone": monotone, "increasing": increasing, "holes": holes}


SIZES = (3, 63, 64, 65, 1000, 4095, 4096)


def test_device_fit_equals_the_host_fit_on_random_laws():
    """Random laws of 3 ... 4096 diagonals -- noisy, already monotone (unchanged bit for bit), strictly increasing (one pool),
    with empty diagonals in the middle and at the end -- and a block of 2 bins (untouched): the device fit == the host fit of
    the unsmoothed device law to rtol 1e-12; a second run gives the same bits."""
    rng = np.random.default_rng(20)
    laws, kinds = [], []
    for n in SIZES:
        for kind, law in make_laws(rng, n).items():
            laws.append(law)
            kinds.append((n, kind))
    laws.append(np.array([1.0, 5.0]))                        # n <= 2: the reference does not fit it
    kinds.append((2, "two bins"))
    dcool = pipeline.DeviceCool(cool_of_laws(laws))
    chroms = list(range(len(laws)))
    plain = [law_of(dcool, b) for b in dcool.stage_blocks(chroms, 4096, 1)]
    for law, got in zip(laws, plain):
        assert np.array_equal(got, law)                      # (the construction: the staged law IS the given one)
    runs = []
    for _ in range(2):
        blocks = dcool.stage_blocks(chroms, 4096, 1, smooth=True)
        assert one_call(blocks) and all(b.smooth for b in blocks)
        runs.append([law_of(dcool, b) for b in blocks])
    for (n, kind), law, got, again in zip(kinds, plain, runs[0], runs[1]):
        assert got.shape == (n,)
        assert np.array_equal(got, again), (n, kind)
        if n <= 2:
            assert np.array_equal(got, law)
            continue
        want = _isotonic_non_increasing(law)
        print(f"n_diags {n:5d} {kind:10s}: {int(np.sum(want != law)):5d} entries change, max rel err "
              f"{np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)):.3g}")
        assert np.allclose(got, want, rtol=RTOL_FIT, atol=0.0), (n, kind)
        assert np.all(np.diff(got) <= 0), (n, kind)
        if kind == "monotone":
            assert np.array_equal(got, law), n
        if kind == "increasing":
            assert np.all(got == got[0]), n
        if kind in ("noisy", "holes") and n >= 63:
            assert np.mean(want != law) > 0.5
    # the unsmoothed staging after a smoothed one on the same tables: what it was before
    for law, blk in zip(plain, dcool.stage_blocks(chroms, 4096, 1)):
        assert np.array_equal(law_of(dcool, blk), law)


@pytest.mark.parametrize("n_diags", [3, 64, 1000, 4096])
def test_device_fit_rewrites_the_reciprocals_of_a_counts_band(n_diags):
    """Blocks staged as bands of raw counts keep 1 / law in float64 and float32 behind the law (what their readers multiply
    with): after the fit they are the reciprocals of the FITTED law, bit for bit what the finish pass derives from a law."""
    rng = np.random.default_rng(n_diags)
    n = 2 * n_diags + 12
    laws = []
    for holes in (False, True):
        law = np.zeros(n)
        law[:n_diags] = rng.integers(1, 2000, n_diags)
        if holes:
            law[:n_diags][rng.random(n_diags) < 0.2] = 0
            law[n_diags - max(n_diags // 5, 1):n_diags] = 0
        laws.append(law)
    dcool = pipeline.DeviceCool(cool_of_laws(laws, integer=True))
    assert dcool.counts_ok
    max_dist, largest = (n_diags - 2, 1) if n_diags > 3 else (1, 1)
    plain = dcool.stage_blocks([0, 1], max_dist, largest, band_dtype=np.float32, counts=True)
    unsmoothed = [law_of(dcool, b) for b in plain]
    runs = []
    for _ in range(2):
        blocks = dcool.stage_blocks([0, 1], max_dist, largest, band_dtype=np.float32, counts=True, smooth=True)
        assert one_call(blocks)
        out = []
        for blk in blocks:
            assert blk.sig32.layout == LAYOUT_BAND_COUNTS and blk.n_diags == n_diags
            f64 = d2h(dcool, blk.d_law, 2 * n_diags + 2)
            f32 = d2h(dcool, blk.d_law + 8 * (2 * n_diags + 2), n_diags + 2, np.float32)
            out.append((f64[:n_diags], f64[n_diags + 1:2 * n_diags + 1], f32[1:n_diags + 1]))
        runs.append(out)
    for c in range(2):
        assert np.array_equal(unsmoothed[c], laws[c][:n_diags])
        law, rlaw, rlaw32 = runs[0][c]
        want = _isotonic_non_increasing(unsmoothed[c])
        assert np.allclose(law, want, rtol=RTOL_FIT, atol=0.0)
        if n_diags >= 64:
            assert np.mean(want != unsmoothed[c]) > 0.3
        with np.errstate(divide="ignore"):
            assert np.array_equal(rlaw, 1.0 / law)
            assert np.array_equal(rlaw32, (1.0 / law).astype(np.float32))
        for a, b in zip(runs[0][c], runs[1][c]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_one_call_smoothed_staging_matches_the_reference_capture(golden, precision):
    """DeviceCool.stage_blocks([0, 1, 2], ..., smooth=True) on the example map, loops and the three borders templates: the
    per-block raw tables of the reference's own `detect --smooth-trend` (tests/golden/options.npz) under the bar of
    test_smooth_trend_and_tsvd_match_reference -- same rows in the same order, scores within 1e-9 -- from blocks of ONE native
    staging call."""
    g = golden("options")
    dcool = pipeline.DeviceCool(golden("example_cool"))
    chromosight_amd.set_precision(precision)
    try:
        total = 0
        for name in ("loops", "borders"):
            cfg = copy.deepcopy(getattr(ck, name))
            max_dist = max(cfg["max_dist"] // dcool.binsize, 1)
            kernels = [np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]
            largest = max(k.shape[0] for k in kernels)
            if name == "loops":
                assert_fit_matters(dcool, [0, 1, 2], max_dist, largest)
            blocks = dcool.stage_blocks([0, 1, 2], max_dist, largest, smooth=True)
            assert one_call(blocks), "the one-call staging did not take smooth=True"
            assert all(b.smooth for b in blocks)
            for ci, blk in enumerate(blocks):
                # ... and the maps themselves against the block-by-block path with its host fit
                slow = download_block(dcool, dcool.stage_intra(ci, max_dist, largest, smooth=True))
                fast = download_block(dcool, blk)
                assert np.abs(fast - slow).max() <= 1e-11 * max(np.abs(slow).max(), 1.0), (name, ci)
                for ki, kern in enumerate(kernels):
                    want = g[f"{name}_smooth_c{ci}_k{ki}"]
                    tab, _ = pipeline.detect_block(dcool, blk, cfg, kern, raw=True)
                    got = np.zeros((0, 4)) if tab is None else tab
                    assert got.shape == want.shape, (name, ci, ki, got.shape, want.shape)
                    if len(want):
                        assert np.array_equal(got[:, :2], want[:, :2]), (name, ci, ki)
                        assert np.abs(got[:, 2] - want[:, 2]).max() < 1e-9, (name, ci, ki)
                    total += len(want)
        assert total > 200
    finally:
        chromosight_amd.set_precision("f32")


def block_by_block_detect(dcool, cfg):
    """`detect --smooth-trend` built from stage_intra(smooth=True) (host fit) + detect_block, assembled like pipeline.detect."""
    max_dist = max(cfg["max_dist"] // dcool.binsize, 1)
    kernels = [np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]
    largest = max(k.shape[0] for k in kernels)
    blocks = [dcool.stage_intra(ci, max_dist, largest, smooth=True, resident=True) for ci in range(dcool.n_chrom)]
    cols = {k: [] for k in ("bin1", "bin2", "score", "pvalue", "kernel_id", "iteration")}
    for ki, kern in enumerate(kernels):
        for ci, blk in enumerate(blocks):
            tab, _ = pipeline.detect_block(dcool, blk, cfg, kern, raw=True, want_windows=False)
            if tab is None or not len(tab):
                continue
            first = int(dcool.offsets[ci])
            cols["bin1"].append(tab[:, 0].astype(np.int64) + first)
            cols["bin2"].append(tab[:, 1].astype(np.int64) + first)
            cols["score"].append(tab[:, 2])
            cols["pvalue"].append(tab[:, 3])
            cols["kernel_id"].append(np.full(len(tab), ki, dtype=np.int64))
            cols["iteration"].append(np.zeros(len(tab), dtype=np.int64))
    coords = {k: np.concatenate(v) for k, v in cols.items()}
    return pipeline.postprocess(coords, cfg, dcool.binsize, dcool.offsets, dcool.names, dcool.bin_start, dcool.bin_end)


def assert_same_table(got, want, what):
    assert len(got) == len(want) and len(want) > 0, (what, len(got), len(want))
    for col in ("chrom1", "start1", "chrom2", "start2", "bin1", "bin2", "kernel_id"):
        assert np.array_equal(np.asarray(got[col]), np.asarray(want[col])), (what, col)
    assert np.abs(np.asarray(got["score"], dtype=float) - np.asarray(want["score"], dtype=float)).max() < 1e-9, what


def loops_at(max_dist_bins, binsize):
    cfg = copy.deepcopy(ck.loops)
    cfg["max_dist"] = max_dist_bins * binsize
    return cfg


@pytest.fixture(scope="module")
def genome():
    cool, _ = make_cool(20_000, 1000, 2000, seed=2, template=np.asarray(ck.loops["kernels"][0], dtype=np.float64))
    return cool


@pytest.mark.parametrize("max_dist_bins", [1000, 300, 120])
def test_detect_smooth_through_genome_step_equals_block_by_block(genome, max_dist_bins):
    """pipeline.detect(smooth=True) on a 23-chromosome genome of 300 ... 1640 bins -- every block staged dense (1000), dense and
    banded (300), every block banded (120: the step is replayed as one native call list) -- first call and repeats == the run
    built from stage_intra(smooth=True) + detect_block: the same rows in order, scores within 1e-9."""
    dcool = pipeline.DeviceCool(genome)
    cfg = loops_at(max_dist_bins, dcool.binsize)
    assert_fit_matters(dcool, range(dcool.n_chrom), max_dist_bins, 17)
    want = block_by_block_detect(dcool, cfg)
    plain = pipeline.detect(dcool, cfg)
    for step in range(3):
        assert_same_table(pipeline.detect(dcool, cfg, smooth=True), want, (max_dist_bins, step))
    plans = [p for key, p in dcool.__dict__.get("_step_plans", {}).items() if key[1] is True]
    assert len(plans) == 1
    if max_dist_bins == 120:
        assert plans[0].ok, plans[0].why                     # (steps 1 and 2 above were replays of the recorded list)
    # the smoothed and the plain run are different runs (else the comparison above shows nothing), and stay apart
    assert len(plain) != len(want) or not np.allclose(np.asarray(plain["score"], float), np.asarray(want["score"], float), atol=1e-9)
    again = pipeline.detect(dcool, cfg)
    assert_same_table(again, plain, "plain after smoothed")


def test_detect_smooth_falls_back_for_a_law_beyond_4096_diagonals():
    """A chromosome whose keep distance gives more than 4096 diagonals: the one-call staging declines, every block takes the
    block-by-block path with the host fit, and detect(smooth=True) is still the block-by-block result."""
    cool, _ = make_cool(10_000, 4_200, 2000, seed=7, chrom_sizes=[9_000, 600, 400],
                        template=np.asarray(ck.loops["kernels"][0], dtype=np.float64))
    dcool = pipeline.DeviceCool(cool)
    cfg = loops_at(4_200, dcool.binsize)
    blocks = dcool.stage_blocks([0, 1, 2], 4_200, 17, smooth=True)
    assert not one_call(blocks) and all(b.smooth for b in blocks)
    law = d2h(dcool, dcool.stage_blocks([1], 4_200, 17)[0].d_law, 600)
    assert np.mean(_isotonic_non_increasing(law) != law) >= 0.10
    del blocks
    assert_same_table(pipeline.detect(dcool, cfg, smooth=True), block_by_block_detect(dcool, cfg), "long law")


def test_quantify_smooth_equals_block_by_block(genome, monkeypatch):
    """pipeline.quantify(smooth=True): its intra blocks now come from the one-call staging; the scores are those of the
    block-by-block staging with the host fit (the one-call path switched off)."""
    dcool = pipeline.DeviceCool(genome)
    cfg = loops_at(300, dcool.binsize)
    assert_fit_matters(dcool, range(dcool.n_chrom), 300, 17)
    found = pipeline.detect(dcool, cfg, smooth=True)
    assert len(found) > 10
    positions = found.iloc[::3][["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].reset_index(drop=True)
    calls = []
    real = pipeline.DeviceCool._stage_fast

    def counting(self, *args, **kw):
        out = real(self, *args, **kw)
        calls.append((bool(kw.get("smooth")), out is not None))
        return out

    monkeypatch.setattr(pipeline.DeviceCool, "_stage_fast", counting)
    got, got_win = pipeline.quantify(dcool, positions, cfg, smooth=True)
    assert calls and all(c == (True, True) for c in calls), calls
    monkeypatch.setattr(pipeline.DeviceCool, "_stage_fast", lambda self, *a, **k: None)
    want, want_win = pipeline.quantify(dcool, positions, cfg, smooth=True)
    monkeypatch.setattr(pipeline.DeviceCool, "_stage_fast", real)
    plain, _ = pipeline.quantify(dcool, positions, cfg)
    assert len(got) == len(want) == len(positions) and list(got.columns) == list(want.columns)
    for col in ("chrom1", "start1", "chrom2", "start2"):
        assert np.array_equal(np.asarray(got[col]), np.asarray(want[col])), col
    a, b = np.asarray(got["score"], float), np.asarray(want["score"], float)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.nanmax(np.abs(a - b)) < 1e-9
    assert np.allclose(np.asarray(got_win), np.asarray(want_win), rtol=0, atol=1e-9, equal_nan=True)
    assert np.nanmax(np.abs(a - np.asarray(plain["score"], float))) > 1e-6      # (smoothing changed the scores)


def test_two_patterns_smoothed_equal_the_patterns_run_separately(genome):
    """A smoothed step of loops + borders (keep distances 317 and 18): a fitted law depends on how many diagonals were fitted,
    so no smoothed block may serve as a band view at another keep distance -- the pair == each pattern on its own, and ==
    the block-by-block run."""
    dcool = pipeline.DeviceCool(genome)
    loops, borders = loops_at(300, dcool.binsize), copy.deepcopy(ck.borders)
    assert_fit_matters(dcool, range(dcool.n_chrom), 300, 17)
    wide = dcool.stage_blocks([0], 300, 17, smooth=True)[0]
    assert dcool.view_for(wide, 1, 17) is None and dcool.view_for(dcool.stage_blocks([0], 300, 17)[0], 1, 17) is not None
    for step in range(2):
        rec_l, rec_b = parallel.genome_step(dcool, [loops, borders], local=True, smooth=True)
        one_l = parallel.genome_step(dcool, [loops], local=True, smooth=True)[0]
        one_b = parallel.genome_step(dcool, [borders], local=True, smooth=True)[0]
        for name, pair, alone in (("loops", rec_l, one_l), ("borders", rec_b, one_b)):
            assert pair.shape == alone.shape and alone.shape[0] > 10, (name, step)
            assert np.array_equal(pair[:, [0, 1, 2, 5, 6]], alone[:, [0, 1, 2, 5, 6]]), (name, step)
            assert np.abs(pair[:, 3] - alone[:, 3]).max() < 1e-9, (name, step)
    for cfg, rec in ((loops, rec_l), (borders, rec_b)):
        want = block_by_block_detect(dcool, cfg)
        first = np.asarray(dcool.offsets, dtype=np.int64)[rec[:, 0].astype(np.int64)]
        coords = {"bin1": rec[:, 1].astype(np.int64) + first, "bin2": rec[:, 2].astype(np.int64) + first, "score": rec[:, 3],
                  "pvalue": rec[:, 4], "kernel_id": rec[:, 5].astype(np.int64), "iteration": rec[:, 6].astype(np.int64)}
        got = pipeline.postprocess(coords, cfg, dcool.binsize, dcool.offsets, dcool.names, dcool.bin_start, dcool.bin_end)
        assert_same_table(got, want, cfg["max_dist"])


WORKER = r"""
import os, sys, copy, numpy as np
sys.path.insert(0, os.environ["CS_ROOT"])
import torch.distributed as dist
import chromosight_amd.kernels as ck
from chromosight_amd import parallel, pipeline
from tools.synthetic_genome import make_cool
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
cool, _ = make_cool(20_000, 1000, 2000, seed=2, template=np.asarray(ck.loops["kernels"][0], dtype=np.float64))
dcool = pipeline.DeviceCool(cool)
cfg = copy.deepcopy(ck.loops); cfg["max_dist"] = 300 * 2000
taken = []
real = pipeline.DeviceCool._stage_fast
def counting(self, *a, **k):
    out = real(self, *a, **k)
    taken.append((bool(k.get("smooth")), out is not None))
    return out
pipeline.DeviceCool._stage_fast = counting
rec = parallel.detect_genome(dcool, cfg, smooth=True)
assert taken and all(t == (True, True) for t in taken), taken
if dist.get_rank() == 0:
    np.save(os.environ["CS_OUT"], rec)
dist.destroy_process_group()
"""


def test_detect_genome_smooth_on_two_ranks_equals_block_by_block(genome, tmp_path, monkeypatch):
    """parallel.detect_genome(smooth=True) on 2 ranks (gloo rendezvous, both on this GPU), each rank's blocks from the one-call
    staging == the single process on the block-by-block staging with the host fit."""
    dcool = pipeline.DeviceCool(genome)
    cfg = loops_at(300, dcool.binsize)
    assert_fit_matters(dcool, range(dcool.n_chrom), 300, 17)
    monkeypatch.setattr(pipeline.DeviceCool, "_stage_fast", lambda self, *a, **k: None)
    single = parallel.detect_genome(dcool, cfg, smooth=True)
    monkeypatch.undo()
    assert single.shape[0] > 10
    out = tmp_path / "rec.npy"
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CS_ROOT=root, CS_OUT=str(out), CHROMOSIGHT_HIP_DEVICE="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29557", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0")) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    both = np.load(out)
    assert both.shape == single.shape
    assert np.array_equal(both[:, [0, 1, 2, 5, 6]], single[:, [0, 1, 2, 5, 6]])
    assert np.abs(both[:, 3] - single[:, 3]).max() < 1e-9


def test_unsmoothed_staging_is_what_it_was(golden):
    """stage_blocks(smooth=False) -- before and after smoothed stagings on the same context -- against the block-by-block
    kernels this change does not touch, as the existing staging tests compare (bands equal up to the summation order of the
    law, 1e-13 relative, the same zero pattern), and against itself under the same bar (the law pass adds a diagonal's pixels
    in the order its waves arrive)."""
    dcool = pipeline.DeviceCool(golden("example_cool"))
    chroms = [0, 1, 2]
    for max_dist in (2000, 60):
        before = [(download_block(dcool, b), law_of(dcool, b)) for b in dcool.stage_blocks(chroms, max_dist, 17)]
        smoothed = dcool.stage_blocks(chroms, max_dist, 17, smooth=True)
        assert one_call(smoothed)
        after = dcool.stage_blocks(chroms, max_dist, 17)
        assert not any(b.smooth for b in after)
        for ci, ((band0, law0), blk) in enumerate(zip(before, after)):
            band1 = download_block(dcool, blk)
            assert np.abs(band1 - band0).max() <= 1e-13 * np.abs(band0).max() and np.array_equal(band1 == 0, band0 == 0)
            assert np.allclose(law_of(dcool, blk), law0, rtol=1e-13, atol=0.0)
            slow = download_block(dcool, dcool.stage_intra(ci, max_dist, 17))
            assert np.abs(band0 - slow).max() <= 1e-13 * max(np.abs(slow).max(), 1e-300), (max_dist, ci)
            assert np.array_equal(band0 == 0, slow == 0)
            if max_dist == 2000:
                assert not np.array_equal(download_block(dcool, smoothed[ci]), band0)
