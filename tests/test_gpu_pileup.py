"""The pileup of `detect --iterations` reduced on the device (cs_pileup_blocks, pipeline.pileup_blocks,
parallel.detect_genome): (1) bit for bit the documented summation order (tests/pileup_util.py) applied to the windows the
quantify chain returns for the same pixels -- every staging layout, templates of 7 x 7 .. 81 x 81 and a non-square one, list
lengths around the chunk size; (2) against the windows of the CPU oracle; (3) detect_genome with two iterations: the device
route == the host route (CHROMOSIGHT_HIP_HOST_PILEUP=1), its second iteration == the oracle pipeline run with the template
rebuilt from the first one's records, and no call asks for windows."""
import copy

import numpy as np
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import engine, parallel, pipeline
from chromosight_amd._lib import CS_F64, LAYOUT_BAND, LAYOUT_BAND_LAZY, LAYOUT_DENSE, CsMatrix
from chromosight_amd.utils import detection as cid
from tools.synthetic_genome import make_cool

import quantify_oracle_util as qo
from pileup_util import oracle_block_tables, restated_pileup, sum_bound

pytestmark = pytest.mark.gpu

BINSIZE = 2000
MD = 60                                     # max_dist, bins
SIZES_A = [150, 90, 40, 12]                 # the 40- and 12-bin blocks are staged dense
SIZES_B = [400, 150, 36]
LOOPS_PER_10K = 1500                        # planted loops: a few dozen on these few hundred bins
LOOPS = np.asarray(ck.loops["kernels"][0], dtype=np.float64)


def with_trans_pixels(cool, ca, cb, seed):
    """The decoded .cool with random contacts between chromosomes ca < cb added (make_cool writes intra pixels only)."""
    off = cool["chrom_offset"]
    rng = np.random.default_rng(seed)
    n_r, n_c = int(off[ca + 1] - off[ca]), int(off[cb + 1] - off[cb])
    keep = rng.random((n_r, n_c)) < 0.4
    r, c = np.nonzero(keep)
    b1 = np.concatenate([cool["bin1_id"], r + off[ca]])
    b2 = np.concatenate([cool["bin2_id"], c + off[cb]])
    cnt = np.concatenate([cool["count"], rng.integers(1, 9, size=r.size).astype(np.int32)])
    order = np.lexsort((b2, b1))
    return dict(cool, bin1_id=b1[order], bin2_id=b2[order], count=cnt[order])


@pytest.fixture(scope="module")
def genome_a():
    cool, _ = make_cool(sum(SIZES_A), MD, BINSIZE, seed=41, template=LOOPS, chrom_sizes=SIZES_A, loops_per_10k=LOOPS_PER_10K)
    cool = with_trans_pixels(cool, 0, 1, 42)
    return cool, pipeline.DeviceCool(cool)


@pytest.fixture(scope="module")
def genome_b():
    cool, _ = make_cool(sum(SIZES_B), 150, BINSIZE, seed=43, template=LOOPS, chrom_sizes=SIZES_B, loops_per_10k=LOOPS_PER_10K)
    return cool, pipeline.DeviceCool(cool)


def pixel_list(dcool, chroms, blocks, n, rng):
    """n pixels over the blocks, with repeats: inside the map, windows that leave it, on and next to the main diagonal, on
    missing rows."""
    blk = rng.integers(0, len(blocks), size=n)
    rows, cols = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for t in range(n):
        b = blocks[blk[t]]
        n_r, n_c = b.shape
        kind = t % 6 if t < 12 else int(rng.integers(0, 6))           # (every kind is in every list of 6 or more)
        r, c = int(rng.integers(0, n_r)), int(rng.integers(0, n_c))
        if kind == 1:                                                  # the window leaves the map
            r = -1 if t == 1 else int(rng.choice([-3, -1, 0, 1, n_r - 2, n_r - 1, n_r, n_r + 2]))
        elif kind == 2 and not b.inter:                                # on the main diagonal
            c = r
        elif kind == 3 and not b.inter:                                # next to it, either side
            c = min(max(r + int(rng.choice([-1, 1])), 0), n_c - 1)
        elif kind == 4 and chroms[blk[t]] is not None:                 # a missing row
            ci = chroms[blk[t]]
            miss = np.flatnonzero(dcool.miss_host[dcool.offsets[ci]:dcool.offsets[ci + 1]])
            if miss.size:
                r = int(rng.choice(miss))
                c = min(r + int(rng.integers(0, 20)), n_c - 1)
        elif kind == 5 and t > 0:                                      # a pixel the list already holds
            s = int(rng.integers(0, t))
            blk[t], r, c = blk[s], rows[s], cols[s]
        elif not b.inter:
            c = min(r + int(rng.integers(0, MD)), n_c - 1)
        rows[t], cols[t] = r, c
    return blk.astype(np.int32), rows, cols


def stored_twin(b):
    """The quantify entry reads stored bands.  A block staged with lazy64="all" holds every diagonal of its float64 band beside
    the descriptor, which evaluates to exactly those values: the same buffers as a plain band."""
    if b.sig.layout != LAYOUT_BAND_LAZY:
        return b
    twin = pipeline.StagedBlock(b.name, CsMatrix(b.buffer.ptr, CS_F64, LAYOUT_BAND, b.sig.ld, 0, b.sig.band_w, 0), b.shape, b.miss_row,
                                b.miss_col, b.max_dist, b.inter, b.keep)
    twin.parent = b                  # (keeps the buffers alive; a twin owns none)
    return twin


def check_primitive(dcool, chroms, blocks, shape, ns, seed, restaged=False):
    """pipeline.pileup_blocks == the restated order on the windows of engine.run_quantify_blocks, bit for bit; twice the same.
    restaged: the blocks' bands exist only as descriptors; the quantify entry gets the blocks staged once more with their bands
    stored (StagedBlock.full) -- another reduction of the distance law, so every window value is the same to rounding only (1e-12,
    what the project grants a window: tests/test_gpu_device_pipeline.py) and the sums are held to the bound of
    tests/pileup_util.py with that per value."""
    rng = np.random.default_rng(seed)
    kspec = engine.KernelSpec(rng.random(shape))
    live = [k for k, b in enumerate(blocks) if min(b.shape) > max(shape)]
    blocks, chroms = [blocks[k] for k in live], [chroms[k] for k in live]
    assert blocks
    for n in ns:
        blk, rows, cols = pixel_list(dcool, chroms, blocks, n, rng)
        total, count = pipeline.pileup_blocks(dcool, blocks, shape, blk, rows, cols)
        assert total.shape == shape and count.shape == shape and total.dtype == np.float64 and count.dtype == np.int64
        if n:
            ref_blocks = [b.full() for b in blocks] if restaged else [stored_twin(b) for b in blocks]
            _, wins = engine.run_quantify_blocks(dcool.dev, ref_blocks, kspec, blk, rows, cols, want_windows=True)
            if n >= 12:
                gone = np.isnan(wins).all(axis=(1, 2))
                assert gone.any() and not gone.all(), n          # windows that leave the map, and windows that do not
        else:
            wins = np.zeros((0,) + shape)
        want_sum, want_cnt = restated_pileup(wins)
        assert np.array_equal(count, want_cnt), (shape, n)
        if restaged:
            assert (np.abs(total - want_sum) <= sum_bound(wins, per_value=1e-12)).all(), (shape, n, float(np.abs(total - want_sum).max()))
        else:
            assert np.array_equal(total.view(np.int64), want_sum.view(np.int64)), (shape, n, float(np.abs(total - want_sum).max()))
        again = pipeline.pileup_blocks(dcool, blocks, shape, blk, rows, cols)
        assert np.array_equal(again[0].view(np.int64), total.view(np.int64)) and np.array_equal(again[1], count)
        if n >= 12:
            assert count.max() > 1 and np.abs(total).max() > 0


def chunk_lengths():
    s = engine.pileup_chunk(1)
    assert engine.pileup_chunk(3 * s + 5) == s
    return [0, 1, s - 1, s, s + 1, 3 * s + 5]


@pytest.mark.parametrize("stored", [False, True], ids=["lazy bands", "stored float64 bands"])
@pytest.mark.parametrize("shape", [(7, 7), (15, 15), (17, 17), (31, 31), (9, 15)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pileup_equals_restated_order_on_quantify_windows(genome_a, shape, stored):
    _, dcool = genome_a
    chroms = list(range(len(SIZES_A)))
    options = dict(band_dtype=np.float64) if stored else dict(lazy64="all")
    blocks = dcool.stage_blocks(chroms, MD, max(shape), **options)
    dcool.dev.sync()
    # (a block is a band while the band is less than half of the dense map, pipeline.intra_geometry: the 150- and 90-bin
    # blocks up to 13 x 13 / 7 x 7 here, dense above -- the wider templates meet lazily evaluated bands on the 400-bin
    # chromosome below)
    layouts = [b.sig.layout for b in blocks]
    assert layouts[2] == LAYOUT_DENSE and layouts[3] == LAYOUT_DENSE
    assert all(lay != LAYOUT_BAND_LAZY for lay in layouts) if stored else all(lay in (LAYOUT_BAND_LAZY, LAYOUT_DENSE) for lay in layouts)
    if shape == (7, 7):
        assert layouts[0] == (LAYOUT_BAND if stored else LAYOUT_BAND_LAZY)
    ns = chunk_lengths()
    if shape == (7, 7):
        ns = ns + [5003]                       # past 512 chunks of 8: the chunk grows with n
        assert engine.pileup_chunk(5003) > engine.pileup_chunk(1)
    check_primitive(dcool, chroms, blocks, shape, ns, seed=shape[0] * 100 + shape[1] + int(stored))


@pytest.mark.parametrize("shape", [(7, 7), (15, 15), (17, 17), (31, 31), (9, 15)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pileup_on_lazily_evaluated_bands(genome_b, shape):
    """The 400-bin chromosome, a band for every template here.  Scanned to 60 bins with every diagonal stored beside the
    descriptor, and to 150 bins with only the first diagonals stored (stage_genome's default for the detection path): windows
    gathered per record from the pixel table (17 x 17: the compile-time-size gather; up to 17 x 17: the general one) or read
    pixel by pixel (beyond the gather's LDS slots)."""
    _, dcool = genome_b
    for max_dist, lazy64, ns in ((MD, "all", chunk_lengths()), (150, True, [1, 29])):
        blocks = dcool.stage_blocks([0], max_dist, max(shape), lazy64=lazy64)
        dcool.dev.sync()
        assert blocks[0].sig.layout == LAYOUT_BAND_LAZY
        check_primitive(dcool, [0], blocks, shape, ns, seed=500 + shape[0] + max_dist, restaged=lazy64 is True)


def test_pileup_equals_restated_order_on_detect_windows(genome_b):
    """The windows the detect chain itself returns for a block whose band exists only as a descriptor (what detect_genome's
    host route fetches): the pileup at the records' pixels is the restated order applied to them, bit for bit."""
    _, dcool = genome_b
    blocks = dcool.stage_blocks([0], 150, 17, lazy64=True)
    dcool.dev.sync()
    assert blocks[0].sig.layout == LAYOUT_BAND_LAZY
    cfg = copy.deepcopy(ck.loops)
    cfg["max_dist"] = 150 * BINSIZE
    res = cid.detect_blocks_on_device(dcool.dev, blocks, engine.KernelSpec(LOOPS), cfg, want_windows=True)
    assert res is not None
    table, wins = res[0]
    assert len(table) > 8 and wins.shape == (len(table), 17, 17)
    total, count = pipeline.pileup_blocks(dcool, blocks, (17, 17), np.zeros(len(table), dtype=np.int32), table[:, 0], table[:, 1])
    want_sum, want_cnt = restated_pileup(wins)
    assert np.array_equal(count, want_cnt)
    assert np.array_equal(total.view(np.int64), want_sum.view(np.int64)), float(np.abs(total - want_sum).max())


def test_pileup_81x81(genome_b):
    _, dcool = genome_b
    blocks = dcool.stage_blocks([0], MD, 81)
    dcool.dev.sync()
    check_primitive(dcool, [0], blocks, (81, 81), [1, 9, 29], seed=81)


def test_pileup_trans_block(genome_a):
    """A trans block (stage_inter, inter = 1: no NaN sub-diagonals) beside an intra block in one call."""
    _, dcool = genome_a
    intra = dcool.stage_blocks([0], MD, 15)[0]
    trans = dcool.stage_inter(0, 1, resident=True)
    dcool.dev.sync()
    assert trans.inter and trans.shape == (150, 90)
    check_primitive(dcool, [0, None], [intra, trans], (15, 15), [1, 29], seed=7)
    check_primitive(dcool, [None], [trans], (9, 15), [29], seed=8)


def test_pileup_against_the_oracle_windows(genome_a):
    """One intra block: counts equal to the oracle's (foci_oracle.quantify_table_band, reached as
    tests/quantify_oracle_util.py reaches it), sums within the bound of two orderings of a float64 sum plus the 1e-12 per
    value the project grants a device window (tests/test_gpu_device_pipeline.py), per pixel."""
    cool, dcool = genome_a
    shape = (15, 15)
    rng = np.random.default_rng(15)
    blocks = dcool.stage_blocks([0], MD, 15)
    dcool.dev.sync()
    blk, rows, cols = pixel_list(dcool, [0], blocks, 61, rng)
    total, count = pipeline.pileup_blocks(dcool, blocks, shape, blk, rows, cols)
    prepared, miss = qo.intra_block(cool, 0, MD, 15)
    # (the tolerances out of the way: the pileup takes every window that lies in the map; the acceptance rules are the caller's)
    lax = dict(max_perc_undetected=200.0, max_perc_zero=200.0, max_dist=MD * BINSIZE)
    wins = qo.quantify_intra(prepared, miss, rng.random(shape), np.column_stack([rows, cols]), lax, MD)["windows"]
    assert np.array_equal(count, np.sum(~np.isnan(wins), axis=0))
    assert count.max() > 20 and count.min() < count.max()          # (NaN sub-diagonals, missing bins: the pixels differ)
    err, bound = np.abs(total - np.nansum(wins, axis=0)), sum_bound(wins, per_value=1e-12)
    print("pileup vs oracle windows: max |sum_dev - sum_oracle| =", float(err.max()), "bound at that pixel =", float(bound.ravel()[err.argmax()]))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------
# end to end: parallel.detect_genome, two iterations
# ------------------------------------------------------------------------------------------------
def two_iterations(monkeypatch, cool, cfg, host):
    """(records, want_windows of every pipeline.detect_blocks call)."""
    asked = []
    inner = pipeline.detect_blocks

    def spy(*args, **kwargs):
        asked.append(bool(kwargs.get("want_windows", True)))
        return inner(*args, **kwargs)

    with monkeypatch.context() as m:
        m.setattr(pipeline, "detect_blocks", spy)
        if host:
            m.setenv("CHROMOSIGHT_HIP_HOST_PILEUP", "1")
        else:
            m.delenv("CHROMOSIGHT_HIP_HOST_PILEUP", raising=False)
        rec = parallel.detect_genome(pipeline.DeviceCool(cool), cfg)
    return rec, asked


@pytest.mark.parametrize("which", ["a", "b"], ids=["150+90+40+12 bins", "400+150+36 bins"])
def test_detect_genome_two_iterations_loops(monkeypatch, genome_a, genome_b, which):
    cool, dcool = genome_a if which == "a" else genome_b
    cfg = copy.deepcopy(ck.loops)
    cfg["max_dist"] = MD * BINSIZE
    cfg["max_iterations"] = 2
    rec, asked = two_iterations(monkeypatch, cool, cfg, host=False)
    rec_host, asked_host = two_iterations(monkeypatch, cool, cfg, host=True)
    n0, n1 = int((rec[:, 6] == 0).sum()), int((rec[:, 6] == 1).sum())
    print(f"two iterations of loops: {n0} + {n1} records")
    # (d) patterns in both iterations
    assert n0 > 0 and n1 > 0
    # (a) the device route == the host route
    assert rec.shape == rec_host.shape
    assert np.array_equal(rec[:, [0, 1, 2, 5, 6]], rec_host[:, [0, 1, 2, 5, 6]])
    assert np.abs(rec[:, 3] - rec_host[:, 3]).max() < 1e-9
    # (c) no call asked for windows on the device route (the host route fetches those of the first iteration)
    assert len(asked) == 2 and not any(asked)
    assert asked_host == [True, False]
    # (b) the second iteration == the oracle pipeline with the template rebuilt from the first one's records
    first = rec[rec[:, 6] == 0]
    chroms = list(range(dcool.n_chrom))
    blocks = dcool.stage_blocks(chroms, MD, 17)
    dcool.dev.sync()
    ids, blk = np.unique(first[:, 0].astype(np.int64), return_inverse=True)       # (the 12-bin block is smaller than the template)
    total, count = pipeline.pileup_blocks(dcool, [blocks[ci] for ci in ids], LOOPS.shape, blk, first[:, 1], first[:, 2])
    assert count.min() > 0
    template = total / count
    found = 0
    for ci in chroms:
        want = oracle_block_tables(cool, ci, cfg, MD, [template])[0]
        got = rec[(rec[:, 0] == ci) & (rec[:, 6] == 1)]
        assert got.shape[0] == want.shape[0], (ci, got.shape[0], want.shape[0])
        if want.shape[0]:
            assert np.array_equal(got[:, 1:3], want[:, :2]), ci                  # same foci, same order
            assert np.abs(got[:, 3] - want[:, 2]).max() < 1e-9, ci
        found += want.shape[0]
    assert found == n1


def test_detect_genome_two_iterations_borders(monkeypatch, genome_b):
    """The three borders templates with two iterations.  A 1-D pattern cannot be iterated (tests/test_gpu_reference_pins.py:
    the windows of intra maps carry NaN on the first sub-diagonals, so does their pileup, and the next iteration refuses the
    template as the reference does): that stays as it is on both routes -- the device pileup has its NaN where the host mean
    has them --, and the device route has not asked for windows by then."""
    cool, dcool = genome_b
    cfg = copy.deepcopy(ck.borders)
    cfg["max_iterations"] = 2
    assert len(cfg["kernels"]) == 3
    for host in (False, True):
        asked = []
        inner = pipeline.detect_blocks

        def spy(*args, **kwargs):
            asked.append(bool(kwargs.get("want_windows", True)))
            return inner(*args, **kwargs)

        with monkeypatch.context() as m:
            m.setattr(pipeline, "detect_blocks", spy)
            if host:
                m.setenv("CHROMOSIGHT_HIP_HOST_PILEUP", "1")
            else:
                m.delenv("CHROMOSIGHT_HIP_HOST_PILEUP", raising=False)
            with pytest.raises(ValueError, match="Cannot have flat kernel."):
                parallel.detect_genome(pipeline.DeviceCool(cool), cfg)
        assert asked and asked[0] == host and (host or not any(asked))
    # the pileup of the first template's first iteration, device and host: the same NaN, the same means to rounding
    one = dict(cfg, max_iterations=1, kernels=cfg["kernels"][:1])
    first = parallel.detect_genome(dcool, one)
    assert first.shape[0] > 0
    chroms = list(range(dcool.n_chrom))
    shape = np.shape(cfg["kernels"][0])
    blocks = dcool.stage_blocks(chroms, 1, shape[0])
    dcool.dev.sync()
    ids, blk = np.unique(first[:, 0].astype(np.int64), return_inverse=True)
    blocks, rows, cols = [blocks[ci] for ci in ids], first[:, 1], first[:, 2]
    total, count = pipeline.pileup_blocks(dcool, blocks, shape, blk, rows, cols)
    _, wins = engine.run_quantify_blocks(dcool.dev, blocks, engine.KernelSpec(np.asarray(cfg["kernels"][0], dtype=np.float64)), blk,
                                         rows.astype(np.int64), cols.astype(np.int64), want_windows=True)
    want_sum, want_cnt = restated_pileup(wins)
    assert np.array_equal(count, want_cnt) and np.array_equal(total.view(np.int64), want_sum.view(np.int64))
    assert (count[np.tril_indices(shape[0], -1)] == 0).all() and (count[np.triu_indices(shape[0])] > 0).all()
