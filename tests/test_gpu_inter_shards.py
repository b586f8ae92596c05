"""Sharded `detect --inter` and `quantify --inter` (parallel.detect_inter_genome, parallel.quantify_genome): ranks as
subprocesses over gloo, all on GPU 0, each with its share of intra blocks and trans blocks (in row strips); every rank returns
the single-process table and windows."""
import copy
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import parallel, pipeline
from tools.synthetic_inter import make_trans_cool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LOOPS = np.asarray(ck.loops["kernels"][0], dtype=np.float64)

WORKER = r"""
import json, os, sys, numpy as np, pandas as pd
sys.path.insert(0, os.environ["CS_ROOT"])
import torch.distributed as dist
from chromosight_amd import parallel, pipeline
spec = json.loads(os.environ["CS_SPEC"])
sys.path.insert(0, os.path.join(os.environ["CS_ROOT"], "tests"))
from test_gpu_inter_shards import make_input
dist.init_process_group("gloo", rank=int(os.environ["RANK"]), world_size=int(os.environ["WORLD_SIZE"]))
rank = dist.get_rank()
out = os.environ["CS_OUT"] + f".{rank}"
cool, cfg, positions = make_input(spec)
if spec.get("no_resident"):
    # a trans block staged whole is an error here: the sharded quantify stages strips only
    def refuse(*a, **k):
        raise RuntimeError("trans block staged whole")
    pipeline.DeviceCool.stage_inter_many = refuse
    orig = pipeline.DeviceCool.stage_inter
    def stage_inter(self, *a, **k):
        if k.get("resident"):
            raise RuntimeError("trans block staged whole")
        return orig(self, *a, **k)
    pipeline.DeviceCool.stage_inter = stage_inter
dcool = pipeline.DeviceCool(cool)
if spec["mode"] == "detect":
    table, windows = parallel.detect_inter_genome(dcool, cfg, return_windows=True, inter_budget=spec["budget"])
else:
    table, windows = parallel.quantify_genome(dcool, positions, cfg, inter=True, inter_budget=spec["budget"],
                                              max_dist_bp=spec.get("max_dist_bp"))
table.to_pickle(out + ".pkl")
np.save(out + ".npy", windows)
with open(out + ".json", "w") as f:
    json.dump({"high_water": int(dcool.inter_high_water)}, f)
dist.destroy_process_group()
"""


def _crop(cool, chroms):
    """The map of the given chromosomes only (a smaller genome)."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    keep = np.concatenate([np.arange(off[c], off[c + 1]) for c in chroms])
    new_of = np.full(int(off[-1]), -1, dtype=np.int64)
    new_of[keep] = np.arange(keep.size)
    b1, b2 = new_of[np.asarray(cool["bin1_id"])], new_of[np.asarray(cool["bin2_id"])]
    sel = (b1 >= 0) & (b2 >= 0)
    out = dict(cool)
    out.update(bin1_id=b1[sel], bin2_id=b2[sel], count=np.asarray(cool["count"])[sel], weight=np.asarray(cool["weight"])[keep],
               bin_start=np.asarray(cool["bin_start"])[keep], bin_end=np.asarray(cool["bin_end"])[keep],
               chrom_offset=np.concatenate([[0], np.cumsum(off[1:][chroms] - off[:-1][chroms])]),
               chrom_names=np.asarray(cool["chrom_names"])[chroms])
    return out


def _yeast_positions(cool, g):
    names = [str(n) for n in cool["chrom_names"]]
    binsize = int(cool["binsize"])
    rows = []
    for bi in range(int(g["n_blocks"])):
        ca, cb = (int(x) for x in g[f"b{bi}_chroms"])
        for r, c in g[f"b{bi}_coords"]:
            rows.append((names[ca], int(r) * binsize, (int(r) + 1) * binsize, names[cb], int(c) * binsize, (int(c) + 1) * binsize))
    return pd.DataFrame(rows, columns=["chrom1", "start1", "end1", "chrom2", "start2", "end2"])


def make_input(spec, cool=None):
    """(cool, config, positions) of a test case -- built alike by the test and by every rank."""
    positions = None
    if cool is not None:
        pass
    elif spec["input"] == "scale":
        cool, _ = make_trans_cool(template=LOOPS, seed=5)
    else:
        cool = dict(np.load(os.path.join(GOLDEN, "yeast_cool.npz"), allow_pickle=False))
        if spec.get("crop"):
            cool = _crop(cool, spec["crop"])
    if spec["pattern"] == "quantify":
        g = dict(np.load(os.path.join(GOLDEN, "yeast_quantify.npz"), allow_pickle=False))
        cfg = dict(pearson=0.15, max_perc_undetected=75.0, max_perc_zero=10.0, max_dist=0, min_dist=0,
                   kernels=[g[f"kernel{ki}"] for ki in range(3)], max_iterations=1, min_separation=5000)
        positions = _yeast_positions(cool, g)
    else:
        cfg = copy.deepcopy(getattr(ck, spec["pattern"]))
        cfg["max_perc_zero"] = 100.0                # (sparse trans windows: keep the ones with zeros)
        if spec["pattern"] == "centromeres":
            cfg["pearson"] = 0.15
        cfg["max_iterations"] = spec.get("iterations", 1)
    return cool, cfg, positions


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(tmp_path, spec, world, timeout):
    """`world` ranks of WORKER on GPU 0; every wait has a time limit, and a rank that fails or times out ends the others."""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    out = tmp_path / "rank"
    env = dict(os.environ, CS_ROOT=ROOT, CS_OUT=str(out), CS_SPEC=json.dumps(spec), CHROMOSIGHT_HIP_DEVICE="0",
               MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world))
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r), LOCAL_RANK="0")) for r in range(world)]
    try:
        for r, p in enumerate(procs):
            rc = p.wait(timeout=timeout)
            assert rc == 0, f"rank {r} exited with {rc}"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    res = []
    for r in range(world):
        with open(f"{out}.{r}.json") as f:
            meta = json.load(f)
        res.append((pd.read_pickle(f"{out}.{r}.pkl"), np.load(f"{out}.{r}.npy"), meta))
    return res


def _same(got, want):
    """Every column identical except score, pvalue and qvalue; scores within 1e-9, p-values within rtol 1e-6, windows 1e-12."""
    (ta, wa), (tb, wb) = got, want
    assert len(ta) == len(tb) and list(ta.columns) == list(tb.columns)
    for col in tb.columns:
        a, b = ta[col].to_numpy(), tb[col].to_numpy()
        if col == "score":
            assert np.array_equal(np.isnan(a.astype(float)), np.isnan(b.astype(float)))
            assert np.allclose(a.astype(float), b.astype(float), rtol=0, atol=1e-9, equal_nan=True)
        elif col in ("pvalue", "qvalue"):
            a, b = a.astype(float), b.astype(float)
            bad = ~np.isclose(a, b, rtol=1e-6, atol=0, equal_nan=True)
            assert not bad.any(), (col, np.flatnonzero(bad)[:5], a[bad][:5], b[bad][:5], np.isnan(a).sum(), np.isnan(b).sum())
        elif a.dtype == object:
            assert (a == b).all(), col
        else:
            assert np.array_equal(a, b, equal_nan=True), col
    assert wa.shape == wb.shape
    assert np.array_equal(np.isnan(wa), np.isnan(wb))
    assert np.allclose(wa, wb, rtol=0, atol=1e-12, equal_nan=True)


def _cut_budget(dcool, reach, own=8):
    """The smallest budget that holds `own` rows and their halo of every trans block: the larger blocks go in several strips."""
    sizes = np.diff(dcool.offsets)
    halo = (reach - 1) // 2
    return max((own + 2 * halo) * ((int(n_c) + 15) // 16 * 16) * 8 for n_c in sizes[1:])


def _single_detect(spec, cool=None):
    cool, cfg, _ = make_input(spec, cool)
    dcool = pipeline.DeviceCool(cool)
    return dcool, pipeline.detect(dcool, cfg, inter=True, return_windows=True, inter_budget=spec["budget"])


@pytest.mark.parametrize("iterations", [1, 2])
def test_yeast_loops_two_ranks_equal_single_process(tmp_path, iterations):
    spec = dict(input="yeast", pattern="loops", iterations=iterations, mode="detect")
    cool, cfg, _ = make_input(spec)
    spec["budget"] = _cut_budget(pipeline.DeviceCool(cool), pipeline._strip_reach(cfg["kernels"]))
    dcool, want = _single_detect(spec)
    sizes = np.diff(dcool.offsets)
    halo = (pipeline._strip_reach(cfg["kernels"]) - 1) // 2
    assert max(len(pipeline.plan_inter_strips(sizes[a], sizes[b], spec["budget"], halo))
               for a in range(len(sizes)) for b in range(a + 1, len(sizes))) >= 3
    assert (want[0].chrom1 != want[0].chrom2).sum() > 0 and (want[0].chrom1 == want[0].chrom2).sum() > 0
    if iterations == 2:
        assert (want[0].iteration == 1).sum() > 0
    for r, (table, windows, meta) in enumerate(_run_ranks(tmp_path, spec, 2, 900)):
        _same((table, windows), want)
        assert 0 < meta["high_water"] <= spec["budget"], r
    print(f"yeast loops --inter, {iterations} iteration(s), 2 ranks: {len(want[0])} patterns, budget {spec['budget']} B")


def test_yeast_centromeres_two_ranks_equal_single_process(tmp_path):
    spec = dict(input="yeast", pattern="centromeres", mode="detect")
    cool, cfg, _ = make_input(spec)
    spec["budget"] = _cut_budget(pipeline.DeviceCool(cool), pipeline._strip_reach(cfg["kernels"]), own=64)
    _, want = _single_detect(spec)
    assert (want[0].chrom1 != want[0].chrom2).sum() > 0
    for table, windows, _ in _run_ranks(tmp_path, spec, 2, 900):
        _same((table, windows), want)
    print(f"yeast centromeres --inter, 2 ranks: {len(want[0])} patterns")


def test_a_rank_without_units(tmp_path):
    """2 chromosomes = 3 units on 4 ranks: a rank owns nothing, and still takes part in every exchange."""
    spec = dict(input="yeast", crop=[10, 3], pattern="loops", mode="detect", budget=1 << 30)
    _, want = _single_detect(spec)
    cool, cfg, _ = make_input(spec)
    sizes = np.diff(np.asarray(cool["chrom_offset"]))
    assert len(sizes) == 2
    pairs = [(0, 0), (0, 1), (1, 1)]
    assert [] in parallel.assign_blocks(parallel.inter_unit_costs(pairs, sizes, 1000, 17), 4)
    assert len(want[0]) > 0
    for table, windows, _ in _run_ranks(tmp_path, spec, 4, 900):
        _same((table, windows), want)


def test_quantify_two_ranks_through_strips(tmp_path):
    """quantify_genome(inter=True) with a small inter_budget: the trans units of every rank go through their strips (a whole-
    block staging raises in the ranks), and both ranks return the single-process table and windows."""
    spec = dict(input="yeast", pattern="quantify", mode="quantify", no_resident=True)
    cool, cfg, positions = make_input(spec)
    g = dict(np.load(os.path.join(GOLDEN, "yeast_quantify.npz"), allow_pickle=False))
    spec["max_dist_bp"] = int(g["cfg_max_dist_bp"])
    dcool = pipeline.DeviceCool(cool)
    spec["budget"] = _cut_budget(dcool, pipeline._strip_reach(cfg["kernels"]))
    want = pipeline.quantify(dcool, positions, cfg, inter=True, inter_budget=spec["budget"], max_dist_bp=spec["max_dist_bp"])
    assert 0 < dcool.inter_high_water <= spec["budget"]
    for r, (table, windows, meta) in enumerate(_run_ranks(tmp_path, spec, 2, 900)):
        _same((table, windows), want)
        assert 0 < meta["high_water"] <= spec["budget"], r
    print(f"quantify --inter, 2 ranks in strips: {len(want[0])} positions, budget {spec['budget']} B")


def test_scale_two_ranks(tmp_path):
    """The 310 000-bin genome in hg38 proportions, loops, 2 GiB budget, 2 ranks: 40 of 40 planted trans patterns, the
    single-process table on both ranks."""
    spec = dict(input="scale", pattern="loops", mode="detect", budget=2 << 30)
    cool, planted = make_trans_cool(template=LOOPS, seed=5)
    dcool, want = _single_detect(spec, cool)
    del cool
    assert dcool.inter_high_water <= spec["budget"]
    del dcool
    trans = want[0][want[0].chrom1 != want[0].chrom2]
    found = set(zip(trans.bin1.astype(int), trans.bin2.astype(int)))
    runs = _run_ranks(tmp_path, spec, 2, 1200)
    for table, windows, meta in runs:
        _same((table, windows), want)
        assert meta["high_water"] <= spec["budget"]
        t = table[table.chrom1 != table.chrom2]
        got = set(zip(t.bin1.astype(int), t.bin2.astype(int)))
        hit = sum(any(abs(i - a) <= 1 and abs(j - b) <= 1 for a, b in got) for i, j in planted)
        assert hit == len(planted) == 40
    assert found
    print(f"scale --inter, 2 ranks: {len(want[0])} patterns, {len(trans)} trans")
