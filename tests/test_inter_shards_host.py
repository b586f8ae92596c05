"""Sharded `detect --inter` on CPU (gloo): the assignment of DetectShard.select over intra and trans units, the per-unit
exchange of DetectShard.merge on 2 and 3 ranks, and the argument checks of pipeline.detect(shard=...) (the device route
itself is covered by tests/test_gpu_inter_shards.py)."""
import copy
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import chromosight_amd.kernels as ck
from chromosight_amd import parallel, pipeline
from tools.synthetic_inter import trans_chrom_sizes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pairs(n_chrom):
    return [(a, b) for a in range(n_chrom) for b in range(n_chrom) if a == b or a < b]


def _yeast_sizes():
    cool = np.load(os.path.join(GOLDEN, "yeast_cool.npz"), allow_pickle=False)
    return np.diff(np.asarray(cool["chrom_offset"], dtype=np.int64)), int(cool["binsize"])


class _Alone(parallel.DetectShard):
    """A DetectShard as rank `rank` of `world` would build it (select only reads the rank and world)."""

    def __init__(self, rank, world):
        super().__init__()
        self.rank, self.world = rank, world


def _check_assignment(sizes, max_dist, largest):
    pairs = _pairs(len(sizes))
    costs = parallel.inter_unit_costs(pairs, sizes, max_dist, largest)
    for (a, b), c in zip(pairs, costs):
        want = sizes[a] * min(max_dist + largest, sizes[a]) if a == b else sizes[a] * sizes[b]
        assert c == want
    assert parallel.DetectShard().select(pairs, sizes, max_dist, largest) == list(range(len(pairs)))     # world 1: everything
    for world in (2, 3, 8):
        shares = [_Alone(r, world).select(pairs, sizes, max_dist, largest) for r in range(world)]
        # the same lists whichever rank computes them, in unit order, disjoint and covering all units: LPT of assign_blocks
        assert shares == parallel.assign_blocks(costs, world)
        assert shares == [_Alone(r, world).select(pairs, sizes, max_dist, largest) for r in range(world)]
        assert all(s == sorted(s) for s in shares)
        assert sorted(sum(shares, [])) == list(range(len(pairs)))
    return pairs, costs


def test_select_yeast_shapes():
    sizes, binsize = _yeast_sizes()
    assert len(sizes) == 17
    max_dist = max(ck.loops["max_dist"] // binsize, 1)
    pairs, costs = _check_assignment(sizes, max_dist, 17)
    assert len(pairs) == 153
    # LPT: no share exceeds the mean by more than the largest unit
    for world in (2, 3, 8):
        loads = [sum(costs[i] for i in s) for s in parallel.assign_blocks(costs, world)]
        assert max(loads) <= sum(costs) / world + max(costs)


def test_select_hg38_shapes_balance():
    sizes = trans_chrom_sizes()
    pairs, costs = _check_assignment(sizes, 200, 17)
    assert len(pairs) == 300
    assert 45.5e9 < sum(costs) < 46e9 and max(costs) < 0.62e9
    ratio = {}
    for world in (8, 16):
        loads = [sum(costs[i] for i in s) for s in parallel.assign_blocks(costs, world)]
        ratio[world] = max(loads) / (sum(costs) / world)
    assert ratio[8] < 1.001 and ratio[16] < 1.005, ratio


def test_owned_units_are_kept():
    pairs = _pairs(4)
    sizes = [50, 40, 30, 20]
    assert parallel.DetectShard(owned=[7, 2]).select(pairs, sizes, 10, 3) == [2, 7]
    with pytest.raises(ValueError):
        parallel.DetectShard(owned=[len(pairs)]).select(pairs, sizes, 10, 3)


# ------------------------------------------------------------------------------------------------
# merge: every rank ends with the single-process list of (unit, table, windows), in unit order
# ------------------------------------------------------------------------------------------------
KSHAPE = (5, 5)


def _fake_result(u, it):
    """What a unit yields on the device in iteration `it`: nothing for some units, a few records (with NaN in windows) else."""
    n = (u * 7 + it * 3) % 5
    if n == 0 or u % 4 == 3:
        return None, None
    tab = np.column_stack([np.arange(n) + 10.0 * u, np.arange(n)[::-1] + 1.0, np.sin(u + np.arange(n) + it), np.full(n, 0.01 * u)])
    win = np.cos(np.arange(n * 25, dtype=np.float64) + u).reshape((n,) + KSHAPE)
    win[::2, 1, 3] = np.nan
    return tab, win


def _single(n_units, it, need_windows):
    done, out = [], []
    for u in range(n_units):
        tab, win = _fake_result(u, it)
        if tab is not None:
            done.append(u)
            out.append((tab, win if need_windows else None))
    return done, out


def _merge_worker(rank, world, port, out_dir, n_units, owned_all):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shard = parallel.DetectShard(owned=owned_all[rank])
        units = shard.select(_pairs(8)[:n_units], [1] * 8, 1, 1)
        got = {}
        for it, need in ((0, True), (1, False), (2, True)):
            results = [_fake_result(u, it) for u in units]
            if not need:
                results = [(t, None) for t, _ in results]
            done, out = shard.merge(units, results, KSHAPE, need)
            got[f"done{it}"] = np.asarray(done, dtype=np.int64)
            got[f"tab{it}"] = np.concatenate([t for t, _ in out]) if out else np.zeros((0, 4))
            if need:
                got[f"win{it}"] = np.concatenate([w for _, w in out]) if out else np.zeros((0,) + KSHAPE)
            else:
                assert all(w is None for _, w in out)
        np.savez(os.path.join(out_dir, f"m{rank}.npz"), **got)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n_units,owned", [
    (2, 11, None),
    (3, 11, None),
    (3, 3, [[0, 2], [], [1]]),              # a rank that owns nothing
    (3, 8, [[3, 7], [0, 1, 2], [4, 5, 6]]),  # a rank whose units find nothing (3, 7)
])
def test_merge_gives_every_rank_the_single_process_list(tmp_path, world, n_units, owned):
    if owned is None:
        owned = parallel.assign_blocks([(u * 13) % 7 + 1 for u in range(n_units)], world)
    mp.spawn(_merge_worker, args=(world, _free_port(), str(tmp_path), n_units, owned), nprocs=world, join=True)
    for it, need in ((0, True), (1, False), (2, True)):
        done, out = _single(n_units, it, need)
        tab = np.concatenate([t for t, _ in out])
        for r in range(world):
            got = np.load(tmp_path / f"m{r}.npz")
            assert got[f"done{it}"].tolist() == done, (r, it)
            assert np.array_equal(got[f"tab{it}"], tab), (r, it)
            if need:
                win = np.concatenate([w for _, w in out])
                assert np.isnan(win).any()
                assert np.array_equal(got[f"win{it}"], win, equal_nan=True), (r, it)


def test_merge_world1_and_no_exchange_keep_the_local_list():
    units = [1, 4]
    results = [_fake_result(u, 0) for u in units]
    for shard in (parallel.DetectShard(), parallel.DetectShard(owned=units, exchange=False)):
        done, out = shard.merge(units, results, KSHAPE, True)
        assert done == units and out is results


# ------------------------------------------------------------------------------------------------
# argument checks, before any device work
# ------------------------------------------------------------------------------------------------
def test_detect_shard_needs_inter():
    cool = {"count": np.zeros(0)}                       # (never reaches the device: the checks come first)
    with pytest.raises(ValueError, match="inter"):
        pipeline.detect(cool, copy.deepcopy(ck.loops), inter=False, shard=parallel.DetectShard())


def test_detect_shard_without_exchange_needs_one_iteration():
    cfg = copy.deepcopy(ck.loops)
    cfg["max_iterations"] = 2
    with pytest.raises(ValueError, match="max_iterations"):
        pipeline.detect({"count": np.zeros(0)}, cfg, inter=True, shard=parallel.DetectShard(owned=[0], exchange=False))
    with pytest.raises(ValueError):
        pipeline.detect({"count": np.zeros(0)}, cfg, inter=True, shard=parallel.DetectShard(), inter_budget=0)
