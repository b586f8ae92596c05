"""Sharded `detect --inter` on the 310 000-bin scale genome (tools/synthetic_inter.make_trans_cool, defaults, seed 5), loops and
centromeres, inter_budget 2 GiB, one iteration -> profiles/inter_shards_time.json.

- baseline: the 1-rank pipeline.detect(inter=True), warm (the second call on the same DeviceCool);
- shares alone: for N = 2, 4, 8, the LPT assignment of parallel.DetectShard and every rank's share timed alone on one GPU
  (DetectShard(owned=..., exchange=False)), the slowest share's ratio to the 1-rank time, and where each share's time goes
  (intra staging, trans medians, intra scan, trans blocks in strips -- their host acceptance apart --, the rest);
- real runs: when the node has N GPUs, one N-rank run over "nccl", one GPU per rank: every rank's wall time with the exchanges.

Every GPU process is a child started by subprocess with its own time limit; the parent never opens the GPU.  A rank that
fails or times out ends the others.

    python tools/time_inter_shards.py [--out profiles/inter_shards_time.json] [--shares 2,4,8]
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BUDGET = 2 << 30
PATTERNS = ("loops", "centromeres")


def _setup(pattern):
    import copy
    import numpy as np
    import chromosight_amd.kernels as ck
    from tools.synthetic_inter import make_trans_cool
    t0 = time.perf_counter()
    cool, planted = make_trans_cool(template=np.asarray(ck.loops["kernels"][0], dtype=np.float64), seed=5)
    t_make = time.perf_counter() - t0
    cfg = copy.deepcopy(getattr(ck, pattern))
    cfg["max_perc_zero"] = 100.0            # (a planted pattern on an empty background: windows with zeros are kept)
    cfg["max_iterations"] = 1
    return cool, cfg, t_make


class _Laps:
    """Wall time spent inside some pipeline calls during one detect (the device calls return their results to the host)."""
    NAMES = ("stage_blocks", "inter_median", "detect_blocks", "detect_inter_block", "accept_records", "merge")

    def __init__(self):
        from chromosight_amd import parallel, pipeline
        from chromosight_amd.utils import detection as cid
        self.s = dict.fromkeys(self.NAMES, 0.0)
        targets = [(pipeline.DeviceCool, "stage_blocks"), (pipeline.DeviceCool, "inter_median"), (pipeline, "detect_blocks"),
                   (pipeline, "detect_inter_block"), (cid, "_accept_records"), (parallel.DetectShard, "merge")]
        for owner, name in targets:
            setattr(owner, name, self._wrap(getattr(owner, name), name.lstrip("_")))

    def _wrap(self, fn, key):
        def timed(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                self.s[key] += time.perf_counter() - t0
        return timed

    def take(self, wall):
        out = {k: round(v, 4) for k, v in self.s.items()}
        out["trans_blocks_less_acceptance"] = round(self.s["detect_inter_block"] - self.s["accept_records"], 4)
        out["other"] = round(wall - sum(self.s[k] for k in ("stage_blocks", "inter_median", "detect_blocks", "detect_inter_block",
                                                             "merge")), 4)
        self.s = dict.fromkeys(self.NAMES, 0.0)
        return out


def child_alone(pattern, shares):
    """Baseline and the shares of every N, one after the other on this process's GPU."""
    import numpy as np
    from chromosight_amd import parallel, pipeline
    cool, cfg, t_make = _setup(pattern)
    laps = _Laps()
    dcool = pipeline.DeviceCool(cool)
    sizes = np.diff(dcool.offsets)
    pairs = pipeline.sub_matrices(dcool, True)
    max_dist = max(cfg["max_dist"] // dcool.binsize, 1)
    largest = max(np.shape(k)[0] for k in cfg["kernels"])
    costs = parallel.inter_unit_costs(pairs, sizes, max_dist, largest)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        table = pipeline.detect(dcool, cfg, inter=True, inter_budget=BUDGET)
        runs.append(time.perf_counter() - t0)
        split = laps.take(runs[-1])
    base = runs[1]
    res = {"pattern": pattern, "host_generation_s": round(t_make, 2), "units": len(pairs),
           "intra_units": sum(a == b for a, b in pairs), "cost_pixels": int(sum(costs)),
           "one_rank": {"warm_s": round(base, 4), "runs_s": [round(r, 4) for r in runs], "patterns": len(table),
                        "trans_patterns": int((table.chrom1 != table.chrom2).sum()), "where_s_last_run": split,
                        "pool_high_water_bytes": int(dcool.inter_high_water)},
           "shares": {}}
    for n in shares:
        owned = parallel.assign_blocks(costs, n)
        per = []
        for r, units in enumerate(owned):
            shard = parallel.DetectShard(owned=units, exchange=False)
            t0 = time.perf_counter()
            pipeline.detect(dcool, cfg, inter=True, inter_budget=BUDGET, shard=shard)
            wall = time.perf_counter() - t0
            per.append({"rank": r, "units": len(units), "intra_units": sum(pairs[u][0] == pairs[u][1] for u in units),
                        "cost_pixels": int(sum(costs[u] for u in units)), "wall_s": round(wall, 4), "where_s": laps.take(wall)})
        slow = max(p["wall_s"] for p in per)
        loads = [p["cost_pixels"] for p in per]
        res["shares"][str(n)] = {"assignment": owned, "per_rank": per, "slowest_share_s": slow,
                                 "speedup_vs_one_rank": round(base / slow, 2), "slowest_over_one_rank": round(slow / base, 4),
                                 "cost_max_over_mean": round(max(loads) / (sum(loads) / n), 5),
                                 "time_max_over_mean": round(slow / (sum(p["wall_s"] for p in per) / n), 4)}
    return res


def child_rank(pattern):
    """One rank of a real N-rank run over nccl: warm call, then one timed call between barriers."""
    import torch
    import torch.distributed as dist
    from chromosight_amd import parallel, pipeline
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", rank=rank, world_size=world)
    cool, cfg, _ = _setup(pattern)
    dcool = pipeline.DeviceCool(cool)
    parallel.detect_inter_genome(dcool, cfg, inter_budget=BUDGET)
    dist.barrier()
    parallel.TIMERS.update(exchange_ms=0.0, exchanges=0)
    t0 = time.perf_counter()
    table = parallel.detect_inter_genome(dcool, cfg, inter_budget=BUDGET)
    mine = time.perf_counter() - t0
    dist.barrier()
    wall = time.perf_counter() - t0
    out = {"rank": rank, "own_s": round(mine, 4), "wall_to_barrier_s": round(wall, 4), "patterns": len(table),
           "exchange_s": round(parallel.TIMERS["exchange_ms"] / 1e3, 4), "exchanges": parallel.TIMERS["exchanges"],
           "transport": parallel.transport(), "pool_high_water_bytes": int(dcool.inter_high_water)}
    dist.destroy_process_group()
    return out


def _child(args, timeout, env=None):
    """Run this tool as a child; returns its JSON result (the last stdout line) or raises."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout,
                       env=env, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"child {args} exited with {p.returncode}:\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def real_run(pattern, n, timeout):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(n))
    procs = []
    for r in range(n):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), CHROMOSIGHT_HIP_DEVICE=str(r))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child-rank", pattern], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, env=e, cwd=ROOT))
    deadline = time.time() + timeout
    outs = []
    try:
        for r, p in enumerate(procs):
            out, err = p.communicate(timeout=max(1.0, deadline - time.time()))
            if p.returncode != 0:
                raise RuntimeError(f"rank {r} exited with {p.returncode}:\n{err[-3000:]}")
            outs.append(json.loads(out.strip().splitlines()[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)
    return {"ranks": n, "backend": "nccl", "slowest_rank_wall_s": max(o["wall_to_barrier_s"] for o in outs), "per_rank": outs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inter_shards_time.json"))
    ap.add_argument("--shares", default="2,4,8")
    ap.add_argument("--patterns", default=",".join(PATTERNS))
    ap.add_argument("--timeout", type=float, default=600.0)
    ap.add_argument("--child-alone", default=None)
    ap.add_argument("--child-rank", default=None)
    ap.add_argument("--child-count", action="store_true")
    args = ap.parse_args()
    shares = [int(x) for x in args.shares.split(",") if x]
    if max(shares, default=1) > 8:
        raise SystemExit("at most 8 ranks")
    if args.child_count:
        import torch
        return print(json.dumps({"devices": torch.cuda.device_count()}))
    if args.child_alone:
        return print(json.dumps(child_alone(args.child_alone, shares)))
    if args.child_rank:
        return print(json.dumps(child_rank(args.child_rank)))
    devices = _child(["--child-count"], 120)["devices"]
    out = {"what": "sharded detect --inter (parallel.DetectShard) on the scale genome, tools/time_inter_shards.py",
           "genome": "tools/synthetic_inter.make_trans_cool defaults, seed 5 (309 988 bins, 24 chromosomes in hg38 proportions)",
           "inter_budget_bytes": BUDGET, "max_iterations": 1, "devices": devices,
           "share_convention": "each rank's share timed alone on one GPU (DetectShard(owned=..., exchange=False)), warm DeviceCool",
           "patterns": {}}
    for pattern in args.patterns.split(","):
        res = _child(["--child-alone", pattern, "--shares", args.shares], args.timeout)
        res["real_runs"] = {}
        for n in shares:
            res["real_runs"][str(n)] = real_run(pattern, n, args.timeout) if devices >= n else f"not run: {devices} device(s)"
        out["patterns"][pattern] = res
        print(json.dumps({pattern: {"one_rank_s": res["one_rank"]["warm_s"],
                                    **{f"share_of_{n}": res["shares"][str(n)]["speedup_vs_one_rank"] for n in shares}}}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
