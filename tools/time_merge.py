"""Wall time of DeviceCool.merged() of 2 and of 8 replicates against the route a user has without it -- merging the decoded
dictionaries on the host (the numpy oracle of tests/merge_util.py) and uploading the merged table with DeviceCool(...) -- on
two tables (profiles/merge_time.json):

- the table of bench.py's synthetic genome (tools/synthetic_genome.make_cool: 200 000 bins of 2 kb in 23 chromosomes);
- the yeast fixture (tests/golden/yeast_cool.npz) with its trans pixels.

The replicates are seeded binomial splits of the table (every count halved binomially, log2(ways) times over: a multinomial split
with equal odds); a pixel that gets 0 stays in its replicate as a stored zero, so every replicate has the table's pixels and the
replicates sum back to it.  That is checked (exactly) on the device result before anything is timed.

The device time is a host clock around the call, which ends in a device synchronise (cs_merge_fill is synchronous): warm-up calls
first, then the median of --reps calls.  The bytes are what the two walks need, computed from the tables' shapes: both read every
source's row pointers, column bins and counts; the second writes the merged table.  Their sum over the call time is an end-to-end
rate (allocations, the descriptor upload and the host synchronisations included), not a kernel's share of peak.  The host route is
run --host-reps times where its concatenated table fits comfortably in memory (--host-pixel-limit), else it is "not measured".
One process, its own time limit.

    python tools/time_merge.py [--out profiles/merge_time.json] [--reps 7] [--tables bench,yeast] [--ways 2,8] [--time-limit 1100]
"""
import argparse
import json
import os
import pathlib
import signal
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from chromosight_amd import pipeline  # noqa: E402
from tests.merge_util import oracle_merge  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s, specification
HBM_COPY = 6.29e12          # measured with a float4 copy


def bench_table():
    import chromosight_amd.kernels as ck
    from tools.synthetic_genome import make_cool
    template = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    cool, _ = make_cool(200_000, 1000, 2000, seed=2, template=template)
    return cool


def yeast_table():
    return dict(np.load(ROOT / "tests" / "golden" / "yeast_cool.npz", allow_pickle=False))


def binomial_splits(cool, ways, seed):
    """`ways` (a power of two) replicates of `cool`: the counts halved binomially, level by level; int32 counts."""
    rng = np.random.default_rng(seed)
    cnt = np.asarray(cool["count"])
    if not (np.all(cnt == np.rint(cnt)) and cnt.min() >= 0 and cnt.max() < 2 ** 31):
        raise SystemExit("the table's counts are not non-negative integers below 2^31")
    level = [cnt.astype(np.int32)]
    while len(level) < ways:
        nxt = []
        for c in level:
            left = rng.binomial(c, 0.5).astype(np.int32)
            nxt += [left, c - left]
        level = nxt
    return [{**cool, "count": c, "weight": None} for c in level]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
        del r
    return float(np.median(out)), [round(x, 5) for x in out]


def measure(name, cool, ways, reps, host_reps, host_pixel_limit):
    dev = pipeline.get_device()
    t0 = time.perf_counter()
    parts = binomial_splits(cool, ways, seed=ways)
    split_s = time.perf_counter() - t0
    dparts = [pipeline.DeviceCool(p, dev) for p in parts]
    first = dparts[0]
    merged = first.merged(*dparts[1:])                                           # warm-up (code objects, allocator) and the check
    cnt = np.asarray(cool["count"])
    keep = cnt > 0
    n = merged.nnz
    dtype = np.float32 if cnt.max() < (1 << 24) else np.float64
    indptr = np.searchsorted(np.asarray(cool["bin1_id"])[keep], np.arange(first.n_bins + 1)).astype(np.int64)
    same = (n == int(keep.sum()) and merged.val_dtype is dtype and np.array_equal(merged.indptr.download(), indptr)
            and np.array_equal(merged.indices.download()[:n], np.asarray(cool["bin2_id"])[keep].astype(np.int32))
            and np.array_equal(merged.data.download()[:n], cnt[keep].astype(dtype)))
    if not same:
        raise SystemExit(f"{name} x{ways}: the merged replicates differ from the table they were split from")
    del merged
    first.merged(*dparts[1:])
    dev_s, dev_all = timed(lambda: first.merged(*dparts[1:]), reps)

    def host_route():
        up = pipeline.DeviceCool(oracle_merge(parts), dev)
        dev.sync()
        return up

    src_pixels = sum(d.nnz for d in dparts)
    if src_pixels <= host_pixel_limit:
        host_s, host_all = timed(host_route, host_reps)
    else:
        host_s, host_all = None, "not measured: the concatenated table is beyond --host-pixel-limit"
    esz = np.dtype(first.val_dtype).itemsize
    walk = src_pixels * (4 + esz) + ways * (first.n_bins + 1) * 8
    read = 2 * walk + (first.n_bins + 1) * 8 * 2
    written = n * (4 + np.dtype(dtype).itemsize) + (first.n_bins + 1) * 8 * 2
    rate = (read + written) / dev_s
    rec = {"ways": ways, "bins": first.n_bins, "chromosomes": first.n_chrom, "pixels_per_source": first.nnz, "source_pixels": src_pixels,
           "merged_pixels": n, "in_dtype": np.dtype(first.val_dtype).name, "out_dtype": np.dtype(dtype).name,
           "equal_to_the_split_table": True, "split_on_host_s": round(split_s, 2),
           "device_s": round(dev_s, 5), "device_runs_s": dev_all,
           "host_route_s": None if host_s is None else round(host_s, 3), "host_route_runs_s": host_all,
           "speedup": None if host_s is None else round(host_s / dev_s, 1), "bytes_read": int(read), "bytes_written": int(written),
           "call_rate_GBps": round(rate / 1e9, 1), "share_of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4),
           "share_of_measured_copy_6.29TBps": round(rate / HBM_COPY, 4)}
    host_txt = "not measured" if host_s is None else f"{host_s:.2f} s, x{host_s / dev_s:.0f}"
    print(f"{name} x{ways}: {src_pixels} -> {n} pixels, device {dev_s * 1e3:.2f} ms, host route {host_txt}, "
          f"{rate / 1e9:.0f} GB/s over the call", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "merge_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--tables", default="bench,yeast")
    ap.add_argument("--ways", default="2,8")
    ap.add_argument("--host-pixel-limit", type=int, default=400_000_000,
                    help="source pixels beyond which the host route is not run (its sort needs some 60 bytes per pixel)")
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds after which the process is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    dev = pipeline.get_device()
    rec = {"reps": args.reps, "warmup_calls": 2,
           "timing": "host clock around DeviceCool.merged (ends in a device synchronise); medians",
           "host_route": "tests/merge_util.oracle_merge of the decoded replicates + DeviceCool(merged) + synchronise",
           "box": {"library": dev.lib.cs_version().decode(), "compute_units": dev.cu_count, "cpus_usable": len(os.sched_getaffinity(0)),
                   "loadavg_start": [round(x, 2) for x in os.getloadavg()]}}
    tables = {"bench": ("bench_200000_bins", bench_table), "yeast": ("yeast_with_trans", yeast_table)}
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for key in args.tables.split(","):
        name, make = tables[key]
        cool = make()
        for ways in (int(w) for w in args.ways.split(",")):
            rec[f"{name}_x{ways}"] = measure(name, cool, ways, args.reps, args.host_reps, args.host_pixel_limit)
            rec["box"]["loadavg_end"] = [round(x, 2) for x in os.getloadavg()]
            out.write_text(json.dumps(rec, indent=1) + "\n")                     # (after every shape: a time limit keeps what is done)


if __name__ == "__main__":
    main()
