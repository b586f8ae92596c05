"""Wall time of one parallel.detect_genome(loops, max_iterations=2) on bench.py's synthetic genome (tools/synthetic_genome.make_cool:
200 000 bins of 2 kb in 23 chromosomes, max_dist 1000 bins) with the pileup of the first iteration reduced on the device
(pipeline.pileup_blocks, the default) and formed on the host from fetched windows (CHROMOSIGHT_HIP_HOST_PILEUP=1, the route
before cs_pileup_blocks existed), and the time of the pileup call alone (profiles/pileup_time.json).

The two routes alternate in ONE process: warm-up runs of each first, then --reps rounds of (device, host); medians and every run
are reported.  A step is a host clock around detect_genome, which returns host tables (the device is idle when it returns).  The
pileup call alone -- the accepted records of the first iteration at their staged blocks -- is timed with device events around
cs_pileup_blocks and with a host clock around the same call (it is synchronous).  The records of the two routes are compared
before anything is timed.  On a checkout that has no pipeline.pileup_blocks (the parent commit) only the one route there is
timed, under "parent": run the tool on both checkouts on the same box to compare commits.

    python tools/time_pileup.py [--out profiles/pileup_time.json] [--reps 7] [--warmup 2] [--bins 200000]
"""
import argparse
import copy
import json
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import chromosight_amd.kernels as ck  # noqa: E402
from chromosight_amd import parallel, pipeline  # noqa: E402
from tools.synthetic_genome import make_cool  # noqa: E402

SWITCH = "CHROMOSIGHT_HIP_HOST_PILEUP"


def summary(runs):
    return {"median_s": round(float(np.median(runs)), 6), "min_s": round(float(np.min(runs)), 6), "runs_s": [round(x, 6) for x in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bins", type=int, default=200_000)
    ap.add_argument("--max-dist", type=int, default=1000)
    args = ap.parse_args()
    template = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    cool, _ = make_cool(args.bins, args.max_dist, 2000, seed=2, template=template)
    dcool = pipeline.DeviceCool(cool)
    dev = dcool.dev
    cfg = copy.deepcopy(ck.loops)
    cfg["max_dist"] = args.max_dist * 2000
    cfg["max_iterations"] = 2
    has_device_route = hasattr(pipeline, "pileup_blocks")
    routes = ["device", "host"] if has_device_route else ["parent"]

    def step(route):
        if route == "host":
            os.environ[SWITCH] = "1"
        else:
            os.environ.pop(SWITCH, None)
        try:
            t0 = time.perf_counter()
            rec = parallel.detect_genome(dcool, cfg)
            return time.perf_counter() - t0, rec
        finally:
            os.environ.pop(SWITCH, None)

    res = {"bins": int(dcool.n_bins), "chromosomes": int(dcool.n_chrom), "max_dist_bins": args.max_dist, "template": list(template.shape),
           "reps": args.reps, "warmup_runs": args.warmup,
           "timing": "host clock around parallel.detect_genome(loops, max_iterations=2), which returns host tables; routes alternate in one process",
           "library": dev.lib.cs_version().decode(), "loadavg_start": [round(x, 2) for x in os.getloadavg()]}
    recs = {}
    for route in routes:
        for _ in range(max(args.warmup, 1)):
            _, recs[route] = step(route)
    rec = recs[routes[0]]
    n0, n1 = int((rec[:, 6] == 0).sum()), int((rec[:, 6] == 1).sum())
    res["records_iteration_0"], res["records_iteration_1"] = n0, n1
    if has_device_route:
        a, b = recs["device"], recs["host"]
        same = a.shape == b.shape and np.array_equal(a[:, [0, 1, 2, 5, 6]], b[:, [0, 1, 2, 5, 6]])
        res["routes_agree"] = bool(same)
        res["max_score_difference"] = float(np.abs(a[:, 3] - b[:, 3]).max()) if same and a.shape[0] else None
        if not same:
            raise SystemExit("the device and the host route report different records")
    runs = {route: [] for route in routes}
    for _ in range(args.reps):
        for route in routes:
            runs[route].append(step(route)[0])
    for route in routes:
        res["step_" + route] = summary(runs[route])
    if has_device_route:
        res["step_host_over_device"] = round(res["step_host"]["median_s"] / res["step_device"]["median_s"], 4)
        # the pileup call alone: the first iteration's records at their staged blocks
        first = rec[rec[:, 6] == 0]
        chroms = list(range(dcool.n_chrom))
        blocks = dcool.stage_blocks(chroms, args.max_dist, template.shape[0])
        dev.sync()
        ids, blk = np.unique(first[:, 0].astype(np.int64), return_inverse=True)
        used = [blocks[ci] for ci in ids]
        call = lambda: pipeline.pileup_blocks(dcool, used, template.shape, blk, first[:, 1], first[:, 2])      # noqa: E731
        for _ in range(max(args.warmup, 1)):
            total, count = call()
        e0, e1 = dev.new_event(), dev.new_event()
        ev, host = [], []
        for _ in range(args.reps):
            dev.record(e0)
            t0 = time.perf_counter()
            call()
            host.append(time.perf_counter() - t0)
            dev.record(e1)
            dev.sync()
            ev.append(dev.elapsed_ms(e0, e1) * 1e-3)
        res["pileup_call"] = {"records": int(first.shape[0]), "blocks": len(used), "chunk": int(dev.lib.cs_pileup_chunk(int(first.shape[0]))),
                              "device_events": summary(ev), "host_clock": summary(host),
                              "bytes_back": int(total.nbytes + count.nbytes),
                              "bytes_of_the_accepted_windows": int(first.shape[0]) * int(template.size) * 8}
    try:
        import bench
        res["gpu_state"] = bench.gpu_state(lambda: parallel.detect_genome(dcool, cfg), dev.sync)
    except Exception as exc:                                  # noqa: BLE001 -- the clocks are a side note of the timing
        res["gpu_state"] = repr(exc)
    res["loadavg_end"] = [round(x, 2) for x in os.getloadavg()]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
