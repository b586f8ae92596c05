#!/usr/bin/env python3
"""Timing of `detect --smooth-trend` on the 200 000-bin / 23-block synthetic genome of bench.py's genome leg:

    python tools/time_smooth_trend.py [--bins 200000] [--steps 15] [--label NAME] [--out FILE.json] [--only-steps]

Times pipeline.detect(dcool, loops, smooth=True) (warm steps: median, minimum, maximum, every sample) and the staging call alone
(DeviceCool.stage_blocks(..., smooth=True), complete on the device), and for orientation the same two without smoothing.  Prints
one JSON object (and writes it to --out); run it on two checkouts on the same machine to compare them
(profiles/smooth_trend_time.json).  --only-steps: nothing but the warm-up and the smoothed detect steps, for a run under a
profiler (rocprofv3 --kernel-trace --stats -- python tools/time_smooth_trend.py --only-steps --steps 5)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import chromosight_amd.kernels as ck  # noqa: E402
from chromosight_amd import pipeline  # noqa: E402
from tools.synthetic_genome import make_cool  # noqa: E402


def summary(ms):
    ms = [float(x) for x in ms]
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "spread": round((max(ms) - min(ms)) / float(np.median(ms)), 4), "samples_ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=200_000)
    ap.add_argument("--max-dist", type=int, default=1000, help="scanning distance in bins")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--only-steps", action="store_true")
    args = ap.parse_args()
    template = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    cool, _ = make_cool(args.bins, args.max_dist, 2000, seed=2, template=template)
    dcool = pipeline.DeviceCool(cool)
    dev = dcool.dev
    cfg = copy.deepcopy(ck.loops)
    cfg["max_dist"] = args.max_dist * dcool.binsize
    chroms = list(range(dcool.n_chrom))

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        out = []
        for _ in range(steps):
            dev.sync()
            t0 = time.perf_counter()
            fn()
            dev.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def stage(smooth):
        blocks = dcool.stage_blocks(chroms, args.max_dist, 17, smooth=smooth)
        dev.sync()
        del blocks

    n_rows = len(pipeline.detect(dcool, cfg, smooth=True))
    if args.only_steps:
        timed(lambda: pipeline.detect(dcool, cfg, smooth=True), args.steps, args.warmup)
        return
    res = {"label": args.label, "bins": int(dcool.n_bins), "blocks": int(dcool.n_chrom), "max_dist_bins": args.max_dist,
           "rows_smooth": n_rows, "rows_plain": len(pipeline.detect(dcool, cfg))}
    res["detect_smooth"] = summary(timed(lambda: pipeline.detect(dcool, cfg, smooth=True), args.steps, args.warmup))
    res["stage_smooth"] = summary(timed(lambda: stage(True), args.steps, args.warmup))
    res["detect_plain"] = summary(timed(lambda: pipeline.detect(dcool, cfg), args.steps, args.warmup))
    res["stage_plain"] = summary(timed(lambda: stage(False), args.steps, args.warmup))
    try:
        import bench
        res["gpu_state"] = bench.gpu_state(lambda: pipeline.detect(dcool, cfg, smooth=True), dev.sync)
    except Exception as exc:                                  # noqa: BLE001 -- the clocks are a side note of the timing
        res["gpu_state"] = repr(exc)
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
