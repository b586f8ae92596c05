"""Wall time of DeviceCool.coarsened(5) against the route a user has without it -- coarsening on the host (the numpy oracle of
tests/coarsen_util.py) and an upload of the coarse table -- on two tables (profiles/coarsen_time.json):

- the table of bench.py's synthetic genome (tools/synthetic_genome.make_cool: 200 000 bins of 2 kb in 23 chromosomes);
- the yeast fixture (tests/golden/yeast_cool.npz) with its trans pixels.

The device time is a host clock around the call, which ends in a device synchronise (cs_coarsen is synchronous): warm-up calls first,
then the median of --reps calls.  The bytes are what the two walks need, computed from the tables' shapes: both read the row
pointers, the column bins and the counts; the second writes the coarse table.  Their sum over the call time is an end-to-end rate
(allocations, the upload of the two bin maps and both host synchronisations included), not a kernel's share of peak.  Both routes'
results are compared (exactly) before anything is timed.  One process, its own time limit.

    python tools/time_coarsen.py [--out profiles/coarsen_time.json] [--reps 7] [--tables bench,yeast] [--time-limit 900]
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
from tests.coarsen_util import csr_of, oracle_coarsen  # noqa: E402

HBM_PEAK = 8.0e12           # bytes / s, specification
HBM_COPY = 6.29e12          # measured with a float4 copy
FACTOR = 5


def bench_table():
    import chromosight_amd.kernels as ck
    from tools.synthetic_genome import make_cool
    template = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    cool, _ = make_cool(200_000, 1000, 2000, seed=2, template=template)
    return cool


def yeast_table():
    return dict(np.load(ROOT / "tests" / "golden" / "yeast_cool.npz", allow_pickle=False))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
        del r
    return float(np.median(out)), [round(x, 5) for x in out]


def measure(name, cool, reps, host_reps):
    dc = pipeline.DeviceCool(cool)
    dev = dc.dev
    want = oracle_coarsen(cool, FACTOR)
    indptr, indices, cnt, dtype = csr_of(want)
    co = dc.coarsened(FACTOR)                                                   # warm-up (code objects, allocator) and the check
    same = (co.nnz == cnt.size and co.val_dtype is dtype and np.array_equal(co.indptr.download(), indptr)
            and np.array_equal(co.indices.download()[:co.nnz], indices)
            and np.array_equal(co.data.download().view(dtype)[:co.nnz], cnt.astype(dtype)))
    if not same:
        raise SystemExit(f"{name}: the device table differs from the host oracle's")
    dc.coarsened(FACTOR)
    dev_s, dev_all = timed(lambda: dc.coarsened(FACTOR), reps)

    def host_route():
        up = pipeline.DeviceCool(oracle_coarsen(cool, FACTOR), dev)
        dev.sync()
        return up

    host_s, host_all = timed(host_route, host_reps)
    in_esz, out_esz = np.dtype(dc.val_dtype).itemsize, np.dtype(dtype).itemsize
    walk = dc.nnz * (4 + in_esz) + (dc.n_bins + 1) * 8
    read = 2 * walk + (co.n_bins + 1) * 8 * 2
    written = co.nnz * (4 + out_esz) + (co.n_bins + 1) * 8 * 2
    rate = (read + written) / dev_s
    rec = {"bins": dc.n_bins, "pixels": dc.nnz, "chromosomes": dc.n_chrom, "coarse_bins": co.n_bins, "coarse_pixels": co.nnz,
           "in_dtype": np.dtype(dc.val_dtype).name, "out_dtype": np.dtype(dtype).name, "equal_to_host_oracle": True,
           "device_s": round(dev_s, 5), "device_runs_s": dev_all, "host_route_s": round(host_s, 3), "host_route_runs_s": host_all,
           "speedup": round(host_s / dev_s, 1), "bytes_read": int(read), "bytes_written": int(written),
           "call_rate_GBps": round(rate / 1e9, 1), "share_of_hbm_peak_8TBps": round(rate / HBM_PEAK, 4),
           "share_of_measured_copy_6.29TBps": round(rate / HBM_COPY, 4)}
    print(f"{name}: {dc.nnz} -> {co.nnz} pixels, device {dev_s * 1e3:.2f} ms, host route {host_s:.2f} s, x{host_s / dev_s:.0f}, "
          f"{rate / 1e9:.0f} GB/s over the call", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "coarsen_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tables", default="bench,yeast")
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the process is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    dev = pipeline.get_device()
    rec = {"factor": FACTOR, "reps": args.reps, "warmup_calls": 2,
           "timing": "host clock around DeviceCool.coarsened (ends in a device synchronise); medians",
           "box": {"library": dev.lib.cs_version().decode(), "compute_units": dev.cu_count, "cpus_usable": len(os.sched_getaffinity(0)),
                   "loadavg_start": [round(x, 2) for x in os.getloadavg()]}}
    tables = {"bench": ("bench_200000_bins", bench_table, 1), "yeast": ("yeast_with_trans", yeast_table, 3)}
    for key in args.tables.split(","):
        name, make, host_reps = tables[key]
        rec[name] = measure(name, make(), args.reps, host_reps)
    rec["box"]["loadavg_end"] = [round(x, 2) for x in os.getloadavg()]
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
