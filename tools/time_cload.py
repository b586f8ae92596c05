"""Wall time of the binning of read pairs on the device (DeviceCool.from_pairs: cs_pairs_count / cs_pairs_fill) against the route a
user has without it -- binning on the host (the numpy oracle of tests/cload_util.py) and uploading the table with DeviceCool(...)
-- on two inputs (profiles/cload_time.json):

- the yeast fixture (tests/golden/yeast_cool.npz) expanded into its 5.9 M read pairs (tests/cload_util.pairs_of_table);
- the table of bench.py's synthetic genome (tools/synthetic_genome.make_cool: 200 000 bins of 2 kb in 23 chromosomes), its counts
  thinned binomially (seeded) to about --max-pairs contacts so that the host arrays fit, then expanded the same way.  The cap and
  the pairs it left are recorded.

The device result is checked (exactly) against the table the pairs were expanded from before anything is timed.  The device time is
a host clock around a call that ends in a device synchronise (cs_pairs_fill is synchronous): warm-up calls first, then the median
of --reps calls; reported twice -- from host columns (the upload of 24 bytes per pair included) and from columns already resident.
The rate is the input columns' bytes over the call time: an end-to-end figure (allocations, the sort's passes and the host
synchronisations included), not a kernel's share of peak.  The host route is run --host-reps times where the chunk is within
--host-pair-limit, else it is "not measured".  One process, its own time limit.

    python tools/time_cload.py [--out profiles/cload_time.json] [--reps 7] [--inputs yeast,bench] [--max-pairs 50000000]
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

from chromosight_amd import cload, pipeline  # noqa: E402
from tests.cload_util import chromsizes_of, oracle_cload, pairs_of_table  # noqa: E402


def yeast_table(max_pairs):
    return dict(np.load(ROOT / "tests" / "golden" / "yeast_cool.npz", allow_pickle=False)), None


def bench_table(max_pairs):
    import chromosight_amd.kernels as ck
    from tools.synthetic_genome import make_cool
    template = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    cool, _ = make_cool(200_000, 1000, 2000, seed=2, template=template)
    cnt = np.asarray(cool["count"]).astype(np.int64)
    total = int(cnt.sum())
    if total > max_pairs:                                   # seeded binomial thinning: the table's shape, fewer contacts
        cnt = np.random.default_rng(9).binomial(cnt, max_pairs / total)
    keep = cnt > 0
    thin = dict(cool)
    thin["bin1_id"], thin["bin2_id"], thin["count"] = np.asarray(cool["bin1_id"])[keep], np.asarray(cool["bin2_id"])[keep], cnt[keep]
    return thin, {"max_pairs": int(max_pairs), "contacts_of_the_whole_table": total}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
        del r
    return float(np.median(out)), [round(x, 5) for x in out]


def measure(name, cool, cap, reps, host_reps, host_pair_limit):
    dev = pipeline.get_device()
    sizes, binsize = chromsizes_of(cool), int(cool["binsize"])
    geo = cload.bin_geometry(sizes, binsize)
    t0 = time.perf_counter()
    cols = cload.check_chunk(*pairs_of_table(cool, seed=1))
    expand_s = time.perf_counter() - t0
    n = int(cols[0].size)
    binned = pipeline.DeviceCool.from_pairs(cols, geo, binsize, dev=dev)              # warm-up (code objects, allocator) and the check
    cnt = np.asarray(cool["count"])
    dtype = np.float32 if cnt.max() < (1 << 24) else np.float64
    indptr = np.searchsorted(np.asarray(cool["bin1_id"]), np.arange(binned.n_bins + 1)).astype(np.int64)
    same = (binned.nnz == cnt.size and binned.val_dtype is dtype and binned.dropped == 0 and np.array_equal(binned.indptr.download(), indptr)
            and np.array_equal(binned.indices.download()[:cnt.size], np.asarray(cool["bin2_id"]).astype(np.int32))
            and np.array_equal(binned.data.download()[:cnt.size], cnt.astype(dtype)))
    if not same:
        raise SystemExit(f"{name}: the binned pairs differ from the table they were expanded from")
    pixels = binned.nnz
    del binned
    pipeline.DeviceCool.from_pairs(cols, geo, binsize, dev=dev)
    up_s, up_all = timed(lambda: pipeline.DeviceCool.from_pairs(cols, geo, binsize, dev=dev), reps)
    d_cols = [dev.to_device(c) for c in cols]
    dev.sync()
    res_s, res_all = timed(lambda: cload.pairs_csr_resident(dev, geo, tuple(d_cols), n), reps)
    del d_cols

    def host_route():
        want = oracle_cload(sizes, binsize, *cols)
        up = pipeline.DeviceCool({k: v for k, v in want.items() if k not in ("val_dtype", "dropped")}, dev)
        dev.sync()
        return up

    if n <= host_pair_limit:
        host_s, host_all = timed(host_route, host_reps)
    else:
        host_s, host_all = None, "not measured: the chunk is beyond --host-pair-limit"
    in_bytes = 24 * n
    rec = {"pairs": n, "pixels": int(pixels), "bins": int(geo.offsets[-1]), "chromosomes": len(geo.names), "binsize": binsize,
           "count_dtype": np.dtype(dtype).name, "equal_to_the_expanded_table": True, "expand_on_host_s": round(expand_s, 2),
           "device_with_upload_s": round(up_s, 5), "device_with_upload_runs_s": up_all,
           "device_resident_s": round(res_s, 5), "device_resident_runs_s": res_all,
           "host_route_s": None if host_s is None else round(host_s, 3), "host_route_runs_s": host_all,
           "speedup_with_upload": None if host_s is None else round(host_s / up_s, 1),
           "speedup_resident": None if host_s is None else round(host_s / res_s, 1),
           "input_bytes": in_bytes, "end_to_end_input_rate_with_upload_GBps": round(in_bytes / up_s / 1e9, 2),
           "end_to_end_input_rate_resident_GBps": round(in_bytes / res_s / 1e9, 2),
           "pairs_per_s_resident": round(n / res_s)}
    if cap:
        rec.update(cap)
    host_txt = "not measured" if host_s is None else f"{host_s:.2f} s"
    print(f"{name}: {n} pairs -> {pixels} pixels, device {up_s * 1e3:.1f} ms with upload, {res_s * 1e3:.1f} ms resident, host route {host_txt}",
          flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cload_time.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--inputs", default="yeast,bench")
    ap.add_argument("--max-pairs", type=int, default=50_000_000, help="contacts the bench table is thinned to (host arrays: 24 bytes per pair, twice)")
    ap.add_argument("--host-pair-limit", type=int, default=100_000_000, help="pairs beyond which the host route is not run")
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds after which the process is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    dev = pipeline.get_device()
    rec = {"reps": args.reps, "warmup_calls": 2,
           "timing": "host clock around DeviceCool.from_pairs / cload.pairs_csr_resident (both end in a device synchronise); medians",
           "host_route": "tests/cload_util.oracle_cload of the same columns + DeviceCool(table) + synchronise",
           "routes": "global radix sort of packed keys (the only route built)",
           "box": {"library": dev.lib.cs_version().decode(), "compute_units": dev.cu_count, "cpus_usable": len(os.sched_getaffinity(0)),
                   "loadavg_start": [round(x, 2) for x in os.getloadavg()]}}
    inputs = {"yeast": ("yeast_5.9M_pairs", yeast_table), "bench": ("bench_200000_bins", bench_table)}
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for key in args.inputs.split(","):
        name, make = inputs[key]
        cool, cap = make(args.max_pairs)
        rec[name] = measure(name, cool, cap, args.reps, args.host_reps, args.host_pair_limit)
        rec["box"]["loadavg_end"] = [round(x, 2) for x in os.getloadavg()]
        out.write_text(json.dumps(rec, indent=1) + "\n")                     # (after every input: a time limit keeps what is done)


if __name__ == "__main__":
    main()
