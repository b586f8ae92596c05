"""Wall time of open_pairs' way from the text of a .pairs file to a resident table, on its two routes (profiles/pairs_parse_time.json):

- host:   DeviceCool.from_pairs_file(parse="host") -- io.read_pairs (pandas) chunk by chunk into the device binning;
- device: DeviceCool.from_pairs_file(parse="device") -- the body read in pieces, uploaded, parsed by cs_pairs_text_count /
  cs_pairs_text_parse (chromosight_amd/csrc/cs_pairs_text.hip), binned and merged piece by piece,

on the two inputs of tools/time_cload.py: the yeast fixture's 5.9 M pairs and the pairs of bench.py's synthetic table thinned to
--max-pairs contacts, each written as a seven-field .pairs file (readID chr1 pos1 chr2 pos2 strand1 strand2, a #chromsize: header)
to a temporary directory.  The file has just been written when it is read, so reads come from the page cache: the `read` share is
a lower bound on what a cold disk costs, and the same for both routes.

The device table is checked (exactly) against the host route's before anything is timed -- or, where the host route is beyond
--host-pair-limit, against the table the pairs were expanded from.  Times are a host clock around calls that end in a device
synchronise: warm-up calls first, then the median of --reps calls; the device call is also split, by clocks inside it, into file
read (inflate included for .gz), cutting the pieces at line ends, upload, the counting entry, the parsing entry and binning + merge
(medians of the same calls); `other` is what is left of the call.
Rates are the file's body bytes over the whole call: end-to-end figures, not a kernel's share of peak.  The host route runs
--host-reps times.  One process, its own time limit.

    python tools/time_pairs_parse.py [--out profiles/pairs_parse_time.json] [--reps 5] [--inputs yeast,bench] [--max-pairs 50000000]
"""
import argparse
import json
import os
import pathlib
import signal
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from chromosight_amd import cload, io as cio, pipeline  # noqa: E402
from tests.cload_util import chromsizes_of, pairs_of_table  # noqa: E402
from tools.time_cload import bench_table, yeast_table  # noqa: E402

STAGES = ("read", "cut", "upload", "count", "parse", "bin")


def write_pairs_file(path, sizes, cols):
    """A seven-field .pairs file of the pairs; returns the bytes of its header."""
    import pandas as pd
    names = np.asarray([n for n, _ in sizes])
    head = "## pairs format v1.0\n" + "".join(f"#chromsize: {n} {s}\n" for n, s in sizes) \
        + "#columns: readID chr1 pos1 chr2 pos2 strand1 strand2\n"
    with open(path, "w") as handle:
        handle.write(head)
        step = 1 << 22
        for a in range(0, cols[0].size, step):
            b = min(a + step, cols[0].size)
            ids = np.char.add("SRR1.", np.arange(a, b).astype(str))
            pd.DataFrame({0: ids, 1: names[cols[0][a:b]], 2: cols[1][a:b], 3: names[cols[2][a:b]], 4: cols[3][a:b], 5: "+", 6: "-"}).to_csv(
                handle, sep="\t", header=False, index=False)
    return len(head.encode())


def table_of(dcool):
    n = dcool.nnz
    return dcool.indptr.download(), dcool.indices.download()[:n].copy(), dcool.data.download().view(dcool.val_dtype)[:n].copy()


def same_tables(a, b):
    return a.nnz == b.nnz and a.val_dtype is b.val_dtype and a.dropped == b.dropped and \
        all(np.array_equal(x, y) for x, y in zip(table_of(a), table_of(b)))


def measure(name, cool, cap, args, workdir):
    dev = pipeline.get_device()
    sizes, binsize = chromsizes_of(cool), int(cool["binsize"])
    cols = cload.check_chunk(*pairs_of_table(cool, seed=1))
    n = int(cols[0].size)
    path = str(pathlib.Path(workdir) / f"{name}.pairs")
    t0 = time.perf_counter()
    head_bytes = write_pairs_file(path, sizes, cols)
    write_s = time.perf_counter() - t0
    del cols
    body_bytes = os.path.getsize(path) - head_bytes
    pf = cio.read_pairs(path)

    def device_route(timings=None):
        table = cload.pairs_file_device(pf, binsize, piece_bytes=args.piece_bytes, dev=dev, timings=timings)
        dev.sync()
        return table

    def host_route():
        table = pipeline.DeviceCool.from_pairs_file(path, binsize, parse="host", dev=dev)
        dev.sync()
        return table

    got = device_route()                            # warm-up (code objects, allocator) and the check
    host_runs = []
    if n <= args.host_pair_limit:
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            want = host_route()
            host_runs.append(time.perf_counter() - t0)
            if not same_tables(got, want):
                raise SystemExit(f"{name}: the device route's table differs from the host route's")
            del want
        checked = "the host route's table"
    else:
        cnt = np.asarray(cool["count"])
        indptr = np.searchsorted(np.asarray(cool["bin1_id"]), np.arange(got.n_bins + 1)).astype(np.int64)
        tab = table_of(got)
        if not (got.nnz == cnt.size and got.dropped == 0 and np.array_equal(tab[0], indptr)
                and np.array_equal(tab[1], np.asarray(cool["bin2_id"]).astype(np.int32)) and np.array_equal(tab[2], cnt.astype(got.val_dtype))):
            raise SystemExit(f"{name}: the device route's table differs from the table the pairs were expanded from")
        checked = "the table the pairs were expanded from (the host route is beyond --host-pair-limit)"
    pixels = got.nnz
    del got
    device_route()                                  # second warm-up
    runs, stages = [], {k: [] for k in STAGES}
    for _ in range(args.reps):
        timings = {}
        t0 = time.perf_counter()
        table = device_route(timings)
        runs.append(time.perf_counter() - t0)
        del table
        for k in STAGES:
            stages[k].append(timings.get(k, 0.0))
    dev_s = float(np.median(runs))
    host_s = float(np.median(host_runs)) if host_runs else None
    split = {k: round(float(np.median(v)), 5) for k, v in stages.items()}
    split["other"] = round(dev_s - sum(split.values()), 5)
    rec = {"pairs": n, "pixels": int(pixels), "binsize": binsize, "chromosomes": len(sizes), "file_bytes": head_bytes + body_bytes,
           "body_bytes": body_bytes, "bytes_per_line": round(body_bytes / max(n, 1), 1), "pieces": -(-body_bytes // args.piece_bytes),
           "write_file_s": round(write_s, 2), "checked_against": checked,
           "device_s": round(dev_s, 5), "device_runs_s": [round(x, 5) for x in runs], "device_split_s": split,
           "device_text_GBps": round(body_bytes / dev_s / 1e9, 3), "device_pairs_per_s": round(n / dev_s),
           "parse_entries_text_GBps": round(body_bytes / max(split["count"] + split["parse"], 1e-9) / 1e9, 2),
           "host_s": None if host_s is None else round(host_s, 3),
           "host_runs_s": [round(x, 3) for x in host_runs] if host_runs else "not measured: beyond --host-pair-limit",
           "host_pairs_per_s": None if host_s is None else round(n / host_s),
           "host_text_GBps": None if host_s is None else round(body_bytes / host_s / 1e9, 4),
           "device_faster": None if host_s is None else bool(dev_s < host_s),
           "speedup": None if host_s is None else round(host_s / dev_s, 1)}
    if cap:
        rec.update(cap)
    host_txt = "not measured" if host_s is None else f"{host_s:.2f} s ({n / host_s / 1e6:.2f} M pairs/s)"
    print(f"{name}: {n} pairs, {body_bytes / 1e6:.0f} MB: device {dev_s:.3f} s {split}, host {host_txt}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pairs_parse_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--inputs", default="yeast,bench")
    ap.add_argument("--max-pairs", type=int, default=50_000_000, help="contacts the bench table is thinned to")
    ap.add_argument("--host-pair-limit", type=int, default=20_000_000, help="pairs beyond which the host route is not run (minutes at 50 M)")
    ap.add_argument("--piece-bytes", type=int, default=cload.PIECE_BYTES)
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds after which the process is ended (SIGALRM)")
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    dev = pipeline.get_device()
    rec = {"reps": args.reps, "warmup_calls": 2, "piece_bytes": args.piece_bytes,
           "timing": "host clock around DeviceCool.from_pairs_file on either route, ending in a device synchronise; medians; the file "
                     "was written just before and is read from the page cache",
           "device_split": "clocks inside the device call: read = file reads (and inflate), cut = finding a piece's last line end and "
                           "carrying the rest, upload = pageable host-to-device copy of a piece, count / parse = the two entries (synchronous), bin = cs_pairs_count + cs_pairs_fill + merge",
           "box": {"library": dev.lib.cs_version().decode(), "compute_units": dev.cu_count, "cpus_usable": len(os.sched_getaffinity(0)),
                   "loadavg_start": [round(x, 2) for x in os.getloadavg()]}}
    inputs = {"yeast": ("yeast_5.9M_pairs", yeast_table), "bench": ("bench_200000_bins", bench_table)}
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as workdir:
        for key in args.inputs.split(","):
            name, make = inputs[key]
            cool, cap = make(args.max_pairs)
            rec[name] = measure(name, cool, cap, args, workdir)
            os.remove(pathlib.Path(workdir) / f"{name}.pairs")
            rec["box"]["loadavg_end"] = [round(x, 2) for x in os.getloadavg()]
            verdicts = [rec[n].get("device_faster") for n, _ in inputs.values() if n in rec]
            rec["device_faster_on_every_measured_input"] = bool(verdicts) and all(v is True for v in verdicts)
            rec["AUTO_PARSE_ON_DEVICE"] = {"rule": "True only if the device route is faster end to end on both inputs",
                                           "inputs_measured": len(verdicts),
                                           "value": len(verdicts) == len(inputs) and all(v is True for v in verdicts)}
            out.write_text(json.dumps(rec, indent=1) + "\n")                     # (after every input: a time limit keeps what is done)


if __name__ == "__main__":
    main()
