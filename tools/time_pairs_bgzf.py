"""Wall time of DeviceCool.from_pairs_file on a bgzip-compressed .pairs.gz with the members inflated on the device (inflate="device":
cs_bgzf_inflate, chromosight_amd/csrc/cs_inflate.hip) against the route that inflates on one host thread (profiles/pairs_bgzf_time.json).

Inputs: the two of tools/time_pairs_parse.py (the yeast fixture's 5.9 M pairs, 20 M pairs of bench.py's genome) as seven-field .pairs
text, written as BGZF at level 6 in blocks of 65 280 bytes of text plus the end marker -- what bgzip writes -- to a temporary directory.
The files have just been written when they are read, so reads come from the page cache.

Every measurement runs in a child process of its own, and the two trees take turns (--rounds): a child on --parent-tree (an export of
the parent commit, built: its from_pairs_file(path_gz, parse="device") is the baseline; without the option no baseline is measured)
and a child on this tree, which first checks the table of inflate="device" exactly against that of inflate="host", then times
inflate="device" (split by the clocks inside the call into read, inflate, upload, count, parse, bin, cut; `other` is the rest),
inflate="host" beside it, and the inflate entry alone: every member of the file, resident, in one synchronous cs_bgzf_inflate call
(descriptor upload and status download included), with its rates of compressed input and text output.  Times are a host clock around
calls that end in a device synchronise: --warmup calls first, then --reps calls; the figure of a route is the median over the
repetitions of all its children.

The rule for inflate="auto" (pipeline.AUTO_INFLATE_ON_DEVICE): True only if, on both inputs, the device route's median lies below the
baseline's by more than the baseline's own run-to-run spread (max - min of its repetitions).

    python tools/time_pairs_bgzf.py --parent-tree /path/to/built/export [--out profiles/pairs_bgzf_time.json] [--reps 3] [--rounds 2]
"""
import argparse
import json
import os
import pathlib
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
STAGES = ("read", "inflate", "upload", "count", "parse", "bin", "cut")
BLOCK = 65280


# ---- a child: one tree, one file -----------------------------------------------------------------------------------------------------
def _table_of(dcool):
    n = dcool.nnz
    return dcool.indptr.download(), dcool.indices.download()[:n].copy(), dcool.data.download().view(dcool.val_dtype)[:n].copy()


def child(args):
    sys.path.insert(0, args.tree)
    from chromosight_amd import pipeline
    assert pathlib.Path(pipeline.__file__).resolve().parents[1] == pathlib.Path(args.tree).resolve(), "the package of another tree was imported"
    dev = pipeline.get_device()
    load = pipeline.DeviceCool.from_pairs_file

    def timed(call, reps):
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            table = call()
            dev.sync()
            runs.append(time.perf_counter() - t0)
            del table
        return runs

    out = {}
    if args.child == "parent":
        call = lambda: load(args.path, args.binsize, parse="device", dev=dev)          # noqa: E731
        timed(call, args.warmup)
        out["parent_runs_s"] = timed(call, args.reps)
    else:
        from chromosight_amd import cload, engine, io as cio
        pf = cio.read_pairs(args.path)
        device = load(args.path, args.binsize, parse="device", inflate="device", dev=dev)
        host = load(args.path, args.binsize, parse="device", inflate="host", dev=dev)
        same = device.nnz == host.nnz and device.val_dtype is host.val_dtype and device.dropped == host.dropped and \
            all(np.array_equal(x, y) for x, y in zip(_table_of(device), _table_of(host)))
        if not same:
            raise SystemExit(f"{args.path}: the table of inflate='device' differs from that of inflate='host'")
        out["pixels"] = int(device.nnz)
        del device, host
        stages = {k: [] for k in STAGES}

        def device_call():
            timings = {}
            table = cload.pairs_file_device(pf, args.binsize, dev=dev, timings=timings, inflate="device")
            stages_now.append(timings)
            return table

        stages_now = []
        timed(device_call, max(args.warmup - 1, 0))
        stages_now.clear()
        out["device_runs_s"] = timed(device_call, args.reps)
        for timings in stages_now:
            for k in STAGES:
                stages[k].append(timings.get(k, 0.0))
        out["device_stage_runs_s"] = stages
        out["host_inflate_runs_s"] = timed(lambda: load(args.path, args.binsize, parse="device", inflate="host", dev=dev), args.host_reps)
        # the entry alone: the whole file resident, every member in one call
        data = np.fromfile(args.path, dtype=np.uint8)
        blocks = list(cload.bgzf_blocks(data))
        isizes = np.asarray([b.isize for b in blocks], dtype=np.int64)
        out_offsets = np.concatenate([[0], np.cumsum(isizes)[:-1]])
        text_bytes = int(isizes.sum())
        d_file, d_text = dev.to_device(data), dev.empty(max(text_bytes, 1), np.uint8)
        entry = lambda: engine.run_bgzf_inflate(dev, d_file, data.size, [b.body_offset for b in blocks], [b.body_bytes for b in blocks],        # noqa: E731
                                                out_offsets, isizes, d_text, text_bytes)
        timed(entry, 2)
        out["inflate_entry_runs_s"] = timed(entry, max(args.reps, 5))
        out["blocks"], out["compressed_bytes"], out["text_bytes"] = len(blocks), int(data.size), text_bytes
    out["library"], out["compute_units"] = dev.lib.cs_version().decode(), dev.cu_count
    print("RESULT " + json.dumps(out), flush=True)


# ---- the parent process: files, children, the record ---------------------------------------------------------------------------------
def _compress_span(span):
    from tests.bgzf_util import block
    return b"".join(block(span[at:at + BLOCK]) for at in range(0, len(span), BLOCK))


def write_bgzf(text_path, gz_path, workers):
    """The text file as BGZF: level 6, blocks of 65 280 bytes, the end marker."""
    import multiprocessing
    from tests.bgzf_util import END_MARKER
    per_task = 64 * BLOCK

    def spans():
        with open(text_path, "rb") as handle:
            while True:
                span = handle.read(per_task)
                if not span:
                    return
                yield span

    with multiprocessing.get_context("fork").Pool(workers) as pool, open(gz_path, "wb") as out:
        for packed in pool.imap(_compress_span, spans()):
            out.write(packed)
        out.write(END_MARKER)


def run_child(role, tree, path, binsize, args):
    cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--child", role, "--tree", str(tree), "--path", str(path), "--binsize", str(binsize),
           "--reps", str(args.reps), "--warmup", str(args.warmup), "--host-reps", str(args.host_reps)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_time_limit)
    if res.returncode != 0:
        raise SystemExit(f"the {role} child ended with {res.returncode}:\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    line = [x for x in res.stdout.splitlines() if x.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def med(values):
    return round(float(np.median(values)), 5)


def measure(name, cool, cap, args, workdir):
    from chromosight_amd import cload
    from tests.cload_util import chromsizes_of, pairs_of_table
    from tools.time_pairs_parse import write_pairs_file
    sizes, binsize = chromsizes_of(cool), int(cool["binsize"])
    cols = cload.check_chunk(*pairs_of_table(cool, seed=1))
    text_path, gz_path = pathlib.Path(workdir) / f"{name}.pairs", pathlib.Path(workdir) / f"{name}.pairs.gz"
    t0 = time.perf_counter()
    write_pairs_file(str(text_path), sizes, cols)
    n = int(cols[0].size)
    del cols
    write_bgzf(text_path, gz_path, args.workers)
    write_s = time.perf_counter() - t0
    text_file_bytes = os.path.getsize(text_path)
    os.remove(text_path)
    parent_runs, device_runs, host_runs, entry_runs = [], [], [], []
    stage_runs = {k: [] for k in STAGES}
    this = {}
    for _ in range(args.rounds):
        if args.parent_tree:
            parent_runs += run_child("parent", args.parent_tree, gz_path, binsize, args)["parent_runs_s"]
        this = run_child("this", ROOT, gz_path, binsize, args)
        device_runs += this["device_runs_s"]
        host_runs += this["host_inflate_runs_s"]
        entry_runs += this["inflate_entry_runs_s"]
        for k in STAGES:
            stage_runs[k] += this["device_stage_runs_s"][k]
    os.remove(gz_path)
    dev_s, entry_s = med(device_runs), med(entry_runs)
    split = {k: med(v) for k, v in stage_runs.items()}
    split["other"] = round(dev_s - sum(split.values()), 5)
    rec = {"pairs": n, "pixels": this["pixels"], "binsize": binsize, "text_bytes": text_file_bytes, "gz_bytes": this["compressed_bytes"],
           "blocks": this["blocks"], "write_files_s": round(write_s, 2), "checked_against": "the table of inflate='host', exactly, in every child",
           "device_s": dev_s, "device_runs_s": [round(x, 5) for x in device_runs], "device_split_s": split,
           "host_inflate_same_process_s": med(host_runs), "host_inflate_runs_s": [round(x, 5) for x in host_runs],
           "inflate_entry_s": entry_s, "inflate_entry_runs_s": [round(x, 5) for x in entry_runs],
           "inflate_entry_compressed_GBps": round(this["compressed_bytes"] / entry_s / 1e9, 2),
           "inflate_entry_text_GBps": round(this["text_bytes"] / entry_s / 1e9, 2)}
    if parent_runs:
        spread = max(parent_runs) - min(parent_runs)
        rec.update({"parent_s": med(parent_runs), "parent_runs_s": [round(x, 5) for x in parent_runs], "parent_spread_s": round(spread, 5),
                    "device_below_parent_by_more_than_its_spread": bool(dev_s < med(parent_runs) - spread),
                    "speedup_over_parent": round(med(parent_runs) / dev_s, 2)})
    if cap:
        rec.update(cap)
    print(f"{name}: {json.dumps(rec)}", flush=True)
    return rec, this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pairs_bgzf_time.json"))
    ap.add_argument("--parent-tree", default=None, help="a built export of the parent commit: the baseline")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--inputs", default="yeast,bench")
    ap.add_argument("--max-pairs", type=int, default=20_000_000, help="contacts the bench table is thinned to")
    ap.add_argument("--workers", type=int, default=min(16, len(os.sched_getaffinity(0))), help="processes that compress the inputs")
    ap.add_argument("--time-limit", type=int, default=1100, help="seconds after which the process is ended (SIGALRM)")
    ap.add_argument("--child-time-limit", type=int, default=400)
    ap.add_argument("--child", choices=("parent", "this"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--path", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--binsize", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    signal.alarm(args.time_limit)
    sys.path.insert(0, str(ROOT))
    from tools.time_cload import bench_table, yeast_table
    rec = {"reps_per_child": args.reps, "host_reps_per_child": args.host_reps, "warmup_calls": args.warmup, "rounds": args.rounds,
           "timing": "host clock around DeviceCool.from_pairs_file(path_gz, parse='device', ...) ending in a device synchronise; one child "
                     "process per tree and round, the trees taking turns; medians over all repetitions; the files were written just before "
                     "and are read from the page cache",
           "inputs": "seven-field .pairs text as BGZF: zlib level 6, 65 280 bytes of text per member, the end marker",
           "baseline": "parent_s: the parent commit's from_pairs_file(path_gz, parse='device') from a built export of its tree" if args.parent_tree
                       else "not measured: no --parent-tree",
           "device_split": "clocks inside the device call: read = walking the members and inflating the header's on the host, inflate = "
                           "cs_bgzf_inflate (synchronous), upload = the pieces' compressed bytes and the carry, count / parse = the two "
                           "parser entries, bin = cs_pairs_count + cs_pairs_fill + merge, cut = choosing a piece's members and fetching the carry",
           "box": {"cpus_usable": len(os.sched_getaffinity(0)), "loadavg_start": [round(x, 2) for x in os.getloadavg()]}}
    inputs = {"yeast": ("yeast_5.9M_pairs", yeast_table), "bench": ("bench_200000_bins", bench_table)}
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with tempfile.TemporaryDirectory() as workdir:
        for key in args.inputs.split(","):
            name, make = inputs[key]
            cool, cap = make(args.max_pairs)
            rec[name], this = measure(name, cool, cap, args, workdir)
            rec["box"].update({"library": this["library"], "compute_units": this["compute_units"],
                               "loadavg_end": [round(x, 2) for x in os.getloadavg()]})
            verdicts = [rec[n].get("device_below_parent_by_more_than_its_spread") for n, _ in inputs.values() if n in rec]
            rec["AUTO_INFLATE_ON_DEVICE"] = {"rule": "True only if the device route's median is below the parent's by more than the parent's own "
                                                     "spread (max - min of its repetitions) on both inputs",
                                             "inputs_measured": sum(v is not None for v in verdicts),
                                             "value": len(verdicts) == len(inputs) and all(v is True for v in verdicts)}
            out.write_text(json.dumps(rec, indent=1) + "\n")                     # (after every input: a time limit keeps what is done)


if __name__ == "__main__":
    main()
