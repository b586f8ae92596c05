"""Wall time of opening a .cool's pixel table on the device (cs_inflate_chunks on the three stored columns + the finish pass
cs_table_from_columns_*) against the host route (per chunk: zlib.decompress, the inverse shuffle as a numpy transpose, a copy into
the column -- the loop of hdf5_lite.File.dataset -- then DeviceCool's constructor with its upload), profiles/cool_decode_time.json.

No .cool writer exists in this stack, so the dataset is synthesised in memory: the pixel table of bench.py's synthetic genome
(tools/synthetic_genome.make_cool: 200 000 bins of 2 kb), thinned to --pixels pixels (a seeded choice that keeps the order), its
columns stored as cooler stores them -- int64 bin ids, int32 counts -- cut into chunks of 1899 elements, shuffled and deflated at
level 6 with Python's zlib.  Compressing is the slow part: --cache keeps the compressed columns in an .npz.

The two routes alternate in one process, a warm-up of each first, --reps rounds, medians reported with every sample.  The device
time is a host clock around synchronous calls, from the compressed bytes in host memory to the resident table (upload included);
its result is compared with the host's, bit for bit, before anything is timed.  Rates: compressed bytes in, and resident table bytes
(row pointers, column bins, counts) out, over the device route's time.  open_cool of tests/golden/example.cool is timed both ways as
well, and the Python walk of its chunk B-trees (hdf5_lite.File.chunk_index), which the synthetic dataset does not cover: its cost on
a file of 10^5 chunks is the per-chunk cost there times 10^5 -- extrapolated, not measured.

The serial symbol loop's share of the device time comes from two runs under `rocprofv3 --kernel-trace --stats` of their own
(--profile-variant deflate / stored: the device route alone, on the level-6 columns and on the same columns at level 0, whose
chunks are stored blocks and take no symbol loop); --fold-profile DIR_DEFLATE DIR_STORED adds the kernels' times to the JSON.

    python tools/time_cool_decode.py [--pixels 8000000] [--reps 5] [--cache FILE.npz] [--out profiles/cool_decode_time.json]
"""
import argparse
import csv
import json
import pathlib
import sys
import time
import zlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from chromosight_amd import engine, hdf5_lite, pipeline  # noqa: E402

CHUNK = 1899
COLUMNS = (("bin1_id", np.int64), ("bin2_id", np.int64), ("count", np.int32))
EXAMPLE = ROOT / "tests" / "golden" / "example.cool"


def thinned_table(pixels):
    import chromosight_amd.kernels as ck
    from tools.synthetic_genome import make_cool
    cool, _ = make_cool(200_000, 1000, 2000, seed=2, template=np.asarray(ck.loops["kernels"][0], dtype=np.float64))
    n = int(np.asarray(cool["bin1_id"]).size)
    keep = np.sort(np.random.default_rng(9).choice(n, min(pixels, n), replace=False))
    table = {name: np.ascontiguousarray(np.asarray(cool[name])[keep], dtype=dtype) for name, dtype in COLUMNS}
    geometry = {k: np.asarray(cool[k]) for k in ("chrom_offset", "chrom_names", "bin_start", "bin_end", "weight")}
    geometry["binsize"] = np.int64(cool["binsize"])
    return table, geometry, n


def store_column(values, level):
    """(blob, offsets, nbytes) of `values` cut into CHUNK-element chunks (the last one padded with zeros), shuffled and deflated."""
    parts, sizes = [], []
    for a in range(0, values.size, CHUNK):
        chunk = values[a:a + CHUNK]
        if chunk.size < CHUNK:
            chunk = np.concatenate([chunk, np.zeros(CHUNK - chunk.size, dtype=values.dtype)])
        raw = chunk.view(np.uint8).reshape(CHUNK, values.dtype.itemsize).T.tobytes()
        parts.append(zlib.compress(raw, level))
        sizes.append(len(parts[-1]))
    nbytes = np.asarray(sizes, dtype=np.int64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64), nbytes


def index_of(dtype, length, offsets, nbytes):
    n = offsets.size
    return hdf5_lite.ChunkIndex(np.dtype(dtype), int(length), CHUNK, ((2, (np.dtype(dtype).itemsize,)), (1, (6,))), offsets, nbytes,
                                np.arange(n, dtype=np.int64) * CHUNK, np.zeros(n, dtype=np.uint32))


def dataset(pixels, cache):
    """{column: (blob, ChunkIndex)}, the geometry, and what the table was thinned from."""
    if cache and pathlib.Path(cache).exists():
        z = np.load(cache, allow_pickle=False)
        if int(z["pixels_asked"]) == pixels:
            stored = {name: (z[f"{name}_blob"], index_of(dtype, int(z["length"]), z[f"{name}_offsets"], z[f"{name}_nbytes"])) for name, dtype in COLUMNS}
            geometry = {k: z[f"geo_{k}"] for k in ("chrom_offset", "chrom_names", "bin_start", "bin_end", "weight", "binsize")}
            return stored, geometry, int(z["whole"]), float(z["compress_s"])
    table, geometry, whole = thinned_table(pixels)
    t0 = time.perf_counter()
    cols = {name: store_column(table[name], 6) for name, _ in COLUMNS}
    compress_s = time.perf_counter() - t0
    length = table["count"].size
    if cache:
        flat = {"pixels_asked": pixels, "length": length, "whole": whole, "compress_s": compress_s}
        for name, (blob, offsets, nbytes) in cols.items():
            flat[f"{name}_blob"], flat[f"{name}_offsets"], flat[f"{name}_nbytes"] = blob, offsets, nbytes
        flat.update({f"geo_{k}": v for k, v in geometry.items()})
        np.savez(cache, **flat)
    stored = {name: (cols[name][0], index_of(dtype, length, cols[name][1], cols[name][2])) for name, dtype in COLUMNS}
    return stored, geometry, whole, compress_s


def host_columns(stored):
    """The loop of hdf5_lite.File.dataset over every chunk of every column."""
    out = {}
    for name, (blob, idx) in stored.items():
        col = np.zeros(idx.length, dtype=idx.dtype)
        buf = blob.tobytes() if not isinstance(blob, bytes) else blob
        for off, nb, start in zip(idx.offsets.tolist(), idx.nbytes.tolist(), idx.starts.tolist()):
            raw = zlib.decompress(buf[off:off + nb])
            raw = np.frombuffer(raw, dtype=np.uint8).reshape(idx.dtype.itemsize, -1).T.tobytes()
            vals = np.frombuffer(raw, dtype=idx.dtype, count=idx.chunk)
            m = min(idx.chunk, idx.length - start)
            col[start:start + m] = vals[:m]
        out[name] = col
    return out


def host_route(stored, geometry, dev):
    t0 = time.perf_counter()
    cool = host_columns(stored)
    for key in ("bin1_id", "bin2_id"):                     # io._load
        if cool[key].size and cool[key].max() < 2 ** 31:
            cool[key] = cool[key].astype(np.int32)
    t1 = time.perf_counter()
    cool.update(geometry, weight=None)
    dcool = pipeline.DeviceCool(cool, dev)
    dev.sync()
    return dcool, t1 - t0, time.perf_counter() - t1


def device_route(stored, n_bins, dev):
    t0 = time.perf_counter()
    cols = {name: engine.run_inflate_chunks(dev, blob, idx)[0] for name, (blob, idx) in stored.items()}
    t1 = time.perf_counter()
    res = engine.run_table_from_columns(dev, cols["bin1_id"], cols["bin2_id"], cols["count"], stored["count"][1].length, n_bins)
    return res, t1 - t0, time.perf_counter() - t1


def same_table(res, dcool):
    n = dcool.nnz
    return (res["nnz"] == n and res["val_dtype"] is dcool.val_dtype and res["upper"] == dcool.upper
            and res["indptr"].download().tobytes() == dcool.indptr.download().tobytes()
            and res["indices"].download()[:n].tobytes() == dcool.indices.download()[:n].tobytes()
            and res["data"].download()[:n].tobytes() == dcool.data.download()[:n].tobytes())


def med(samples):
    return {"median_s": round(float(np.median(samples)), 6), "samples_s": [round(float(x), 6) for x in samples]}


def kernel_stats(directory):
    """{kernel name: total ns} of a rocprofv3 --kernel-trace --stats output directory."""
    out = {}
    for path in pathlib.Path(directory).rglob("*kernel_stats.csv"):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = out.get(row["Name"], 0) + int(float(row["TotalDurationNs"]))
    return out


def fold_profile(out_path, dir_deflate, dir_stored):
    result = json.loads(pathlib.Path(out_path).read_text())
    pick = lambda stats, word: sum(ns for name, ns in stats.items() if word in name)          # noqa: E731
    a, b = kernel_stats(dir_deflate), kernel_stats(dir_stored)
    inflate, stored = pick(a, "inflate_kernel"), pick(b, "inflate_kernel")
    finish = pick(a, "table_check_kernel") + pick(a, "table_fill_kernel")
    every = sum(a.values())
    result["kernel_trace"] = {
        "method": "rocprofv3 --kernel-trace --stats, one run per variant, the device route alone (1 warm-up + 3 calls each); stored = the same "
                  "columns at level 0: stored blocks, the same copies, checksum and unshuffle, no symbol loop",
        "inflate_kernel_ns_level6": inflate, "inflate_kernel_ns_level0": stored, "finish_kernels_ns": finish, "all_kernels_ns_level6": every,
        "symbol_loop_share_of_kernel_time": round((inflate - stored) / every, 4) if every else None,
    }
    pathlib.Path(out_path).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=8_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "cool_decode_time.json"))
    ap.add_argument("--prepare-only", action="store_true", help="build the cache and stop (no GPU)")
    ap.add_argument("--profile-variant", choices=("deflate", "stored"), default=None)
    ap.add_argument("--fold-profile", nargs=2, metavar=("DIR_DEFLATE", "DIR_STORED"), default=None)
    args = ap.parse_args()
    if args.fold_profile:
        return fold_profile(args.out, *args.fold_profile)
    stored, geometry, whole, compress_s = dataset(args.pixels, args.cache)
    if args.prepare_only:
        return print(f"{stored['count'][1].length} pixels of {whole}, compressed in {compress_s:.1f} s")
    dev = pipeline.get_device()
    n_bins = int(geometry["chrom_offset"][-1])
    if args.profile_variant:
        if args.profile_variant == "stored":
            hc = host_columns(stored)
            stored = {}
            for name, dtype in COLUMNS:
                blob, offsets, nbytes = store_column(hc[name], 0)
                stored[name] = (blob, index_of(dtype, hc[name].size, offsets, nbytes))
        for _ in range(4):
            device_route(stored, n_bins, dev)
        return print(f"profile variant {args.profile_variant}: done")

    pixels = stored["count"][1].length
    in_bytes = int(sum(int(idx.nbytes.sum()) for _, idx in stored.values()))
    res, _, _ = device_route(stored, n_bins, dev)                                 # warm-up of both, and the check
    dcool, _, _ = host_route(stored, geometry, dev)
    if not same_table(res, dcool):
        raise SystemExit("the device route's table differs from the host route's")
    out_bytes = int(dcool.indptr.nbytes + pixels * (4 + np.dtype(dcool.val_dtype).itemsize))
    del res, dcool
    d_dec, d_fin, h_dec, h_con = [], [], [], []
    for _ in range(args.reps):
        r, a, b = device_route(stored, n_bins, dev)
        d_dec.append(a), d_fin.append(b)
        del r
        r, a, b = host_route(stored, geometry, dev)
        h_dec.append(a), h_con.append(b)
        del r
    d_tot, h_tot = np.add(d_dec, d_fin), np.add(h_dec, h_con)
    result = {
        "tool": "tools/time_cool_decode.py", "device": "MI355X", "chunk_elems": CHUNK, "filters": "shuffle + gzip 6",
        "synthetic": {
            "pixels": pixels, "pixels_of_the_whole_table": whole, "chunks": int(sum(idx.offsets.size for _, idx in stored.values())),
            "compressed_bytes": in_bytes, "stored_column_bytes": pixels * 20, "resident_table_bytes": out_bytes,
            "compress_with_python_zlib_s": round(compress_s, 2),
            "device": {"total": med(d_tot), "decode_3_columns_upload_included": med(d_dec), "finish": med(d_fin)},
            "host": {"total": med(h_tot), "per_chunk_loop_3_columns": med(h_dec), "constructor_and_upload": med(h_con)},
            "host_over_device": round(float(np.median(h_tot) / np.median(d_tot)), 1),
            "device_input_GB_per_s": round(in_bytes / float(np.median(d_tot)) / 1e9, 3),
            "device_output_GB_per_s": round(out_bytes / float(np.median(d_tot)) / 1e9, 3),
            "device_pixels_per_s": round(pixels / float(np.median(d_tot))), "host_pixels_per_s": round(pixels / float(np.median(h_tot))),
        },
    }
    # open_cool of the example, both ways, alternating
    dev_t, host_t = [], []
    for k in range(args.reps + 1):
        for decode, sink in (("device", dev_t), ("host", host_t)):
            t0 = time.perf_counter()
            d = pipeline.open_cool(str(EXAMPLE), decode=decode)
            dev.sync()
            if k:
                sink.append(time.perf_counter() - t0)
            del d
    walk, chunks = [], 0
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        with hdf5_lite.File(EXAMPLE) as f:
            chunks = sum(f.chunk_index(f"/pixels/{name}").offsets.size for name, _ in COLUMNS)
        if k:
            walk.append(time.perf_counter() - t0)
    per_chunk = float(np.median(walk)) / max(chunks, 1)
    result["example_cool"] = {
        "open_cool_device": med(dev_t), "open_cool_host": med(host_t), "host_over_device": round(float(np.median(host_t) / np.median(dev_t)), 2),
        "chunk_index_3_columns": dict(med(walk), chunks=chunks, note="opens the file, resolves the paths and walks the three chunk B-trees"),
        "chunk_index_1e5_chunks_s_EXTRAPOLATED_not_measured": round(per_chunk * 1e5, 3),
    }
    pathlib.Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
