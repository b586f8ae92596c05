"""Wall time of DeviceCool.subsampled with sampler="device" against the numpy path on the same box (profiles/subsample_time.json):

- a synthetic hg38-proportioned table of ~40 M pixels (tools/synthetic_inter.make_trans_cool: 24 chromosomes, intra band and
  sparse trans contacts), intra-only and with --inter (300 blocks), both samplers;
- a ~310 M-pixel table (24 chromosomes in hg38 proportions, a band of 1000 diagonals), device only.

    python tools/time_subsample.py [--out profiles/subsample_time.json] [--big-diags 1000] [--reps 3]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from chromosight_amd import pipeline  # noqa: E402
from tools.synthetic_genome import genome_sizes  # noqa: E402
from tools.synthetic_inter import make_trans_cool  # noqa: E402


def band_cool(total_bins=310_000, diags=1000, seed=3):
    """Decoded-cool dictionary: hg38-proportioned chromosomes, every pixel of the first `diags` diagonals with a count in 1..39."""
    rng = np.random.default_rng(seed)
    mb = np.asarray(list(np.asarray(genome_sizes(1_000_000))[:23]) + [57 * 1_000_000 / 3_100], dtype=np.float64)
    sizes = np.maximum((mb / mb.sum() * total_bins).astype(np.int64), 256)
    off = np.concatenate([[0], np.cumsum(sizes)])
    b1l, b2l = [], []
    d = np.arange(diags, dtype=np.int32)
    for c, m in enumerate(sizes.tolist()):
        rows = np.repeat(np.arange(m, dtype=np.int32), diags)
        cols = rows + np.tile(d, m)
        ok = cols < m
        b1l.append(rows[ok] + np.int32(off[c]))
        b2l.append(cols[ok] + np.int32(off[c]))
    b1, b2 = np.concatenate(b1l), np.concatenate(b2l)
    n = int(off[-1])
    return {"binsize": 10_000, "chrom_offset": off, "chrom_names": np.array([f"chr{c + 1}" for c in range(sizes.size)]),
            "bin1_id": b1, "bin2_id": b2, "count": rng.integers(1, 40, size=b1.size, dtype=np.int32), "weight": np.ones(n),
            "bin_start": np.concatenate([np.arange(s) * 10_000 for s in sizes]),
            "bin_end": np.concatenate([(np.arange(s) + 1) * 10_000 for s in sizes])}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
        del r
    return float(np.median(out)), [round(x, 4) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "subsample_time.json"))
    ap.add_argument("--big-diags", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    rec = {"sample": 0.5, "seed": 1}
    cool, _ = make_trans_cool(seed=5)
    dc = pipeline.DeviceCool(cool)
    mid = {"pixels": dc.nnz, "chromosomes": dc.n_chrom}
    for inter in (False, True):
        tag = "inter" if inter else "intra"
        dc.subsampled(0.5, seed=1, inter=inter, sampler="device")          # warm-up (code objects, allocator)
        dev_s, dev_all = timed(lambda: dc.subsampled(0.5, seed=1, inter=inter, sampler="device"), args.reps)
        np_s, _ = timed(lambda: dc.subsampled(0.5, seed=1, inter=inter), 1)
        mid[tag] = {"device_s": round(dev_s, 4), "device_runs_s": dev_all, "numpy_s": round(np_s, 3), "speedup": round(np_s / dev_s, 1)}
        print(f"{dc.nnz} pixels, {tag}: device {dev_s:.4f} s, numpy {np_s:.2f} s, x{np_s / dev_s:.0f}", flush=True)
    rec["hg38_synthetic"] = mid
    del dc, cool
    big = pipeline.DeviceCool(band_cool(diags=args.big_diags))
    big.subsampled(0.5, seed=1, inter=True, sampler="device")
    dev_s, dev_all = timed(lambda: big.subsampled(0.5, seed=1, inter=True, sampler="device"), args.reps)
    rec["band_device_only"] = {"pixels": big.nnz, "chromosomes": big.n_chrom, "inter": True, "device_s": round(dev_s, 4),
                               "device_runs_s": dev_all}
    print(f"{big.nnz} pixels, inter: device {dev_s:.4f} s", flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
