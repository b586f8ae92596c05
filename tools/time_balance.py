"""Wall time of ICE balancing on the device (balance.ice_balance, cis mode, the reference's arguments) on the C4 synthetic
genome (200 000 bins, its weights dropped):  python tools/time_balance.py [--bins N] [--repeats R] [--out FILE]

Every call is synchronous (cs_ice_balance ends with a stream synchronisation), so a host clock around it is the call's time.
Per iteration: (T(max_iters = all) - T(max_iters = 1)) / (longest span's iterations - 1) -- the difference removes the one-off
part (CSC permutation, filter marginals, host medians, uploads).  Effective bytes of an iteration: what the marginal pass
must read for every kept pixel of a span still iterating -- column index (4 B) and count (4 or 8 B), once from the row
side and once from the column side -- summed over the iterations every span ran, over the same time difference."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

HBM_ROOF = 6.29e12        # MI355X measured copy rate (8.0 TB/s spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from synthetic_genome import make_cool
    from chromosight_amd import pipeline
    from chromosight_amd.balance import ice_balance
    t0 = time.perf_counter()
    cool, _ = make_cool(total_bins=a.bins)
    cool.pop("weight")
    gen_s = time.perf_counter() - t0
    dcool = pipeline.DeviceCool(cool)
    kw = dict(cis_only=True, mad_max=5, min_nnz=10, ignore_diags=2, max_iters=200)

    def timed(**extra):
        t = time.perf_counter()
        w, info = ice_balance(dcool, **dict(kw, **extra))
        return (time.perf_counter() - t) * 1e3, w, info

    timed()                                           # code objects, allocator
    full = [timed() for _ in range(a.repeats)]
    one = [timed(max_iters=1) for _ in range(a.repeats)]
    t_full = float(np.median([x[0] for x in full]))
    t_one = float(np.median([x[0] for x in one]))
    w, info = full[0][1], full[0][2]
    assert all(x[1].tobytes() == w.tobytes() for x in full), "weights differ between calls"
    its = np.asarray(info["iterations"], dtype=np.int64)
    # kept pixels of every span (cis, |bin2 - bin1| >= 2)
    b1, b2 = np.asarray(cool["bin1_id"], dtype=np.int64), np.asarray(cool["bin2_id"], dtype=np.int64)
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))
    kept = (b2 - b1 >= 2) & (chrom[b1] == chrom[b2])
    per_span = np.bincount(chrom[b1[kept]], minlength=off.size - 1)
    vbytes = np.dtype(dcool.val_dtype).itemsize
    bytes_iter = per_span * 2 * (4 + vbytes)
    moved = float(np.sum((its - 1) * bytes_iter))
    span_ms = t_full - t_one
    rate = moved / (span_ms * 1e-3) if span_ms > 0 else float("nan")
    res = {
        "bins": int(dcool.n_bins), "pixels": int(dcool.nnz), "kept_pixels": int(kept.sum()), "val_dtype": np.dtype(dcool.val_dtype).name,
        "spans": int(its.size), "iterations_per_span": its.tolist(), "iterations_max": int(its.max()),
        "converged": bool(np.all(info["converged"])), "nan_bins": int(np.isnan(w).sum()),
        "total_ms": round(t_full, 3), "total_ms_all_repeats": [round(x[0], 3) for x in full],
        "one_iteration_call_ms": round(t_one, 3),
        "ms_per_iteration": round(span_ms / max(int(its.max()) - 1, 1), 4),
        "full_pass_bytes": int(bytes_iter.sum()),
        "effective_bytes_per_s": rate, "share_of_hbm_roof": rate / HBM_ROOF,
        "synthetic_generation_s": round(gen_s, 1),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
