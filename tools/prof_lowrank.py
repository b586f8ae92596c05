#!/usr/bin/env python3
"""--tsvd templates: the same calls on the separable low-rank kernel (cs_corr_lowrank.hip, CHROMOSIGHT_HIP_LOWRANK=1) and on the
kernels of the full template (CHROMOSIGHT_HIP_LOWRANK=0), outputs compared.  What the default dispatch rule (cs_api.cpp
lowrank_wanted) is set from.
    python tools/prof_lowrank.py [dense] [c4p] [c4p_map] [detect] [--json out.json]
dense: an unmasked map call on a dense 4096^2 float32 map; c4p: a candidate call (the detect configuration: per-bin masks,
sym_upper, full, diagonals 0 .. 1000) on the C4' band, 200 000 x 1 001; c4p_map: a map call of that configuration, band out,
loops 41 / 61; detect: pipeline.detect(..., tsvd=0.999) on the C4 genome
(200 000 bins, 23 chromosomes) with loops and with loops at --win-size 41.  Templates at tsvd 0.999: loops 17, borders 17,
stripes 31, loops resized to 33 / 41 / 61."""
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import chromosight_amd  # noqa: E402
import chromosight_amd.kernels as ck  # noqa: E402
from chromosight_amd import engine, pipeline  # noqa: E402
from chromosight_amd._lib import CS_F32, LAYOUT_BAND, LAYOUT_DENSE, MASK_BINS, CsMatrix, get_device, np_dtype_code  # noqa: E402
from chromosight_amd.utils import preprocessing as cup  # noqa: E402
from tools.synthetic_genome import band_workload, make_cool  # noqa: E402

KERNELS = {1: "runtime-size", 2: "streaming", 3: "mfma", 4: "mfma dense", 5: "mfma per-bin", 6: "separable", 7: "mfma 18..33",
           8: "mfma list", 9: "mfma 34..81", 10: "low-rank"}


def templates():
    loops = np.asarray(ck.loops["kernels"][0], dtype=np.float64)
    out = {"loops17": loops, "borders17": np.asarray(ck.borders["kernels"][0], dtype=np.float64),
           "stripes31": np.asarray(ck.stripes_left["kernels"][0], dtype=np.float64)}
    for s in (33, 41, 61):
        out[f"loops{s}"] = cup.resize_kernel(loops, factor=s / 17, quiet=True)
    return out


def timed(dev, call, reps):
    out = call()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = call()
    dev.sync()
    return (time.perf_counter() - t0) / reps * 1e3, out


def both(dev, label, call, reps, compare):
    res, outs = {}, {}
    for route in ("1", "0"):
        os.environ["CHROMOSIGHT_HIP_LOWRANK"] = route
        try:
            ms, out = timed(dev, call, reps)
        finally:
            del os.environ["CHROMOSIGHT_HIP_LOWRANK"]
        k = dev.lib.cs_last_kernel(dev.ctx)
        res["lowrank" if route == "1" else "full"] = {"ms": round(ms, 4), "kernel": KERNELS.get(k, str(k))}
        outs[route] = out
    res["speedup"] = round(res["full"]["ms"] / res["lowrank"]["ms"], 2)
    res.update(compare(outs["1"], outs["0"]))
    print(f"{label:28s} low-rank {res['lowrank']['ms']:9.3f} ms   {res['full']['kernel']:12s} {res['full']['ms']:9.3f} ms   "
          f"{res['speedup']:5.2f}x  {dict((k, v) for k, v in res.items() if k not in ('lowrank', 'full', 'speedup'))}", flush=True)
    return res


def dense_cases(dev, kernels):
    n = 4096
    a = np.random.default_rng(0).gamma(2.0, 1.0, size=(n, n)).astype(np.float32)
    d_sig, ld = engine.to_device_map(dev, a)
    sig = CsMatrix(d_sig.ptr, np_dtype_code(np.float32), LAYOUT_DENSE, ld, 0, 0)
    d_out = dev.empty(n * ld, np.float32)
    out = CsMatrix(d_out.ptr, CS_F32, LAYOUT_DENSE, ld, 0, 0)
    res = {}
    for name, kern in kernels.items():
        spec = engine.KernelSpec(kern, 0.999)

        def call():
            engine.run_normxcorr2(dev, sig, (n, n), spec, out, full=False, sym_upper=False, max_dist=None, precision="f32")
            return d_out.download().reshape(n, ld)[:, :n].copy() if compare_now[0] else None

        compare_now = [False]

        def cmp(x, y):
            return {}
        res[name] = both(dev, f"dense 4096^2 {name}", call, 10, cmp)
        compare_now[0] = True
        os.environ["CHROMOSIGHT_HIP_LOWRANK"] = "1"
        lr = call()
        os.environ["CHROMOSIGHT_HIP_LOWRANK"] = "0"
        fr = call()
        del os.environ["CHROMOSIGHT_HIP_LOWRANK"]
        res[name]["max_abs_diff"] = float(np.abs(lr - fr).max())
        print(f"{'':28s} max |low-rank - full| {res[name]['max_abs_diff']:.2e}", flush=True)
    return res


def band_cases(dev, kernels):
    band, band_w, miss, n, max_dist = band_workload("c4p")
    d_sig, d_miss = dev.to_device(band), dev.to_device(miss)
    sig = CsMatrix(d_sig.ptr, np_dtype_code(np.float32), LAYOUT_BAND, band.shape[1], 0, band_w)
    res = {}
    for name, kern in kernels.items():
        spec = engine.KernelSpec(kern, 0.999)

        def call():
            return engine.run_candidates(dev, sig, (n, n), spec, (0, n), pearson=0.5, lo_diag=0, hi_diag=max_dist, inter=False,
                                         full=True, sym_upper=True, max_dist=max_dist, mask_mode=MASK_BINS, miss_row=d_miss,
                                         miss_col=d_miss, missing_tol=0.5, precision="f32")

        def cmp(x, y):
            return {"same_candidates": all(np.array_equal(p, q) for p, q in zip(x, y)), "candidates": int(len(x[0]))}
        res[name] = both(dev, f"C4' band {name}", call, 3, cmp)
    return res


def band_map_cases(dev, kernels):
    """Map calls on the C4' band (per-bin masks, sym_upper, full, band in / band out): what the default rule sends to the new kernel."""
    band, band_w, miss, n, max_dist = band_workload("c4p")
    d_sig, d_miss = dev.to_device(band), dev.to_device(miss)
    sig = CsMatrix(d_sig.ptr, np_dtype_code(np.float32), LAYOUT_BAND, band.shape[1], 0, band_w)
    out_w = max_dist + 1
    ld = (out_w + 63) // 64 * 64
    d_out = dev.empty(n * ld, np.float32)
    out = CsMatrix(d_out.ptr, CS_F32, LAYOUT_BAND, ld, 0, out_w)
    res = {}
    for name, kern in kernels.items():
        spec = engine.KernelSpec(kern, 0.999)

        def call():
            engine.run_normxcorr2(dev, sig, (n, n), spec, out, full=True, sym_upper=True, max_dist=max_dist, mask_mode=MASK_BINS,
                                  miss_row=d_miss, miss_col=d_miss, missing_tol=0.5, precision="f32")
            return d_out.download().reshape(n, ld)[:, :out_w].copy()

        def cmp(x, y):
            return {"max_abs_diff": float(np.abs(x - y).max())}
        res[name] = both(dev, f"C4' band map {name}", call, 1, cmp)
    return res


def detect_cases(dev):
    cool = make_cool(total_bins=200_000, max_dist_bins=1000, largest_kernel=41)[0]
    dcool = pipeline.DeviceCool(cool)
    res = {}
    for label, win in (("loops", None), ("loops_win41", 41)):
        cfg = copy.deepcopy(ck.loops)

        def call():
            return pipeline.detect(dcool, cfg, tsvd=0.999, win_size=win)

        def cmp(x, y):
            cols = ["chrom1", "start1", "chrom2", "start2", "kernel_id"]
            same = bool(x[cols].equals(y[cols])) and bool(np.allclose(np.asarray(x["score"], dtype=np.float64), np.asarray(y["score"], dtype=np.float64), rtol=0,
                                                                      atol=1e-12))
            return {"same_patterns": same, "rows": int(len(x))}
        res[label] = both(dev, f"detect --tsvd {label}", call, 2, cmp)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out in args:
        args.remove(out)
    chromosight_amd.set_precision("f32")
    dev = get_device()
    kernels = templates()
    res = {"device": "MI355X", "tsvd": 0.999,
           "ranks": {k: [int(cup.factorise_kernel(v.copy(), 0.999)[0].shape[1]), int(cup.factorise_kernel(v ** 2, 0.999)[0].shape[1])]
                     for k, v in kernels.items()}}
    for what in (args or ["dense", "c4p", "c4p_map", "detect"]):
        if what == "dense":
            res["dense_4096_map"] = dense_cases(dev, kernels)
        elif what == "c4p":
            res["c4p_band_candidates"] = band_cases(dev, kernels)
        elif what == "c4p_map":
            res["c4p_band_map"] = band_map_cases(dev, {k: v for k, v in kernels.items() if k in ("loops41", "loops61")})
        elif what == "detect":
            res["detect_c4_genome"] = detect_cases(dev)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
