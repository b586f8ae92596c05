#!/usr/bin/env python3
"""Templates with a side of 34 .. 81 (the 81 x 81 `centromeres` template): the same candidate calls on the matrix-core kernel
(cs_corr_large.hip, the default) and on the runtime-size kernel (CHROMOSIGHT_HIP_NO_LARGE=1), with the candidate lists compared.
    python tools/time_large.py [dense] [c4p] [strips] [--json out.json]
dense: an 81 x 81 candidate call on a dense masked 4096^2 inter-style block; c4p: the same on C4'-style masked band (per-bin
masks, sym_upper, the scanned diagonals 0 .. max_dist); strips: pipeline.detect(..., inter=True) with the centromeres preset on a
synthetic genome (tools/synthetic_inter.py), the trans blocks through their tile lists."""
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
from chromosight_amd._lib import LAYOUT_BAND, LAYOUT_DENSE, MASK_BINS, CsMatrix, get_device, np_dtype_code  # noqa: E402
from tools.synthetic_genome import band_workload  # noqa: E402
from tools.synthetic_inter import make_trans_cool  # noqa: E402

KERNELS = {1: "runtime-size", 9: "matrix cores (34 .. 81)"}
CENTRO = np.asarray(ck.centromeres["kernels"][0], dtype=np.float64)


def timed(dev, call, reps, warm=1):
    for _ in range(warm):
        out = call()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = call()
    dev.sync()
    return (time.perf_counter() - t0) / reps * 1e3, out


def both(dev, label, call, pixels, reps):
    res = {}
    outs = {}
    for name, env in (("large", {}), ("runtime_size", {"CHROMOSIGHT_HIP_NO_LARGE": "1"})):
        os.environ.update(env)
        try:
            ms, out = timed(dev, call, reps if not env else 1)
        finally:
            for a in env:
                del os.environ[a]
        kern = KERNELS.get(dev.lib.cs_last_kernel(dev.ctx), str(dev.lib.cs_last_kernel(dev.ctx)))
        res[name] = {"ms": round(ms, 3), "kernel": kern, "gpixel_per_s": round(pixels / ms / 1e6, 3) if pixels else None}
        outs[name] = out
        print(f"{label:34s} {name:13s} kernel {kern:26s} {ms:10.3f} ms", flush=True)
    a, b = outs["large"], outs["runtime_size"]
    same = all(np.array_equal(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else bool(a)
    res["speedup"] = round(res["runtime_size"]["ms"] / res["large"]["ms"], 2)
    res["same_candidates"] = bool(same)
    print(f"{label:34s} speedup {res['speedup']:.2f}x, same candidates: {same}", flush=True)
    return res


def dense_case(dev):
    n = 4096
    rng = np.random.default_rng(0)
    a = (rng.gamma(4.0, 0.25, size=(n, n)) * (rng.random((n, n)) > 0.3)).astype(np.float32)
    miss = rng.random(n) < 0.02
    a[miss, :] = 0
    a[:, miss] = 0
    d_sig, ld = engine.to_device_map(dev, a)
    sig = CsMatrix(d_sig.ptr, np_dtype_code(np.float32), LAYOUT_DENSE, ld, 0, 0)
    d_miss = dev.to_device(miss.astype(np.uint8))
    spec = engine.KernelSpec(CENTRO)

    def call():
        return engine.run_candidates(dev, sig, (n, n), spec, (0, n), pearson=0.5, lo_diag=-(n - 1), hi_diag=n - 1, inter=True,
                                     full=True, sym_upper=False, max_dist=-1, mask_mode=MASK_BINS, miss_row=d_miss, miss_col=d_miss,
                                     missing_tol=0.5, precision="f32")
    return both(dev, "dense masked 4096^2, 81x81", call, n * n, 5)


def band_case(dev):
    band, band_w, miss, n, max_dist = band_workload("c4p")
    d_sig, d_miss = dev.to_device(band), dev.to_device(miss)
    sig = CsMatrix(d_sig.ptr, np_dtype_code(np.float32), LAYOUT_BAND, band.shape[1], 0, band_w)
    spec = engine.KernelSpec(CENTRO)

    def call():
        return engine.run_candidates(dev, sig, (n, n), spec, (0, n), pearson=0.5, lo_diag=0, hi_diag=max_dist, inter=False,
                                     full=True, sym_upper=True, max_dist=max_dist, mask_mode=MASK_BINS, miss_row=d_miss,
                                     miss_col=d_miss, missing_tol=0.5, precision="f32")
    return both(dev, f"C4' band {n} x {max_dist + 1}, 81x81", call, n * (max_dist + 1), 3)


def strips_case(dev, bins):
    cool, planted = make_trans_cool(total_bins=bins, n_chroms=24, intra_diags=200, n_trans=int(20_000_000 * bins / 310_000),
                                    n_planted=40, template=CENTRO, binsize=10_000, seed=5)
    cfg = copy.deepcopy(ck.centromeres)
    cfg["max_perc_zero"] = 100.0

    def call():
        dcool = pipeline.DeviceCool(cool)
        table = pipeline.detect(dcool, cfg, inter=True, inter_budget=2 << 30)
        trans = table[table.chrom1 != table.chrom2]
        found = set(zip(trans.bin1.astype(int), trans.bin2.astype(int)))
        hit = sum(any(abs(i - a) <= 1 and abs(j - b) <= 1 for a, b in found) for i, j in planted)
        print(f"  {len(table)} patterns, {hit}/{len(planted)} planted found, pool high-water {dcool.inter_high_water} B", flush=True)
        return (table.to_numpy(),)
    return both(dev, f"detect --inter, {bins} bins", call, 0, 1)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
    if out in args:
        args.remove(out)
    chromosight_amd.set_precision("f32")
    dev = get_device()
    res = {"device": "MI355X", "template": "centromeres 81x81", "pearson": 0.5}
    for what in (args or ["dense", "c4p", "strips"]):
        if what == "dense":
            res["dense_masked_4096"] = dense_case(dev)
        elif what == "c4p":
            res["c4p_band"] = band_case(dev)
        elif what.startswith("strips"):
            bins = int(what.split(":")[1]) if ":" in what else 60_000
            res[f"strips_{bins}_bins"] = strips_case(dev, bins)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
