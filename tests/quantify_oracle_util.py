"""The CPU quantify pipeline made of the pinned oracles, shared by tests/test_quantify_oracle.py (which pins it on the
reference's captures) and tests/test_gpu_quantify_oracle.py (which holds the device to it): block preparation
(oracle/detrend_oracle.py; trans blocks as the reference's contacts_map.py:598-601), coefficients of the requested
pixels (oracle/oracle.c through c_oracle.normxcorr2_points), the quantify rules (oracle/foci_oracle.py) and the
selection of cmd_quantify (cli/chromosight.py:383-477).  Nothing here imports chromosight_amd."""
import numpy as np
import pandas as pd

from oracle import c_oracle, detrend_oracle, foci_oracle, pearson_oracle


def intra_block(cool, ci, max_dist, largest, smooth=False):
    """(prepared band [n, keep + 1], miss bool [n]) of chromosome ci as ContactMap.create_mat prepares it."""
    off = cool["chrom_offset"]
    n = int(off[ci + 1] - off[ci])
    keep = min(max_dist, n) + largest
    band, det = detrend_oracle.balanced_band(cool, ci, keep)
    prepared, _ = detrend_oracle.prepare_band(band, det, smooth=smooth)
    return prepared, ~det


def inter_block(cool, ca, cb):
    """(dense trans block, miss_rows, miss_cols): count * w1 * w2, NaN -> 0, divided by the median of the stored values."""
    off = cool["chrom_offset"]
    b1, b2 = np.asarray(cool["bin1_id"]), np.asarray(cool["bin2_id"])
    cnt, w = np.asarray(cool["count"], dtype=np.float64), np.asarray(cool["weight"], dtype=np.float64)
    s1, e1, s2, e2 = int(off[ca]), int(off[ca + 1]), int(off[cb]), int(off[cb + 1])
    sel = (b1 >= s1) & (b1 < e1) & (b2 >= s2) & (b2 < e2)
    with np.errstate(invalid="ignore"):
        vals = cnt[sel] * w[b1[sel]] * w[b2[sel]]
    vals = np.where(np.isnan(vals), 0.0, vals)
    dense = np.zeros((e1 - s1, e2 - s2))
    if vals.size:
        with np.errstate(all="ignore"):
            dense[b1[sel] - s1, b2[sel] - s2] = vals / float(np.median(vals))
    dense[np.isnan(dense)] = 0.0
    return dense, ~np.isfinite(w[s1:e1]), ~np.isfinite(w[s2:e2])


def _truncated(kernel, tsvd):
    """(template of the correlation sums, template of the masked square sums) under --tsvd, else (None, None)."""
    if tsvd is None:
        return None, None
    return pearson_oracle.tsvd_kernel_oracle(kernel, tsvd), pearson_oracle.tsvd_kernel_oracle(kernel ** 2, tsvd)


def quantify_intra(prepared, miss, kernel, coords, cfg, max_dist, tsvd=None):
    """foci_oracle.quantify_table_band with the coefficients of the requested pixels only."""
    n = prepared.shape[0]
    kernel = np.asarray(kernel, dtype=np.float64)
    mtol = cfg["max_perc_undetected"] / 100
    kc, k2 = _truncated(kernel, tsvd)

    def coef_at(r, c):
        return c_oracle.normxcorr2_points(prepared, (n, n), kernel, r, c, band_lo=0, max_dist=max_dist, sym_upper=True, full=True,
                                          miss_row=miss, miss_col=miss, missing_tol=mtol, kernel_conv=kc, kernel_sq=k2)
    return foci_oracle.quantify_table_band(prepared, 0, coef_at, 0, n, coords, miss, kernel.shape, cfg["max_perc_zero"] / 100, mtol,
                                           max_dist, diag_only=cfg["max_dist"] == 0)


def quantify_inter(dense, miss_r, miss_c, kernel, coords, cfg, tsvd=None):
    kernel = np.asarray(kernel, dtype=np.float64)
    mtol = cfg["max_perc_undetected"] / 100
    kc, k2 = _truncated(kernel, tsvd)

    def coef_at(r, c):
        return c_oracle.normxcorr2_points(dense, dense.shape, kernel, r, c, max_dist=None, sym_upper=False, full=True,
                                          miss_row=miss_r, miss_col=miss_c, missing_tol=mtol, kernel_conv=kc, kernel_sq=k2)
    return foci_oracle.quantify_table(dense, coef_at, coords, miss_r, miss_c, kernel.shape, cfg["max_perc_zero"] / 100, mtol,
                                      inter=True)


FIELDS = ("score", "pvalue", "cond", "near", "inside", "n_zero", "n_missing", "valid", "bin1", "bin2", "n_obs")


def quantify_genome(cool, positions, cfg, inter=False, max_dist_bp=None, smooth=False, tsvd=None):
    """cmd_quantify (cli/chromosight.py:295-477) on a decoded .cool with the oracles.  Returns (per-template list of dicts of
    per-position arrays in INPUT order -- FIELDS, `windows`, `located` --, the output table as the reference selects and sorts
    it: columns of the bed2d + bin1, bin2, score, pvalue, src (input row), kernel_id)."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    names = [str(x) for x in cool["chrom_names"]]
    binsize = int(cool["binsize"])
    sizes = np.diff(off)
    bed = positions.loc[:, ["chrom1", "start1", "end1", "chrom2", "start2", "end2"]].reset_index(drop=True)
    cfg = dict(cfg)
    furthest = int(np.max(bed.start2 - bed.start1))                           # :344-347
    cfg["max_dist"] = min(furthest, int(off[-1]) * binsize) if max_dist_bp is None else int(max_dist_bp)
    kernels = [np.asarray(k, dtype=np.float64) for k in cfg["kernels"]]
    km, kn = kernels[0].shape
    max_dist = max(cfg["max_dist"] // binsize, 1)                             # contacts_map.py compute_max_dist
    largest = max(k.shape[0] for k in kernels)
    n_pos = len(bed)
    code = {c: i for i, c in enumerate(names)}
    c1 = np.array([code.get(str(c), -1) for c in bed.chrom1], dtype=np.int64)
    c2 = np.array([code.get(str(c), -1) for c in bed.chrom2], dtype=np.int64)

    def bins(codes, bp):                                                      # coords_to_bins: no such bin -> -1 here
        local = np.asarray(bp, dtype=np.int64) // binsize
        ok = (codes >= 0) & (local >= 0) & (local < sizes[np.maximum(codes, 0)])
        return np.where(ok, local, -1)
    s1, e1, s2, e2 = (bed[c].to_numpy(dtype=np.int64) for c in ("start1", "end1", "start2", "end2"))
    l1, l2 = bins(c1, (s1 + e1) // 2), bins(c2, (s2 + e2) // 2)               # :383-384: the interval centres are scored
    located = (l1 >= 0) & (l2 >= 0)
    res = []
    for k in kernels:
        d = {f: np.full(n_pos, np.nan) for f in ("score", "pvalue", "cond", "n_obs")}
        d.update({f: np.zeros(n_pos, dtype=np.int64) for f in ("inside", "n_zero", "n_missing", "near", "valid")})
        d.update({f: np.full(n_pos, -1, dtype=np.int64) for f in ("bin1", "bin2", "chrom1", "chrom2")})
        d["windows"] = np.full((n_pos, km, kn), np.nan)
        d["scanned"] = np.zeros(n_pos, dtype=bool)
        res.append(d)
    for ca in range(len(names)):
        for cb in range(ca, len(names)):
            if ca != cb and not inter:
                continue
            sel = np.flatnonzero(located & (c1 == ca) & (c2 == cb))
            if not sel.size:
                continue
            coords = np.column_stack([l1[sel], l2[sel]])
            if ca == cb:
                prepared, miss = intra_block(cool, ca, max_dist, largest, smooth=smooth)
            else:
                dense, mr, mc = inter_block(cool, ca, cb)
            for ki, kern in enumerate(kernels):
                q = (quantify_intra(prepared, miss, kern, coords, cfg, max_dist, tsvd) if ca == cb
                     else quantify_inter(dense, mr, mc, kern, coords, cfg, tsvd))
                if not q["scanned"]:
                    continue
                for f in FIELDS:
                    res[ki][f][sel] = q[f]
                res[ki]["windows"][sel] = q["windows"]
                res[ki]["scanned"][sel] = True
                res[ki]["chrom1"][sel], res[ki]["chrom2"][sel] = ca, cb
    for d in res:
        d["located"] = located
    # :432-477: the tables of the templates one below the other, ascending sort by score, last row of every (chrom1, start1,
    # chrom2, start2) group, bins of the interval STARTS, NaN p-value where the score is NaN, sort by (bin1, bin2)
    long = pd.concat([bed.assign(score=d["score"], pvalue=d["pvalue"], src=np.arange(n_pos), kernel_id=ki) for ki, d in enumerate(res)],
                     axis=0).reset_index(drop=True)
    pick = long.sort_values("score", ascending=True).groupby(["chrom1", "start1", "chrom2", "start2"], sort=False).tail(1)
    pick = pick.reset_index(drop=True)
    src = pick.src.to_numpy()
    g1, g2 = bins(c1[src], s1[src]), bins(c2[src], s2[src])
    pick["bin1"] = np.where(g1 < 0, np.nan, off[np.maximum(c1[src], 0)] + g1)
    pick["bin2"] = np.where(g2 < 0, np.nan, off[np.maximum(c2[src], 0)] + g2)
    # :452, 470-471: Benjamini-Hochberg over the p-values of ALL rows before the invalid ones are blanked -- one NaN among them
    # (a position no sub-matrix holds, or one on a map not larger than the template) makes every q-value NaN (stats.py:12-40)
    pick["qvalue_nan"] = np.isnan(pick.score) | bool(np.isnan(pick.pvalue).any())
    pick.loc[np.isnan(pick.score), "pvalue"] = np.nan
    pick = pick.sort_values(["bin1", "bin2"], ascending=True, kind="stable").reset_index(drop=True)
    return res, pick
