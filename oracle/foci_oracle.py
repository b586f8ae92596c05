"""CPU ORACLE (test infrastructure, not product code) for the callers of the correlation:
focus picking and window validation of chromosight's pattern_detector, restated independently of
chromosight_amd (dense / band numpy arrays, scipy.ndimage labelling, one plain loop per pattern).

Reference lines restated here (all in /root/reference/chromosight/utils/detection.py):
  pick_foci        :387-456   threshold (>= pearson passes), 4-connected foci, foci of fewer than
                              min_size pixels dropped, per focus the first row-major pixel holding its
                              maximum; foci numbered by the row-major position of their first pixel
  label_foci       :459-554   4-way adjacency (right / lower neighbour)
  filter_foci      :557-592
  pattern_detector :287-345   zero padding by (kh, kw) in full mode, NaN on the big_k first
                              sub-diagonals of intra maps, 1-D patterns forced on the diagonal
  validate_patterns:18-155    strict window bounds, missing bins -> NaN, zero / missing proportions
  quantify mode    :233-238, 267-273, 277, 287-345 with coords given: nothing from a map not larger than the
                              template, the score read from the diag-trimmed zero-eliminated map at the (kh, kw)-shifted
                              coordinate of maps padded by (kw, kh), drop=False (NaN score + NaN window for an invalid
                              position, :133-141), the p-value from the untrimmed map at the caller's coordinate

Pinned by tests/test_oracle_golden.py against the reference's own outputs (tests/golden/nms.npz,
example_blocks.npz) before it is trusted as the checker of the device path; quantify_table / quantify_table_band by
tests/test_quantify_oracle.py (yeast_quantify.npz, example_blocks.npz, quantify_edges.npz).
"""
import numpy as np
from scipy import ndimage as ndi

FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
# the same 4-neighbourhood in band coordinates (row i, x = j - i): (i, j+1) -> (i, x+1),
# (i+1, j) -> (i+1, x-1)
FOUR_BAND = np.array([[0, 0, 1], [1, 1, 1], [1, 0, 0]])


def pick_foci_dense(corr, pearson, min_size=2, structure=FOUR):
    """corr: dense 2-D array (zeros = nothing).  Returns an (n, 2) int array of (row, col), one per
    focus in label order, or an empty (0, 2) array."""
    cand = (corr >= pearson) & (corr != 0)
    if not cand.any():
        return np.zeros((0, 2), dtype=int)
    labels, n_lab = ndi.label(cand, structure=structure)   # numbered in raster order of first pixel
    sizes = np.bincount(labels.ravel(), minlength=n_lab + 1)
    out = []
    rows, cols = np.nonzero(labels)                         # row-major
    lab = labels[rows, cols]
    vals = corr[rows, cols]
    order = np.argsort(lab, kind="stable")
    rows, cols, lab, vals = rows[order], cols[order], lab[order], vals[order]
    starts = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]]))
    ends = np.concatenate([starts[1:], [lab.size]])
    for s, e in zip(starts, ends):
        if sizes[lab[s]] < min_size:
            continue
        k = s + int(np.argmax(vals[s:e]))                   # first maximum in row-major order
        out.append((rows[k], cols[k]))
    return np.array(out, dtype=int).reshape(-1, 2)


def pick_foci_band(corr_band, lo, pearson, min_size=2):
    """corr_band[i, x] = coefficient of pixel (i, i + lo + x).  Same rules, band coordinates."""
    foci = pick_foci_dense(corr_band, pearson, min_size, structure=FOUR_BAND)
    if foci.shape[0]:
        foci[:, 1] = foci[:, 0] + lo + foci[:, 1]
    return foci


def validate(coords, value_at, shape, miss_row, miss_col, kernel_shape, zero_tol, missing_tol, inter, full=True, stats=False):
    """Window statistics and validity of every pattern, as pattern_detector + validate_patterns do
    them.  value_at(p, q) -> contact value of matrix pixel (p, q) (vectorised, 0 when not stored).
    coords: (n, 2) matrix coordinates (unpadded).  Returns (valid bool[n], windows[n, km, kn]); with stats also a
    dict of inside (the window passes the strict bounds, :99-104), n_zero and n_missing (:123-124; 0 where not inside)."""
    km, kn = kernel_shape
    kh, kw = (km - 1) // 2, (kn - 1) // 2
    half_h, half_w = km // 2 + 1, kn // 2 + 1
    ms, ns = shape
    pad_r, pad_c = (kw, kh) if full else (0, 0)     # zero_pad_sparse(mat, kh, kw): kh columns, kw rows
    sh_r, sh_c = (kh, kw) if full else (0, 0)       # coords[:, 0] += kh; coords[:, 1] += kw
    H, W = ms + 2 * pad_r, ns + 2 * pad_c
    # framed bins that are NOT detectable (det + kh / det + kw are the detectable ones)
    fr_miss = np.ones(H, dtype=bool)
    fc_miss = np.ones(W, dtype=bool)
    ok_r = np.flatnonzero(~np.asarray(miss_row, dtype=bool)) + sh_r
    ok_c = np.flatnonzero(~np.asarray(miss_col, dtype=bool)) + sh_c
    fr_miss[ok_r[ok_r < H]] = False
    fc_miss[ok_c[ok_c < W]] = False
    big_k = max(km, kn)
    n = coords.shape[0]
    valid = np.zeros(n, dtype=bool)
    windows = np.full((n, km, kn), np.nan)
    st = {"inside": np.zeros(n, dtype=bool), "n_zero": np.zeros(n, dtype=np.int64), "n_missing": np.zeros(n, dtype=np.int64)}
    for t in range(n):
        p1, p2 = int(coords[t, 0]) + sh_r, int(coords[t, 1]) + sh_c
        high, low = p1 - half_h + 1, p1 + half_h
        left, right = p2 - half_w + 1, p2 + half_w
        if not (high >= 0 and low < H and left >= 0 and right < W):
            continue
        rr, cc = np.meshgrid(np.arange(high, low), np.arange(left, right), indexing="ij")
        src_r, src_c = rr - pad_r, cc - pad_c
        inside = (src_r >= 0) & (src_r < ms) & (src_c >= 0) & (src_c < ns)
        win = np.where(inside, value_at(np.where(inside, src_r, 0), np.where(inside, src_c, 0)), 0.0).astype(np.float64)
        if not inter:
            d = cc - rr
            win[(d <= -1) & (d >= -big_k)] = np.nan
        win[fr_miss[rr] | fc_miss[cc]] = np.nan
        tot = win.size
        n_zero = int(np.sum(win == 0))
        n_miss = int(np.sum(~np.isfinite(win)))
        st["inside"][t], st["n_zero"][t], st["n_missing"][t] = True, n_zero, n_miss
        with np.errstate(all="ignore"):
            prop_undetected = n_miss / tot
            prop_zero = np.float64(n_zero) / np.float64(tot - n_miss)
        if prop_undetected < missing_tol and prop_zero < zero_tol:
            valid[t] = True
            windows[t] = win
    return (valid, windows, st) if stats else (valid, windows)


def detect_table(matrix, corr_trimmed, miss_row, miss_col, kernel_shape, pearson, zero_tol, missing_tol,
                 inter=False, diag_only=False, full=True, return_windows=False):
    """Dense test-sized maps: (bin1, bin2, score) of the validated foci in the reference's order.
    corr_trimmed: coefficient map already restricted to the scanned diagonals (diag_trim).

    Non-square templates in full mode (detection.py:287-298, preprocessing.py:636-676): the maps are padded by
    (kw rows, kh columns) but the coordinates shifted by (kh, kw), so the score of pattern (r, c) is read at
    (r + kh - kw, c + kw - kh) (0 outside the map) and a 1-D pattern, forced on the diagonal after the shift, ends
    up at (c + kw - kh, c); validate() restates the same offsets for the windows."""
    matrix = np.asarray(matrix, dtype=np.float64)
    corr_trimmed = np.asarray(corr_trimmed, dtype=np.float64)
    km, kn = kernel_shape
    shift = ((km - 1) // 2 - (kn - 1) // 2) if full else 0
    foci = pick_foci_dense(corr_trimmed, pearson)
    if foci.shape[0] == 0:
        return (np.zeros((0, 3)), np.zeros((0, km, kn))) if return_windows else np.zeros((0, 3))
    if diag_only and not inter:
        foci[:, 0] = foci[:, 1] - shift
    valid, wins = validate(foci, lambda p, q: matrix[p, q], matrix.shape, miss_row, miss_col, kernel_shape,
                           zero_tol, missing_tol, inter, full=full)
    keep = foci[valid]
    sr, sc = keep[:, 0] + shift, keep[:, 1] - shift
    inside = (sr >= 0) & (sr < corr_trimmed.shape[0]) & (sc >= 0) & (sc < corr_trimmed.shape[1])
    scores = np.where(inside, corr_trimmed[np.where(inside, sr, 0), np.where(inside, sc, 0)], 0.0)
    table = np.column_stack([keep[:, 0], keep[:, 1], scores]).astype(np.float64)
    return (table, wins[valid]) if return_windows else table


def detect_table_band(band, band_lo, corr_band, out_lo, n, miss, kernel_shape, pearson, zero_tol, missing_tol,
                      diag_only=False):
    """Intra maps in band storage (band[i, j - i - band_lo], corr_band[i, j - i - out_lo], columns of
    corr_band = the scanned diagonals only): the same table for maps whose dense form does not fit."""
    band = np.asarray(band)
    bw = band.shape[1]
    foci = pick_foci_band(np.asarray(corr_band, dtype=np.float64), out_lo, pearson)
    if foci.shape[0] == 0:
        return np.zeros((0, 3))
    scores = corr_band[foci[:, 0], foci[:, 1] - foci[:, 0] - out_lo]
    if diag_only:
        foci[:, 0] = foci[:, 1]
        x = foci[:, 1] - foci[:, 0] - out_lo
        scores = np.where((x >= 0) & (x < corr_band.shape[1]), corr_band[foci[:, 0], np.clip(x, 0, corr_band.shape[1] - 1)], 0.0)

    def value_at(p, q):
        x = q - p - band_lo
        ok = (x >= 0) & (x < bw)
        return np.where(ok, band[p, np.where(ok, x, 0)], 0.0)

    valid, _ = validate(foci, value_at, (n, n), miss, miss, kernel_shape, zero_tol, missing_tol, False)
    keep = foci[valid]
    return np.column_stack([keep[:, 0], keep[:, 1], scores[valid]]).astype(np.float64)


def _quantify(coords, value_at, coef_at, shape, miss_row, miss_col, kernel_shape, zero_tol, missing_tol, inter, max_dist,
              full, diag_only):
    """pattern_detector(coords=...) position by position.  coef_at(rows, cols) -> (coefficient, n_obs or None, cond,
    near) of pixels of the UNTRIMMED coefficient map (0 / - / 1 / False outside it)."""
    from oracle.pearson_oracle import corr_to_pval_oracle
    km, kn = kernel_shape
    coords = np.array(coords, dtype=np.int64).reshape(-1, 2)
    n = coords.shape[0]
    out = {"bin1": coords[:, 0].copy(), "bin2": coords[:, 1].copy(), "score": np.full(n, np.nan), "valid": np.zeros(n, dtype=bool),
           "windows": np.full((n, km, kn), np.nan), "inside": np.zeros(n, dtype=bool), "n_zero": np.zeros(n, dtype=np.int64),
           "n_missing": np.zeros(n, dtype=np.int64), "pvalue": np.full(n, np.nan), "n_obs": np.full(n, np.nan),
           "cond": np.ones(n), "near": np.zeros(n, dtype=bool), "scanned": False}
    if min(shape) <= max(km, kn):                       # :236-238: (None, None), the caller keeps its NaN
        return out
    out["scanned"] = True
    shift = ((km - 1) // 2 - (kn - 1) // 2) if full else 0
    if diag_only and not inter:                         # :314-315, after the (kh, kw) shift of :297-298
        coords[:, 0] = coords[:, 1] - shift
        out["bin1"] = coords[:, 0].copy()
    valid, wins, st = validate(coords, value_at, shape, miss_row, miss_col, kernel_shape, zero_tol, missing_tol, inter,
                               full=full, stats=True)
    # the score: conv_mat[p1, p2] (:134) of the map padded by (kw rows, kh columns) at the coordinate shifted by (kh, kw)
    sr, sc = coords[:, 0] + shift, coords[:, 1] - shift
    kept = (sr >= 0) & (sr < shape[0]) & (sc >= 0) & (sc < shape[1])
    if not inter:                                       # diag_trim(mat_conv, max_dist), :269-270: diagonals 0 .. max_dist
        kept &= (sc - sr >= 0) & (sc - sr <= max_dist)
    coef, _, cond, near = coef_at(sr, sc)
    coef = np.where(np.isnan(coef), 0.0, coef)          # :267
    out["score"] = np.where(valid, np.where(kept, coef, 0.0), np.nan)
    out["cond"], out["near"] = np.where(kept, cond, 1.0), np.where(kept, near, False)
    out["valid"], out["windows"] = valid, wins
    out.update(st)
    # the p-value: mat_log10_pvals[bin1, bin2] (:336-344) -- the untrimmed map, the caller's own coordinate; a pixel the
    # sparse map does not store reads 0, that is p = 1
    c0, nobs, _, _ = coef_at(coords[:, 0], coords[:, 1])
    if nobs is not None:
        c0 = np.where(np.isnan(c0), 0.0, c0)
        with np.errstate(all="ignore"):
            logp = np.where(c0 != 0, corr_to_pval_oracle(c0, nobs), 0.0)
            out["pvalue"] = 10.0 ** logp
        out["n_obs"] = np.asarray(nobs, dtype=np.float64)
    return out


def quantify_table(matrix, corr, coords, miss_row, miss_col, kernel_shape, zero_tol, missing_tol, inter=False, max_dist=None,
                   n_obs=None, full=True, diag_only=False):
    """Quantify mode on a dense test-sized map (intra or inter).  corr: the oracle's UNTRIMMED coefficient map (the trimming
    to the diagonals 0 .. max_dist of an intra map is done here), or a callable (rows, cols) -> (coefficient, n_obs, cond,
    near) such as c_oracle.normxcorr2_points; n_obs: the present-pixel counts of the map (p-values need them).  Returns a
    dict of per-position arrays in input order: bin1, bin2, score (NaN when invalid, 0 outside the trimmed map), valid,
    windows (NaN when invalid), inside, n_zero, n_missing, pvalue, n_obs, cond, near; scanned False when the map is not
    larger than the template (everything NaN)."""
    matrix = np.asarray(matrix, dtype=np.float64)
    if callable(corr):
        coef_at = corr
    else:
        corr = np.asarray(corr, dtype=np.float64)

        def coef_at(r, c):
            ok = (r >= 0) & (r < corr.shape[0]) & (c >= 0) & (c < corr.shape[1])
            rr, cc = np.where(ok, r, 0), np.where(ok, c, 0)
            nobs = None if n_obs is None else np.where(ok, np.asarray(n_obs)[rr, cc], float(kernel_shape[0] * kernel_shape[1]))
            return np.where(ok, corr[rr, cc], 0.0), nobs, np.ones(r.size), np.zeros(r.size, dtype=bool)
    return _quantify(coords, lambda p, q: matrix[p, q], coef_at, matrix.shape, miss_row, miss_col, kernel_shape, zero_tol,
                     missing_tol, inter, max_dist, full, diag_only)


def quantify_table_band(band, band_lo, corr_band, out_lo, n, coords, miss, kernel_shape, zero_tol, missing_tol, max_dist,
                        n_obs_band=None, diag_only=False):
    """The same for an intra map in band storage (band[i, j - i - band_lo]).  corr_band[i, j - i - out_lo]: the oracle's
    coefficient band (what it does not hold reads 0), n_obs_band alike; or a callable as in quantify_table."""
    band = np.asarray(band)
    bw = band.shape[1]

    def value_at(p, q):
        x = q - p - band_lo
        ok = (x >= 0) & (x < bw)
        return np.where(ok, band[p, np.where(ok, x, 0)], 0.0)

    if callable(corr_band):
        coef_at = corr_band
    else:
        corr_band = np.asarray(corr_band, dtype=np.float64)

        def coef_at(r, c):
            x = c - r - out_lo
            ok = (r >= 0) & (r < n) & (c >= 0) & (c < n) & (x >= 0) & (x < corr_band.shape[1])
            rr, xx = np.where(ok, r, 0), np.where(ok, x, 0)
            nobs = None if n_obs_band is None else np.where(ok, np.asarray(n_obs_band)[rr, xx], float(kernel_shape[0] * kernel_shape[1]))
            return np.where(ok, corr_band[rr, xx], 0.0), nobs, np.ones(r.size), np.zeros(r.size, dtype=bool)
    return _quantify(coords, value_at, coef_at, (n, n), miss, miss, kernel_shape, zero_tol, missing_tol, False, max_dist,
                     True, diag_only)
