"""The adversarial staging cases (tests/staging_cases.py) pinned on the CPU before any device sees them: every shape the
metadata lists is really in the table, the exact-law cases have exact laws, no random-valued pixel sits on the cap, and the
expectations -- oracle/detrend_oracle.py's band route -- agree with a dense restatement of the reference's rules that shares no
code with it."""
from fractions import Fraction

import numpy as np
import pytest

import staging_cases as sc


def dense_prepared(cool, ci, keep, smooth=False, max_val=sc.MAX_VAL):
    """create_mat of one intra block in dense numpy, pixel by pixel (the rules detrend_oracle's docstring lists): balanced
    upper triangle; law[d] = mean of the > 0 pixels of diagonal d between detectable bins, d <= keep; smooth: non-finite -> 0,
    closest non-increasing law; matrix / law (NaN law -> 0), >= max_val -> 1; diagonals beyond keep removed; NaN -> 0.
    Returns (dense prepared, dense uncapped ratio)."""
    off = cool["chrom_offset"]
    s, e = int(off[ci]), int(off[ci + 1])
    n = e - s
    w = cool["weight"]
    m = np.zeros((n, n))
    for a, b, v in zip(cool["bin1_id"], cool["bin2_id"], cool["count"]):
        if s <= a < e and s <= b < e and b >= a:
            m[a - s, b - s] = float(v) * w[a] * w[b]
    det = np.isfinite(w[s:e])
    law = np.zeros(n)
    for d in range(min(n, keep + 1)):
        vals = [m[i, i + d] for i in range(n - d) if det[i] and det[i + d] and m[i, i + d] > 0]
        law[d] = sum(vals) / len(vals) if vals else np.nan
    if smooth and n > 2:
        # closest non-increasing law: fit[i] = min over j <= i of max over k >= i of mean(y[j .. k]), every mean from exact
        # rational prefix sums, rounded once.  The reference fits all n entries, zeros behind the kept diagonals: a mean that
        # reaches into those zeros is below the one that stops before them, so the maximum never does -- the first min(n, keep + 1) suffice.
        nd = min(n, keep + 1)
        y = [Fraction(float(v)) if np.isfinite(v) else Fraction(0) for v in law[:nd]]
        cum = [Fraction(0)]
        for v in y:
            cum.append(cum[-1] + v)
        mean = np.full((nd, nd), -np.inf)
        for j in range(nd):
            for k in range(j, nd):
                mean[j, k] = float((cum[k + 1] - cum[j]) / (k - j + 1))
        law[:nd] = [min(mean[j, i:].max() for j in range(i + 1)) for i in range(nd)]
    law = np.where(np.isnan(law), 0.0, law)
    i, j = np.indices((n, n))
    with np.errstate(all="ignore"):
        ratio = m / law[np.abs(i - j)]
    out = ratio.copy()
    out[out >= max_val] = 1.0
    for a in (out, ratio):
        a[(j - i > keep) | (j < i)] = 0.0
    out[np.isnan(out)] = 0.0
    return out, ratio


def band_to_dense(band, n):
    out = np.zeros((n, n))
    for d in range(min(n, band.shape[1])):
        i = np.arange(n - d)
        out[i, i + d] = band[i, d]
    return out


def _checks(case):
    """(ci, keep, smooth) the case is staged with; the widest chromosomes only with the narrower bands (dense n x n work)."""
    seen = set()
    for smooth, stagings in ((False, case.stagings), (True, case.smooth)):
        for st in stagings:
            for ci in case.chroms(st):
                n = case.n(ci)
                if n > 300 and (st[0] > 200 or (smooth and n > 800)):
                    continue
                seen.add((ci, sc.keep_of(st[0], n), smooth))
    return sorted(seen)


@pytest.mark.parametrize("name", list(sc.BUILDERS))
def test_band_oracle_equals_a_dense_restatement(name):
    case = sc.get(name)
    n_blocks = n_capped = 0
    worst = 0.0
    for ci, keep, smooth in _checks(case):
        n = case.n(ci)
        out, law, det, ratio = case.expected(ci, keep, smooth)
        want, want_ratio = dense_prepared(case.cool, ci, keep, smooth)
        got = band_to_dense(out, n)
        assert np.array_equal(got == 0, want == 0), (name, ci, keep, smooth)
        capped = (got == 1.0) & (band_to_dense(np.nan_to_num(ratio, nan=0.0, posinf=np.inf), n) >= sc.MAX_VAL)
        assert np.array_equal(capped, (want == 1.0) & (want_ratio >= sc.MAX_VAL)), (name, ci, keep, smooth)
        err = np.abs(got - want)
        assert np.all(err <= 1e-14 * np.abs(want)), (name, ci, keep, smooth, err.max())
        nz = want != 0
        worst = max(worst, float((err[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0)
        n_blocks += 1
        n_capped += int(capped.sum())
    assert n_blocks > 0
    print(f"{name}: {n_blocks} blocks, worst relative difference {worst:.2e}, {n_capped} capped pixels")


def _cis_rows(case, ci):
    """row -> sorted distances of its stored upper cis pixels, row -> number of its trans pixels."""
    off = case.offsets
    s, e = int(off[ci]), int(off[ci + 1])
    b1, b2 = case.cool["bin1_id"], case.cool["bin2_id"]
    cis, trans = {r: [] for r in range(e - s)}, {r: 0 for r in range(e - s)}
    for a, b in zip(b1, b2):
        if s <= a < e:
            if s <= b < e:
                if b >= a:
                    cis[a - s].append(int(b - a))
            else:
                trans[a - s] += 1
    return cis, trans


def test_row_shapes_are_where_the_metadata_says():
    case = sc.get("row_shapes")
    assert case.cool["count"].dtype == np.int32
    meta, K = case.meta["rows"], case.meta["keep"]
    assert K == sc.keep_of(60, 700) and sc.geometry(60, 700)[1] and sc.geometry(200, 700)[1]
    cis, trans = _cis_rows(case, case.meta["chrom"])
    assert cis[meta["empty"]] == [] and trans[meta["empty"]] == 0
    assert cis[meta["trans_only"]] == [] and trans[meta["trans_only"]] > 0
    assert cis[meta["beyond_keep"]] and min(cis[meta["beyond_keep"]]) > K
    for d0, r in meta["first_d"].items():
        assert cis[r][0] == d0 and trans[r] > 0
    assert sorted(meta["first_d"]) == [0, 1, K - 1, K, K + 1]
    assert cis[meta["single_last_diag"]] == [K]
    for m, r in meta["n_cis"].items():
        assert cis[r] == list(range(m))
    assert sorted(meta["n_cis"]) == [1, 2, 63, 64, 65, 128, 129]
    for gap, (r, d) in meta["gaps"].items():
        k = cis[r].index(d)
        assert cis[r][k + 1] - d - 1 == gap
    assert sorted(meta["gaps"])[:4] == [1, 63, 64, 65] and max(meta["gaps"]) > 128
    for r in meta["tail"]:
        assert cis[r] == list(range(700 - r)) and r + K >= 700 and trans[r] > 0
    twin, _ = _cis_rows(case, case.meta["twin"])
    assert all(d[:218] == list(range(min(218, 700 - r))) for r, d in twin.items())
    w = case.cool["weight"]
    fin = w[np.isfinite(w)]
    assert fin.min() < 1e-2 and fin.max() > 1e2
    assert np.count_nonzero(case.cool["count"] == 0) > 100                      # explicit stored zeros
    sym = sc.get("row_shapes_sym").cool
    assert np.any(sym["bin2_id"] < sym["bin1_id"]) and sym["count"].size > 1.9 * case.cool["count"].size - 1504
    print("row_shapes:", {k: (len(v) if hasattr(v, "__len__") else 1) for k, v in meta.items()})


def test_sizes_cover_both_layouts_and_every_keep_rule():
    case = sc.get("sizes")
    want = set([1, 2, 3, 16, 17, 18, 63, 64, 65, 255, 256, 257, 1031]) | set(range(4, 41))
    assert set(case.meta["sizes"]) == want and case.offsets[-1] <= 3000
    assert case.cool["count"].dtype == np.float64 and np.any(case.cool["count"] != np.rint(case.cool["count"]))
    layouts = {}
    for st in case.stagings:
        for ci in case.chroms(st):
            n = case.n(ci)
            layouts.setdefault(n, set()).add(sc.geometry(st[0], n)[1])
    for ci, n in enumerate(case.meta["sizes"]):
        mds = {st[0] for st in case.stagings if ci in case.chroms(st)}
        assert {1, 5, 60, n - 1, n, n + 1} <= mds and max(mds) >= n
    assert layouts[38] == {False} and layouts[39] == {True, False} and layouts[1031] == {True, False}
    print("sizes: banded at some distance", sorted(n for n, v in layouts.items() if True in v))


def test_missing_bins_are_where_the_metadata_says():
    case = sc.get("missing")
    w, meta = case.cool["weight"], case.meta
    miss0 = np.isnan(w[:300])
    runs = []
    k = 0
    while k < 300:
        if miss0[k]:
            j = k
            while j < 300 and miss0[j]:
                j += 1
            runs.append((k, j - k))
            k = j
        else:
            k += 1
    assert sorted(m for _, m in runs) == sorted([1, 1, 1, 1, 1, 1, 2, 17, 64])
    assert miss0[0] and miss0[299] and all(miss0[meta["isolated"]])
    assert np.array_equal(np.isnan(w[300:500]), np.arange(200) % 2 == 0)
    assert np.all(np.isnan(w[500:540]))
    assert np.flatnonzero(np.isfinite(w[540:660])).tolist() == [meta["one_bin"][1]]
    print("missing: runs in chromosome 0", runs)


@pytest.mark.parametrize("name", ["missing", "diagonals"])
def test_empty_diagonals_are_empty_for_the_reason_given(name):
    case = sc.get(name)
    counts = {}
    for ci, kinds in case.meta["empty_diags"].items():
        n = case.n(ci)
        keep = sc.keep_of(60, n)
        band, det = sc.detrend_oracle.balanced_band(case.cool, ci, keep)
        _, law, _, _ = case.expected(ci, keep)
        cis, _ = _cis_rows(case, ci)
        s = int(case.offsets[ci])
        stored = {d: [(r, r + d) for r in cis if d in cis[r]] for k in kinds.values() for d in k}
        cnt = {(int(a) - s, int(b) - s): v for a, b, v in zip(case.cool["bin1_id"], case.cool["bin2_id"], case.cool["count"])
               if s <= a < s + n and s <= b < s + n}
        for d in kinds.get("unstored", []):
            assert not stored[d] and np.isnan(law[d])
        for d in kinds.get("zeros", []):
            assert stored[d] and all(cnt[p] == 0 for p in stored[d]) and np.isnan(law[d])
        for d in kinds.get("undetectable", []):
            pos = [p for p in stored[d] if cnt[p] > 0]
            assert pos and all(not (det[p[0]] and det[p[1]]) for p in pos) and np.isnan(law[d])
        out, _, _, _ = case.expected(ci, keep)
        for k in kinds.values():
            assert not out[:, k].any()                       # every pixel of an empty-law diagonal comes out 0
        assert np.isfinite(law[0]) and np.isfinite(law[2 if name == "missing" else 8])
        counts[ci] = {k: len(v) for k, v in kinds.items()}
    print(f"{name}: empty diagonals per chromosome", counts)


def test_exact_law_case_has_exact_laws_and_pixels_on_the_cap():
    case = sc.get("cap_exact")
    assert np.all(case.cool["weight"] == 1.0)
    assert np.all(case.cool["count"] * 2 == np.rint(case.cool["count"] * 2))     # multiples of 0.5
    assert np.array_equal(case.cool["count"].astype(np.float32).astype(np.float64), case.cool["count"])
    kinds = {"at": 0, "below": 0, "above": 0}
    for ci in range(3):
        keep = sc.keep_of(60, case.n(ci))
        laws = sc.exact_law(case, ci, keep)
        out, law, _, ratio = case.expected(ci, keep)
        for d, y in enumerate(laws):
            if y is None:                                    # (the last diagonals of the shortest chromosome: no positive pixel)
                assert np.isnan(law[d]) and case.n(ci) - d < 4
                continue
            assert y == Fraction(1 if d % 2 == 0 else 2) and Fraction(float(law[d])) == y, (ci, d, y)
        for cj, r, d, kind in case.meta["cap"]:
            if cj != ci:
                continue
            assert ratio[r, d] == {"at": 10.0, "below": 9.5, "above": 10.5}[kind]
            assert out[r, d] == (9.5 if kind == "below" else 1.0)
            kinds[kind] += 1
    assert min(kinds.values()) >= 3
    print("cap_exact: pixels at / below / above the cap", kinds)


@pytest.mark.parametrize("name", sc.RANDOM_VALUED)
def test_no_random_valued_pixel_sits_on_the_cap(name):
    """|v / law - max_val| > 1e-9 max_val for every pixel of every staging (smoothed laws too): the device tests exclude nothing."""
    case = sc.get(name)
    nearest = np.inf
    for smooth, stagings in ((False, case.stagings), (True, case.smooth)):
        for st in stagings:
            for ci in case.chroms(st):
                ratio = case.expected(ci, sc.keep_of(st[0], case.n(ci)), smooth)[3]
                r = ratio[np.isfinite(ratio)]
                if r.size:
                    nearest = min(nearest, float(np.abs(r / sc.MAX_VAL - 1.0).min()))
    assert nearest > 1e-9
    print(f"{name}: nearest pixel to the cap at {nearest:.2e} relative; excluded: 0")


def test_trans_pairs_hold_what_the_metadata_says():
    case = sc.trans_genome()
    sizes = {m for m in case.meta["pairs"].values()}
    assert {0, 1, 2} <= sizes and any(m % 2 and m > 2 for m in sizes) and any(m % 2 == 0 and m > 2 for m in sizes)
    for (ca, cb), m in case.meta["pairs"].items():
        dense, med, stored = sc.trans_block(case.cool, ca, cb)
        assert stored == m and np.all(np.isfinite(dense))
        if m == 0:
            assert np.isnan(med) and not dense.any()
    assert np.all(np.isnan(case.cool["weight"][case.offsets[4]:case.offsets[5]]))
    assert not sc.trans_block(case.cool, 0, 4)[0].any()
    # tied middle values: the two middle values of an even block are the same number
    for pair in [(2, 5), (3, 5)]:
        off = case.offsets
        b1, b2 = case.cool["bin1_id"], case.cool["bin2_id"]
        sel = (b1 >= off[pair[0]]) & (b1 < off[pair[0] + 1]) & (b2 >= off[pair[1]]) & (b2 < off[pair[1] + 1])
        with np.errstate(invalid="ignore"):
            v = np.sort(np.nan_to_num(case.cool["count"][sel] * case.cool["weight"][b1[sel]] * case.cool["weight"][b2[sel]]))
        assert v.size % 2 == 0 and v[v.size // 2 - 1] == v[v.size // 2] > 0 and np.any(case.cool["count"][sel] == 0)
    print("trans: stored pixels per pair", case.meta["pairs"])
