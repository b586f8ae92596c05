"""The ICE balancing cases (tests/balance_cases.py) pinned on the CPU before any device sees them: ice_restatement, the
yardstick of the device tests, agrees with a dense extended-precision reference that shares no code with it; every case
reaches the branch it is named for; and no variance of any iteration sits within 1e-3 of tol, so that a device variance
within the suite's 1e-6 of the reference's cannot stop a span one iteration earlier or later."""
import numpy as np
import pytest

import balance_cases as bc
from test_balance_host import ice_restatement

GUARD = 1e-3


def _chrom(cool):
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    return off, np.repeat(np.arange(off.size - 1), np.diff(off))


def _kept(cool, ignore_diags, cis_only=True):
    """(bin1, bin2, count) of the pixels the balancing keeps."""
    _, chrom = _chrom(cool)
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    keep = b2 - b1 >= ignore_diags
    if cis_only:
        keep &= chrom[b1] == chrom[b2]
    return b1[keep], b2[keep], cool["count"][keep]


def _case(name):
    case = bc.BY_NAME[name]
    return (case,) + case.reference


@pytest.mark.parametrize("name", bc.DENSE)
def test_restatement_equals_the_dense_reference(name):
    case, w, info = _case(name)
    want, ref = bc.dense_reference(case.cool, **case.kw)
    assert np.array_equal(np.isnan(w), np.isnan(want))
    f = np.isfinite(want)
    err = float(np.max(np.abs(w[f] - want[f]) / np.abs(want[f]))) if f.any() else 0.0
    print(f"{name}: {int(f.sum())} weights, worst relative difference {err:.2e}; iterations {info['iterations']}")
    assert err <= 1e-12
    assert list(info["iterations"]) == list(ref["iterations"]) and list(info["converged"]) == list(ref["converged"])
    np.testing.assert_allclose(info["var"], ref["var"], rtol=1e-6, atol=1e-300)
    np.testing.assert_allclose(info["scale"], ref["scale"], rtol=1e-9)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_no_variance_sits_near_tol(name):
    """A condition on the inputs: the variance of EVERY iteration of every span (the deciding one and the one before it among
    them) lies outside tol * [1 - 1e-3, 1 + 1e-3]."""
    case, _, info = _case(name)
    tol = case.kw.get("tol", 1e-5)
    margins = [abs(v / tol - 1.0) for history in info["variances"] for v in history]
    assert [len(h) for h in info["variances"]] == list(info["iterations"])
    for history, conv, var in zip(info["variances"], info["converged"], info["var"]):
        assert history[-1] == var and all(v >= tol for v in history[:-1]) and (var < tol) == conv
    print(f"{name}: nearest variance to tol at {min(margins):.2e} relative")
    assert min(margins) > GUARD


def test_case_table_covers_the_parameters():
    kws = [c.kw for c in bc.CASES]
    assert {0, 1, 2, 3, 7} <= {kw.get("ignore_diags", 2) for kw in kws}
    assert any(kw.get("mad_max", 5) == 0 for kw in kws) and any(kw.get("rescale_marginals") is False for kw in kws)
    assert any(kw.get("cis_only") is False for kw in kws) and any(kw.get("tol", 1e-5) > 1e-5 for kw in kws)
    assert len({c.name for c in bc.CASES}) == len(bc.CASES) and all(c.purpose for c in bc.CASES)
    for name, args in bc.TABLES.items():
        cool = bc.table(name)
        again = bc.make_table(**args)
        assert all(np.array_equal(cool[k], again[k]) for k in ("bin1_id", "bin2_id", "count", "chrom_offset")), name
        b1, b2, cnt = cool["bin1_id"], cool["bin2_id"], cool["count"]
        assert cnt.dtype == np.int32 and cnt.min() >= 0 and "weight" not in cool
        assert np.all(b2 >= b1) and np.all(np.diff(b1 * int(cool["chrom_offset"][-1]) + b2) > 0), name
        assert cool["chrom_offset"][-1] <= 600 or name == "long"


def test_geometry_chunks():
    case, w, info = _case("geometry_d2")
    off, _ = _chrom(case.cool)
    assert np.diff(off).tolist() == [1, 63, 64, 65, 0, 129]
    for s in (0, 4):                                        # nothing beyond diagonal 1 in one bin; no bin at all
        assert info["var"][s] == 0 and np.isnan(info["scale"][s]) and info["converged"][s] and info["iterations"][s] == 1
    assert np.isnan(w[0]) and all(np.isfinite(w[off[s]:off[s + 1]]).sum() > 0.8 * (off[s + 1] - off[s]) for s in (1, 2, 3, 5))
    _, w0, info0 = _case("geometry_d0")
    assert np.isfinite(w0[0]) and info0["iterations"][0] == 1 and info0["var"][0] == 0 and np.isfinite(info0["scale"][0])
    assert np.isnan(info0["scale"][4])
    _, wg, infog = _case("geometry_genome")
    assert len(infog["iterations"]) == 1 and np.isfinite(wg).sum() > 300


@pytest.mark.parametrize("d", [1, 3, 7])
def test_wide_rows_and_columns_wrap_the_lane_loops(d):
    case, w, info = _case(f"wide_d{d}")
    assert case.kw["ignore_diags"] == d
    b1, b2, cnt = _kept(case.cool, d)
    n = int(case.cool["chrom_offset"][-1])
    rows, cols = np.bincount(b1, minlength=n), np.bincount(b2, minlength=n)
    print(f"wide_d{d}: longest kept row {rows.max()}, longest kept column {cols.max()}")
    assert rows.max() > 128 and cols.max() > 128
    dist = case.cool["bin2_id"] - case.cool["bin1_id"]
    long_rows = np.flatnonzero(rows > 128)
    for edge in (d - 1, d):                                 # the filter cuts into a long row: pixels on both sides of it
        assert np.isin(case.cool["bin1_id"][(dist == edge) & (case.cool["count"] > 0)], long_rows).any()
    assert all(info["converged"]) and np.isfinite(w).sum() > 500


def test_trans_pixels_straddle_the_last_bin():
    case, w, info = _case("trans_cis")
    cool = case.cool
    off, chrom = _chrom(cool)
    b1, b2, cnt = cool["bin1_id"], cool["bin2_id"], cool["count"]
    assert (chrom[b1] != chrom[b2]).sum() > 500
    for k in (0, 1):                                        # a pixel whose column is the first bin behind the row's chromosome
        hi = off[k + 1]
        at = (chrom[b1] == k) & (b2 == hi) & (cnt > 0) & np.isfinite(w[b1]) & np.isfinite(w[hi])
        assert at.any(), k
        rows = [b2[b1 == r] for r in b1[at]]                # one of them holds cis pixels, then several trans pixels
        assert any((row < hi).sum() >= 3 and (row >= hi).sum() >= 2 for row in rows), k
    _, wg, _ = _case("trans_genome_no_rescale")
    assert np.isfinite(wg).sum() >= np.isfinite(w).sum()


def test_mad_filter_removes_bins_that_mad_max_0_keeps():
    _, w, _ = _case("mad_default")
    _, w_off, _ = _case("mad_off")
    lost = np.isnan(w) & np.isfinite(w_off)
    print(f"mad: {int(lost.sum())} bins lost to the MAD filter: {np.flatnonzero(lost).tolist()}")
    assert lost.sum() >= 1 and not np.isnan(w_off).any()
    assert set(bc.MAD_BINS) <= set(np.flatnonzero(lost).tolist())
    case, w_cnt, _ = _case("mad_min_count")
    assert set(np.flatnonzero(np.isnan(w_cnt)).tolist()) == set(bc.MAD_BINS)
    b1, b2, cnt = _kept(case.cool, 2)
    total = np.bincount(b1, weights=cnt, minlength=w.size) + np.bincount(b2, weights=cnt, minlength=w.size)
    on_it = total == case.kw["min_count"]                   # `marginal < min_count` drops: a bin ON min_count stays
    assert on_it.sum() == 1 and np.isfinite(w_cnt[on_it]).all() and np.all(total[bc.MAD_BINS] < case.kw["min_count"])


def test_bins_of_exactly_min_nnz_pixels_are_kept():
    case, w, info = _case("nothing_min_nnz4")
    off, _ = _chrom(case.cool)
    b1, b2, cnt = _kept(case.cool, 2)
    nonzero = np.bincount(b1, weights=cnt != 0, minlength=w.size) + np.bincount(b2, weights=cnt != 0, minlength=w.size)
    inside = slice(off[1], off[2])                          # chromosome 1: diagonals 2 and 3 remain, two pixels each way
    assert (nonzero[inside] == 4).sum() > 40 and np.isfinite(w[inside][nonzero[inside] == 4]).all()
    assert (nonzero[inside] == 3).sum() >= 2 and np.isnan(w[inside][nonzero[inside] < 4]).all()


def test_min_nnz_loses_bins_only_because_zeros_are_stored():
    case, w, _ = _case("zeros_min_nnz")
    min_nnz = 10
    b1, b2, cnt = _kept(case.cool, 2)
    n = w.size
    stored = np.bincount(b1, minlength=n) + np.bincount(b2, minlength=n)
    nonzero = np.bincount(b1, weights=cnt != 0, minlength=n) + np.bincount(b2, weights=cnt != 0, minlength=n)
    w_free, _ = ice_restatement(case.cool, **dict(case.kw, min_nnz=0))
    lost = np.isnan(w) & np.isfinite(w_free)
    print(f"zeros: {int(lost.sum())} bins lost to min_nnz, {int((case.cool['count'] == 0).sum())} zeros stored")
    assert lost.sum() >= len(bc.ZERO_BINS) and set(bc.ZERO_BINS) <= set(np.flatnonzero(lost).tolist())
    assert np.all(stored[lost] >= min_nnz) and np.all(nonzero[lost] < min_nnz)
    assert not (np.isfinite(w) & (nonzero < min_nnz)).any()


def test_spans_with_nothing_to_keep():
    case, w, info = _case("nothing_d2")
    cool = case.cool
    off, chrom = _chrom(cool)
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    cis = chrom[b1] == chrom[b2]
    assert (cis & (chrom[b1] == 1)).sum() > 150                                              # pixels, too few per bin
    assert (cis & (chrom[b1] == 3)).sum() == 50 and np.all((b1 == b2)[cis & (chrom[b1] == 3)])    # the diagonal, whole
    assert not ((chrom[b1] == 5) | (chrom[b2] == 5)).any()
    for s in (1, 3, 5):
        assert info["var"][s] == 0 and np.isnan(info["scale"][s]) and np.isnan(w[off[s]:off[s + 1]]).all()
    for s in (0, 2, 4):
        assert info["converged"][s] and info["var"][s] > 0 and np.isfinite(w[off[s]:off[s + 1]]).any()


def test_diagonal_only_span_oscillates_beside_converging_ones():
    case, w, info = _case("nothing_d0")
    assert not info["converged"][3] and info["iterations"][3] == case.kw["max_iters"] == 100
    assert info["converged"][2] and info["converged"][4] and max(info["iterations"][2], info["iterations"][4]) < 100
    h = info["variances"][3]
    assert h[-1] > h[0] and np.isfinite(w[case.cool["chrom_offset"][3]:case.cool["chrom_offset"][4]]).all()
    assert info["iterations"][5] == 1 and info["var"][5] == 0
    assert bc.unconverged(info) == [1, 3]


def test_spans_stop_at_very_different_iterations():
    _, _, info = _case("timing")
    done = [it for it, conv in zip(info["iterations"], info["converged"]) if conv]
    assert len(done) >= 2 and max(done) >= 3 * min(done) and min(done) > 1
    _, _, loose = _case("trans_loose_tol")
    _, _, tight = _case("trans_cis")
    assert all(a < b for a, b in zip(loose["iterations"], tight["iterations"])) and all(loose["converged"])
    _, _, genome = _case("trans_genome_no_rescale")
    assert genome["converged"] == [True]


def test_long_span_takes_the_second_trip():
    case, w, info = _case("long_span")
    cool = case.cool
    off, chrom = _chrom(cool)
    n0 = int(off[1])
    assert n0 >= 16_449 and -(-n0 // 64) > 256 and cool["count"].size < 100_000
    cis0 = (chrom[cool["bin1_id"]] == 0) & (chrom[cool["bin2_id"]] == 0)
    assert (cool["bin2_id"] - cool["bin1_id"])[cis0].max() <= 3
    assert np.isfinite(w[16_384:n0]).sum() > 50            # the chunks of the second trip hold weights
    assert info["iterations"][0] > 1


def test_relocation_keeps_every_pixel():
    cool = bc.table("trans")
    moved, start = bc.relocate(cool, [2, 1, 0], front=(0, 70))
    off = cool["chrom_offset"]
    assert moved["chrom_offset"].tolist() == [0, 0, 70, 190, 270, 370] and start.tolist() == [270, 190, 70]
    assert np.all(moved["bin2_id"] >= moved["bin1_id"]) and moved["count"].sum() == cool["count"].sum()
    w, info = ice_restatement(cool)
    wm, infom = ice_restatement(moved)
    for k in range(3):
        a, b = w[off[k]:off[k + 1]], wm[start[k]:start[k] + off[k + 1] - off[k]]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
    assert infom["iterations"][2:] == info["iterations"][::-1] and np.isnan(wm[:70]).all()
    assert (bc.without_trans(cool)["count"].size, cool["count"].size) == (int((np.searchsorted(off, cool["bin1_id"], "right")
                                                                                == np.searchsorted(off, cool["bin2_id"], "right")).sum()), 7053)
