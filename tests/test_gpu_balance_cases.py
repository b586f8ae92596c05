"""ICE balancing on the device (cs_ice_balance, cs_balance.hip) on the edge-case tables of tests/balance_cases.py, which
tests/test_balance_cases_host.py pins on the CPU: every case against ice_restatement at the bounds of tests/test_gpu_balance.py,
then properties that need no reference -- the weights of a chromosome do not depend on where it lies in the genome, counts
times 4 give the same iterations and weights halved or equal bit for bit, a float64 container gives the float32 one's bits --
and the refusals of the C ABI.

Relocation.  Every sum of cs_balance.hip but one is laid out from the chromosome's first bin (the chunks) and the span's first
chunk (ice_span_kernel).  The exception is the column half of a marginal: ice_marg_kernel deals the entries of CSC column c
to the lanes from colptr[c] on, and under cis_only the trans pixels above the chromosome stay in the column, as zeros in
front of the cis pixels.  So the lane a cis pixel adds into depends on how many trans pixels are stored above it, and with
it the rounding of the wave's sum.  A table without trans pixels, and any move that leaves every column as it is, give the
same bits wherever the chromosome lies (asserted); chromosomes that change places with trans pixels stored between them agree
to the suite's 1e-9 only (asserted, the differing weights counted in the output: 193 of the 290 of `trans_cis`, 315 of the 543
of `wide_d3`).  The kernel promises the same bits from call to call, not from place to place: it was left as it is."""
import ctypes as C
import warnings

import numpy as np
import pytest

import balance_cases as bc
from chromosight_amd import pipeline
from chromosight_amd._lib import CsCsr, CsIceParams, CsIceSpanStats
from chromosight_amd.balance import ConvergenceWarning, ice_balance
from test_gpu_balance import assert_info, assert_weights

pytestmark = pytest.mark.gpu


def balanced(cool, dcool=None, **kw):
    """(weights, info, the chromosomes -- or "genome" -- a ConvergenceWarning was issued for)."""
    dcool = dcool or pipeline.DeviceCool(cool)
    assert not dcool.has_weights
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        w, info = ice_balance(dcool, **kw)
    assert all(issubclass(c.category, ConvergenceWarning) for c in caught), [str(c.message) for c in caught]
    warned = [str(c.message).split(":")[0].replace("ICE balancing of ", "") for c in caught]
    return w, info, warned


def expected_warnings(cool, ref, kw):
    if not kw.get("cis_only", True):
        return ["the genome"] * len(bc.unconverged(ref))
    return [f"chromosome {cool['chrom_names'][k]}" for k in bc.unconverged(ref)]


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_case_equals_the_restatement(name):
    case = bc.BY_NAME[name]
    want, ref = case.reference
    dcool = pipeline.DeviceCool(case.cool)
    assert dcool.val_dtype is np.float32 and dcool.upper
    w, info, warned = balanced(case.cool, dcool, **case.kw)
    f = np.isfinite(want)
    err = float(np.max(np.abs(w[f] - want[f]) / np.abs(want[f]))) if f.any() and np.array_equal(np.isnan(w), np.isnan(want)) else np.nan
    print(f"{name}: {int(f.sum())} weights, worst relative error {err:.2e}; iterations {[int(k) for k in info['iterations']]}, "
          f"var {[float(f'{v:.4g}') for v in info['var']]}")
    assert_weights(w, want)
    assert_info(info, ref)
    assert warned == expected_warnings(case.cool, ref, case.kw)
    assert np.array_equal(dcool.data.download()[:dcool.nnz], case.cool["count"].astype(np.float32))          # the table is left alone


def _per_chromosome(cool, w, start=None):
    off = cool["chrom_offset"]
    start = off[:-1] if start is None else start
    return [w[s:s + hi - lo] for s, lo, hi in zip(start, off[:-1], off[1:])]


@pytest.mark.parametrize("name", ["geometry_d0", "trans_cis", "nothing_d0", "mad_default"])
def test_relocated_chromosomes_get_the_same_bits(name):
    """cis_only: the chromosomes reversed, behind a chromosome of no bin and one of 70 bins without a pixel."""
    case = bc.BY_NAME[name]
    assert case.kw.get("cis_only", True)
    cool = bc.without_trans(case.cool)
    n_chrom = cool["chrom_offset"].size - 1
    w, info, warned = balanced(cool, **case.kw)
    moved, start = bc.relocate(cool, range(n_chrom)[::-1], front=(0, 70))
    wm, infom, warned_m = balanced(moved, **case.kw)
    assert np.isfinite(w).sum() > 0.5 * w.size and np.isnan(wm[:70]).all()
    for k, (a, b) in enumerate(zip(_per_chromosome(cool, w), _per_chromosome(cool, wm, start))):
        assert a.tobytes() == b.tobytes(), (name, k, int((a != b).sum()))
    for key in ("iterations", "converged", "var", "scale"):
        assert np.array_equal(np.asarray(infom[key])[2:][::-1], np.asarray(info[key]), equal_nan=True), key
    assert list(infom["iterations"][:2]) == [1, 1] and sorted(warned_m) == sorted(warned)


@pytest.mark.parametrize("name", ["trans_cis", "wide_d3"])
def test_relocation_with_trans_pixels_stored(name):
    """Trans pixels kept in the table: moving the whole genome behind pixel-less chromosomes leaves every CSC column as it
    is -- the same bits; reversing the chromosomes changes how many zeroed trans entries precede a column's cis pixels (the
    module docstring) -- the suite's bound."""
    case = bc.BY_NAME[name]
    cool = case.cool
    n_chrom = cool["chrom_offset"].size - 1
    w, info, _ = balanced(cool, **case.kw)
    shifted, start = bc.relocate(cool, range(n_chrom), front=(0, 70))
    ws, infos, _ = balanced(shifted, **case.kw)
    for a, b in zip(_per_chromosome(cool, w), _per_chromosome(cool, ws, start)):
        assert a.tobytes() == b.tobytes()
    assert list(infos["iterations"][2:]) == list(info["iterations"])
    moved, start = bc.relocate(cool, range(n_chrom)[::-1], front=(0,))
    wm, infom, _ = balanced(moved, **case.kw)
    back = np.concatenate(_per_chromosome(cool, wm, start))
    differ = int(((back != w) & np.isfinite(w)).sum())
    print(f"{name}: reversed with trans pixels stored, {differ} of {int(np.isfinite(w).sum())} weights differ in their bits")
    assert_weights(back, w)
    assert list(infom["iterations"][1:][::-1]) == list(info["iterations"])


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("name", ["trans_cis", "mad_min_count", "timing"])
def test_counts_times_four(name, rescale):
    """Every marginal, mean and variance scales by a power of two: the same iterations, the weights exactly half (rescaled by
    1 / sqrt(4 mean)) or exactly equal."""
    case = bc.BY_NAME[name]
    kw = dict(case.kw, rescale_marginals=rescale)
    kw.setdefault("min_count", 50)
    times4 = dict(case.cool, count=case.cool["count"] * 4)
    kw4 = dict(kw, tol=kw.get("tol", 1e-5) * 16, min_count=kw["min_count"] * 4)
    w, info, warned = balanced(case.cool, **kw)
    w4, info4, warned4 = balanced(times4, **kw4)
    assert np.isnan(w).any() and np.isfinite(w).sum() > 0.8 * w.size
    assert list(info4["iterations"]) == list(info["iterations"]) and list(info4["converged"]) == list(info["converged"])
    assert warned4 == warned
    assert (w4 * 2 if rescale else w4).tobytes() == w.tobytes()
    assert np.array_equal(info4["var"], 16 * info["var"]) and np.array_equal(info4["scale"], 4 * info["scale"], equal_nan=True)


@pytest.mark.parametrize("name", ["wide_d3", "geometry_genome"])
def test_float64_container_gives_the_same_bits(name):
    case = bc.BY_NAME[name]
    a = pipeline.DeviceCool(case.cool)
    data64 = a.dev.to_device(case.cool["count"], np.float64)
    b = pipeline.DeviceCool.from_device_csr(a, a.indptr, a.indices, data64, a.nnz, np.float64, weight=None)
    assert a.val_dtype is np.float32 and b.val_dtype is np.float64 and not b.has_weights
    assert a.csr().dtype != b.csr().dtype
    wa, ia, _ = balanced(case.cool, a, **case.kw)
    wb, ib, _ = balanced(case.cool, b, **case.kw)
    assert np.isfinite(wa).sum() > 0.9 * wa.size and wa.tobytes() == wb.tobytes()
    for key in ("iterations", "converged", "var", "scale"):
        assert np.array_equal(ia[key], ib[key], equal_nan=True), key


def test_abi_refusals():
    """The refusals of cs_ice_balance that tests/test_gpu_balance.py does not reach (it has tol, max_iters and the lower
    triangle): each returns non-zero with a message, and neither the weights nor the statistics are written."""
    cool = bc.table("trans")
    dcool = pipeline.DeviceCool(cool)
    dev, n = dcool.dev, dcool.n_bins
    n_chrom = cool["chrom_offset"].size - 1
    offsets = np.ascontiguousarray(cool["chrom_offset"], dtype=np.int64)
    bias = dev.to_device(np.full(n, 7.0))
    good = dict(cis_only=1, ignore_diags=2, min_nnz=10, max_iters=200, min_count=0.0, mad_max=5.0, tol=1e-5, rescale_marginals=1, reserved=0)

    def call(g="table", off=offsets, chroms=n_chrom, p="params", out="bias", stats="stats", **changed):
        g = dcool.csr() if g == "table" else g
        p = CsIceParams(**dict(good, **changed)) if p == "params" else p
        rows = (CsIceSpanStats * n_chrom)()
        for r in rows:
            r.iterations = -5
        with dev.lock:
            rc = dev.lib.cs_ice_balance(dev.ctx, None, None if g is None else C.byref(g),
                                        None if off is None else off.ctypes.data_as(C.POINTER(C.c_int64)), chroms,
                                        None if p is None else C.byref(p), bias.ptr if out == "bias" else None,
                                        rows if stats == "stats" else None)
            msg = dev.lib.cs_last_error(dev.ctx).decode("utf-8", "replace")
        dev.sync()
        return rc, msg, all(r.iterations == -5 for r in rows) and bool(np.all(bias.download() == 7.0))

    def view(**fields):
        g = dcool.csr()
        for k, v in fields.items():
            setattr(g, k, v)
        return g

    some = dcool.indptr.ptr
    refused = {
        "null table": (dict(g=None), "null argument"), "null offsets": (dict(off=None), "null argument"),
        "null parameters": (dict(p=None), "null argument"), "null weights": (dict(out=None), "null argument"),
        "null statistics": (dict(stats=None), "null argument"),
        "not square": (dict(g=view(n_cols=n - 1)), "square"), "column origin": (dict(g=view(col0=1)), "square"),
        "row_end attached": (dict(g=view(d_row_end=some)), "no weights"),
        "row weights attached": (dict(g=view(d_row_weight=some)), "no weights"),
        "column weights attached": (dict(g=view(d_col_weight=some)), "no weights"),
        "offsets not from 0": (dict(off=offsets + 1), "must run from 0"),
        "offsets not to n": (dict(chroms=n_chrom - 1), "must run from 0"),
        "no chromosome": (dict(chroms=0), "must run from 0"),
        "decreasing offsets": (dict(off=np.array([0, 200, 100, 300], dtype=np.int64)), "decreasing"),
        "negative ignore_diags": (dict(ignore_diags=-1), "must be >= 0"), "negative min_nnz": (dict(min_nnz=-1), "must be >= 0"),
        "NaN min_count": (dict(min_count=float("nan")), "must be >= 0"), "NaN mad_max": (dict(mad_max=float("nan")), "must be >= 0"),
        "negative mad_max": (dict(mad_max=-1.0), "must be >= 0"), "reserved": (dict(reserved=1), "reserved must be 0"),
    }
    assert offsets.tolist() == [0, 100, 180, 300] and isinstance(dcool.csr(), CsCsr)
    for what, (args, text) in refused.items():
        rc, msg, untouched = call(**args)
        assert rc != 0 and "cs_ice_balance" in msg and text in msg and untouched, (what, rc, msg, untouched)
    rc, msg, untouched = call()                             # the same call with nothing wrong balances the table
    assert rc == 0 and not untouched
    assert_weights(bias.download()[:n], bc.BY_NAME["trans_cis"].reference[0])
