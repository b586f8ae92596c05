"""ICE balancing (chromosight_amd/balance.py, cs_ice_balance) without a GPU: a numpy restatement of cooler.balance_cooler
that reproduces the weights stored in both committed .cool fixtures (the yardstick of tests/test_gpu_balance.py), the C ABI
of the new entry, and open_cool's argument checks."""
import ctypes
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from chromosight_amd import _lib, hdf5_lite

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"


def ice_restatement(cool, cis_only=True, mad_max=5, min_nnz=10, min_count=0, ignore_diags=2, tol=1e-5, max_iters=200,
                    rescale_marginals=True):
    """cooler.balance_cooler (store=False) in numpy: filters, initial bias, MAD filter, then the ICE loop per span (a chromosome
    with cis_only, else the genome).  Returns (weights, info) with per-span lists iterations, var, scale, converged, and
    variances: per span the list of the variance of every iteration."""
    off = np.asarray(cool["chrom_offset"], dtype=np.int64)
    n = int(off[-1])
    b1 = np.asarray(cool["bin1_id"], dtype=np.int64)
    b2 = np.asarray(cool["bin2_id"], dtype=np.int64)
    v = np.asarray(cool["count"], dtype=np.float64)
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))
    keep = np.abs(b1 - b2) >= ignore_diags
    if cis_only:
        keep &= chrom[b1] == chrom[b2]
    b1, b2, v = b1[keep], b2[keep], v[keep]

    def marginal(x):
        return np.bincount(b1, weights=x, minlength=n) + np.bincount(b2, weights=x, minlength=n)

    bias = np.ones(n)
    if min_nnz > 0:
        bias[marginal((v != 0).astype(np.float64)) < min_nnz] = 0
    marg = marginal(v)
    if min_count > 0:
        bias[marg < min_count] = 0
    if mad_max > 0:
        with np.errstate(invalid="ignore", divide="ignore"):
            parts = []
            for lo, hi in zip(off[:-1], off[1:]):
                s = marg[lo:hi]
                pos = s[s > 0]
                parts.append(s / (np.median(pos) if pos.size else np.nan))
            scaled = np.concatenate(parts) if parts else marg
            logs = np.log(scaled[scaled > 0])
            med = np.median(logs)
            dev = np.median(np.abs(logs - med))
            bias[scaled < np.exp(med - mad_max * dev)] = 0
    spans = list(zip(off[:-1], off[1:])) if cis_only else [(0, n)]
    info = {"iterations": [], "var": [], "scale": [], "converged": [], "variances": []}
    for lo, hi in spans:
        a, b = np.searchsorted(b1, [lo, hi]) if cis_only else (0, b1.size)      # (the table is sorted by bin1)
        s1, s2, sv = b1[a:b] - lo, b2[a:b] - lo, v[a:b]
        it, conv, var, nz, history = 0, False, 0.0, np.zeros(0), []
        while it < max_iters:
            it += 1
            x = sv * bias[lo + s1] * bias[lo + s2]
            m = np.bincount(s1, weights=x, minlength=hi - lo) + np.bincount(s2, weights=x, minlength=hi - lo)
            nz = m[m != 0]
            if nz.size == 0:
                bias[lo:hi] = np.nan
                var, conv = 0.0, True
                history.append(var)
                break
            m = m / nz.mean()
            m[m == 0] = 1
            bias[lo:hi] /= m
            var = nz.var()
            history.append(var)
            if var < tol:
                conv = True
                break
        scale = nz.mean() if nz.size else np.nan
        b = bias[lo:hi]
        b[b == 0] = np.nan
        if rescale_marginals:
            bias[lo:hi] = b / np.sqrt(scale)
        for k, x in zip(("iterations", "var", "scale", "converged", "variances"), (it, var, scale, conv, history)):
            info[k].append(x)
    return bias, info


def _within(got, want, rel):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = np.isfinite(want)
    return float(np.max(np.abs(got[f] - want[f]) / np.abs(want[f]))) <= rel if f.any() else True


def test_restatement_reproduces_example_cool_weights(golden):
    cool = golden("example_cool")
    attrs = hdf5_lite.File(GOLDEN / "example.cool").attrs("/bins/weight")
    assert (int(attrs["cis_only"]), int(attrs["mad_max"]), int(attrs["min_nnz"]), int(attrs["min_count"]),
            int(attrs["ignore_diags"]), float(attrs["tol"])) == (1, 5, 10, 0, 2, 1e-5)
    w, info = ice_restatement(cool)
    assert np.isnan(w).sum() == 83
    assert _within(w, cool["weight"], 1e-12)
    assert all(info["converged"])
    assert abs(info["var"][-1] - float(attrs["var"])) <= 1e-6 * float(attrs["var"])


def test_restatement_reproduces_yeast_cool_weights(golden):
    cool = golden("yeast_cool")
    w, info = ice_restatement(cool, min_nnz=0, ignore_diags=0)
    assert np.isnan(w).sum() == 333
    assert _within(w, cool["weight"], 1e-12)
    assert all(info["converged"])


def test_restatement_genome_wide_mode_runs_one_span(golden):
    w, info = ice_restatement(golden("example_cool"), cis_only=False)
    assert len(info["iterations"]) == 1 and np.isfinite(w).sum() > 0


def test_ice_abi_symbols_declared_and_exported():
    assert "cs_ice_balance" in _lib.ABI_SYMBOLS
    text = (ROOT / "include" / "chromosight_hip.h").read_text()
    assert "int cs_ice_balance(" in text
    lib = _lib.load_library()
    assert hasattr(lib, "cs_ice_balance")


def test_ice_struct_layouts_match_header(tmp_path):
    assert ctypes.sizeof(_lib.CsIceParams) == 48
    assert ctypes.sizeof(_lib.CsIceSpanStats) == 24
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = [("cs_ice_params", _lib.CsIceParams), ("cs_ice_span_stats", _lib.CsIceSpanStats)]
    fields = [("cs_ice_params", f) for f, _ in _lib.CsIceParams._fields_] + [("cs_ice_span_stats", f) for f, _ in _lib.CsIceSpanStats._fields_]
    src = tmp_path / "ice.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s%s    return 0;\n}\n' % (
        ROOT / "include" / "chromosight_hip.h",
        "".join(f'    printf("%zu\\n", sizeof({name}));\n' for name, _ in pairs),
        "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for name, f in fields)))
    exe = tmp_path / "ice"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:2] == [ctypes.sizeof(s) for _, s in pairs]
    want = [getattr(_lib.CsIceParams, f).offset for f, _ in _lib.CsIceParams._fields_] + \
        [getattr(_lib.CsIceSpanStats, f).offset for f, _ in _lib.CsIceSpanStats._fields_]
    assert out[2:] == want


@pytest.mark.parametrize("norm", ["balanced", "ice", "", "Auto"])
def test_open_cool_rejects_unknown_norm(norm):
    from chromosight_amd import pipeline
    with pytest.raises(ValueError, match="norm must be one of: auto, raw, force"):
        pipeline.open_cool(GOLDEN / "example.cool", norm=norm)


def test_load_cool_still_refuses_force():
    from chromosight_amd import io as cio
    with pytest.raises(ValueError, match="not part of this package"):
        cio.load_cool(GOLDEN / "example.cool", norm="force")


def test_private_reader_keeps_the_stored_column_or_none(golden):
    from chromosight_amd import io as cio
    stored = cio._read_cool(GOLDEN / "example.cool")
    assert np.array_equal(stored["weight"], golden("example_cool")["weight"], equal_nan=True)
    assert cio._read_cool(GOLDEN / "example.cool", balance="KR")["weight"] is None
    assert np.array_equal(stored["count"], golden("example_cool")["count"])
