"""ICE balancing on the device (chromosight_amd/balance.py -> cs_ice_balance, cs_balance.hip) against the weights stored in the
committed .cool fixtures and the numpy restatement of tests/test_balance_host.py; pipeline.open_cool end to end."""
import copy
import warnings

import numpy as np
import pytest

import chromosight_amd.kernels as ck
from chromosight_amd import pipeline
from chromosight_amd.balance import ConvergenceWarning, ice_balance
from test_balance_host import GOLDEN, ice_restatement

pytestmark = pytest.mark.gpu


def unbalanced(cool):
    cool = dict(cool)
    cool.pop("weight", None)
    return cool


def assert_weights(got, want, rel=1e-9):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = np.isfinite(want)
    if f.any():
        err = float(np.max(np.abs(got[f] - want[f]) / np.abs(want[f])))
        assert err <= rel, err


def assert_info(info, ref):
    assert list(info["iterations"]) == list(ref["iterations"])
    assert list(info["converged"]) == list(ref["converged"])
    np.testing.assert_allclose(info["var"], ref["var"], rtol=1e-6, atol=1e-300)
    np.testing.assert_allclose(info["scale"], ref["scale"], rtol=1e-9)


def test_example_cool_stored_weights(golden):
    cool = golden("example_cool")
    w, info = ice_balance(pipeline.DeviceCool(unbalanced(cool)))
    assert_weights(w, cool["weight"])
    _, ref = ice_restatement(cool)
    assert_info(info, ref)


def test_yeast_cool_stored_weights(golden):
    cool = golden("yeast_cool")
    w, info = ice_balance(pipeline.DeviceCool(unbalanced(cool)), min_nnz=0, ignore_diags=0)
    assert_weights(w, cool["weight"])
    _, ref = ice_restatement(cool, min_nnz=0, ignore_diags=0)
    assert_info(info, ref)


@pytest.fixture(scope="module")
def synthetic():
    """~20 000 bins: float64 counts, a chromosome without pixels, one whose bins all fail min_nnz = 10."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, str(ROOT / "tools"))
    from synthetic_genome import make_cool
    cool, _ = make_cool(total_bins=20_000, max_dist_bins=60, seed=5)
    off = cool["chrom_offset"]
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    chrom = np.repeat(np.arange(off.size - 1), np.diff(off))[b1]
    d = b2 - b1
    keep = (chrom != 3) & ((chrom != 7) | ((d >= 2) & (d <= 5)))        # chr4: no pixel; chr8: <= 8 pixels per bin beyond diagonal 1
    rng = np.random.default_rng(11)
    cool = dict(cool)
    cool["bin1_id"], cool["bin2_id"] = b1[keep], b2[keep]
    cool["count"] = cool["count"][keep] * rng.uniform(0.5, 1.5, int(keep.sum()))
    cool.pop("weight")
    return cool


@pytest.mark.parametrize("fixture", ["example_cool", "yeast_cool", "synthetic"])
@pytest.mark.parametrize("kw", [dict(cis_only=False), dict(min_count=50)], ids=["genome_wide", "min_count"])
def test_against_restatement(golden, synthetic, fixture, kw):
    cool = synthetic if fixture == "synthetic" else unbalanced(golden(fixture))
    dcool = pipeline.DeviceCool(cool)
    if fixture == "synthetic":
        assert dcool.val_dtype == np.float64
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        w, info = ice_balance(dcool, **kw)
    want, ref = ice_restatement(cool, **kw)
    assert_weights(w, want)
    assert_info(info, ref)
    if fixture == "synthetic" and kw.get("cis_only", True):
        off = cool["chrom_offset"]
        assert np.isnan(w[off[3]:off[4]]).all() and info["var"][3] == 0 and np.isnan(info["scale"][3])
        assert np.isnan(w[off[7]:off[8]]).all()
        assert np.isfinite(w).sum() > 0.9 * (off[-1] - (off[4] - off[3]) - (off[8] - off[7]))


def test_synthetic_cis_default(synthetic):
    w, info = ice_balance(pipeline.DeviceCool(synthetic))
    want, ref = ice_restatement(synthetic)
    assert_weights(w, want)
    assert_info(info, ref)
    off = synthetic["chrom_offset"]
    assert np.isnan(w[off[3]:off[4]]).all() and info["var"][3] == 0 and np.isnan(info["scale"][3])
    assert np.isnan(w[off[7]:off[8]]).all()


def test_iteration_limit_warns(golden):
    cool = golden("example_cool")
    with pytest.warns(ConvergenceWarning):
        w, info = ice_balance(pipeline.DeviceCool(unbalanced(cool)), max_iters=3)
    assert not info["converged"].any() and list(info["iterations"]) == [3, 3, 3]
    want, ref = ice_restatement(cool, max_iters=3)
    assert_weights(w, want)
    assert_info(info, ref)


def test_bitwise_deterministic(golden):
    cool = unbalanced(golden("yeast_cool"))
    a = pipeline.DeviceCool(cool)
    w1, _ = ice_balance(a, min_nnz=0, ignore_diags=0)
    w2, _ = ice_balance(a, min_nnz=0, ignore_diags=0)
    w3, _ = ice_balance(pipeline.DeviceCool(cool), min_nnz=0, ignore_diags=0)
    assert w1.tobytes() == w2.tobytes() == w3.tobytes()


def test_bad_arguments(golden):
    dcool = pipeline.DeviceCool(unbalanced(golden("example_cool")))
    with pytest.raises(ValueError, match="tol"):
        ice_balance(dcool, tol=0)
    with pytest.raises(ValueError, match="max_iters"):
        ice_balance(dcool, max_iters=0)
    cool = unbalanced(golden("example_cool"))
    b1, b2 = cool["bin1_id"], cool["bin2_id"]
    cool["bin1_id"], cool["bin2_id"] = np.maximum(b1, b2), np.minimum(b1, b2)        # lower triangle
    with pytest.raises(ValueError, match="upper-triangle"):
        ice_balance(pipeline.DeviceCool(cool))


def test_weightless_table_is_not_staged(golden):
    dcool = pipeline.DeviceCool(unbalanced(golden("example_cool")))
    assert not dcool.has_weights
    with pytest.raises(ValueError, match="no balancing weights"):
        pipeline.detect(dcool, copy.deepcopy(ck.loops))


TABLES = [("example_loops", dict(pattern="loops", min_dist=8000, max_dist=50000, pearson=0.35)),
          ("example_borders", dict(pattern="borders")), ("example_hairpins", dict(pattern="hairpins"))]


def _written(cool, tmp_path, tag):
    out = {}
    for name, overrides in TABLES:
        overrides = dict(overrides)
        cfg = copy.deepcopy(getattr(ck, overrides.pop("pattern")))
        cfg.update(overrides)
        pipeline.detect_to_files(cool, cfg, str(tmp_path / f"{tag}_{name}"), win_fmt="npy")
        out[name] = (tmp_path / f"{tag}_{name}.tsv").read_text()
    return out


def test_open_cool_unbalanced_file_end_to_end(golden, tmp_path):
    """A file without the weight column (balance="KR" is absent from example.cool) balanced on the device: the tables detect
    writes are the ones the stored weights give, and the committed .tsv files of the reference as the balanced file matches them."""
    dcool = pipeline.open_cool(GOLDEN / "example.cool", balance="KR")
    assert_weights(dcool.host["weight"], golden("example_cool")["weight"])
    got = _written(dcool, tmp_path, "ice")
    base = _written(pipeline.open_cool(GOLDEN / "example.cool"), tmp_path, "stored")
    for name, _ in TABLES:
        ref = (GOLDEN / f"{name}.tsv").read_text().splitlines()
        g, b = got[name].splitlines(), base[name].splitlines()
        assert len(g) == len(b) == len(ref) and g[0] == ref[0]
        for x, y, r in zip(g[1:], b[1:], ref[1:]):
            fx, fy, fr = x.split("\t"), y.split("\t"), r.split("\t")
            assert fx[:10] == fy[:10] == fr[:10], (x, r)
            for u, v in zip(fx[10:], fy[10:]):
                assert abs(float(u) - float(v)) <= 1.5e-10, (x, y)
        assert sum(x == y for x, y in zip(g, b)) >= 0.95 * len(g)


def test_open_cool_force_and_raw(golden, tmp_path):
    stored = golden("example_cool")["weight"]
    forced = pipeline.open_cool(GOLDEN / "example.cool", norm="force")
    assert_weights(forced.host["weight"], stored)
    a = _written(forced, tmp_path, "force")
    b = _written(pipeline.open_cool(GOLDEN / "example.cool"), tmp_path, "auto")
    for name, _ in TABLES:
        assert [l.split("\t")[:10] for l in a[name].splitlines()] == [l.split("\t")[:10] for l in b[name].splitlines()]
    raw = pipeline.open_cool(GOLDEN / "example.cool", balance="KR", norm="raw")
    w = raw.host["weight"]
    assert np.array_equal(np.isfinite(w), np.isfinite(stored))
    assert (w[np.isfinite(w)] == 1.0).all()
    raw_stored = pipeline.open_cool(GOLDEN / "example.cool", norm="raw")
    assert np.array_equal(raw_stored.host["weight"], w, equal_nan=True)
