"""Trans blocks in row strips, host side: the occupancy rule of cs_csr_tile_occupancy restated in numpy against brute-force
dilation, the strip plan of an inter_budget, and the new C entries in the header and the binding.  No GPU."""
import pathlib
import re

import numpy as np
import pytest

from chromosight_amd import _lib, pipeline
from tools.synthetic_inter import occupancy_brute, occupancy_reference

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _random_block(rng, n_r, n_c, density, edges=False):
    n = max(0, int(n_r * n_c * density))
    rows, cols = rng.integers(0, n_r, n), rng.integers(0, n_c, n)
    if edges:                       # nonzeros on the first / last rows and columns
        rows = np.concatenate([rows, [0, n_r - 1, 0, n_r - 1]])
        cols = np.concatenate([cols, [0, 0, n_c - 1, n_c - 1]])
    vals = rng.choice([0.0, 1.0, 2.0, np.nan], size=rows.size, p=[0.2, 0.5, 0.2, 0.1])
    row_w = np.where(rng.random(n_r) < 0.1, np.nan, 1.0)
    col_w = np.where(rng.random(n_c) < 0.1, np.nan, 1.0)
    return rows, cols, vals, row_w, col_w


def _dense_ok(n_r, n_c, rows, cols, vals, row_w, col_w):
    ok = np.zeros((n_r, n_c), dtype=bool)
    with np.errstate(invalid="ignore"):
        s = (vals > 0) & np.isfinite(row_w[rows]) & np.isfinite(col_w[cols])
    ok[rows[s], cols[s]] = True
    return ok


@pytest.mark.parametrize("shape,density,tmpl,window,edges", [
    ((300, 260), 0.0, (17, 17), None, False),          # empty block
    ((300, 260), 2e-4, (17, 17), None, True),          # nonzeros on the block's edges
    ((300, 260), 5e-4, (17, 17), (100, 190), True),    # a row window: nonzeros on its halo rows count
    ((12, 500), 1e-2, (17, 17), None, True),           # narrower than the template
    ((500, 9), 1e-2, (17, 17), None, True),
    ((333, 401), 3e-4, (7, 17), None, False),          # non-square templates
    ((333, 401), 3e-4, (21, 5), (64, 257), True),
    ((200, 200), 1e-3, (1, 1), None, True),
])
def test_occupancy_rule_matches_brute_force_dilation(shape, density, tmpl, window, edges):
    rng = np.random.default_rng(abs(hash((shape, density, tmpl, window))) % 2 ** 32)
    n_r, n_c = shape
    km, kn = tmpl
    rows, cols, vals, row_w, col_w = _random_block(rng, n_r, n_c, density, edges)
    a, b = window or (0, n_r)
    got = occupancy_reference(rows, cols, vals, row_w[rows], col_w[cols], n_c, km, kn, a, b)
    want = occupancy_brute(_dense_ok(n_r, n_c, rows, cols, vals, row_w, col_w), km, kn, a, b)
    assert np.array_equal(got, want)
    if density == 0.0:
        assert got.size == 0


def test_occupancy_halo_pixel_reaches_the_window():
    """A single pixel just above a row window (within the template's half-height) lists the window's first tile row."""
    n_r, n_c = 300, 200
    got = occupancy_reference([99], [130], [1.0], [1.0], [1.0], n_c, 17, 17, 100, 228)
    assert np.array_equal(got, [1, 2])       # output rows 100 .. 107 reach row 99; columns 122 .. 138: tile columns 1 and 2
    assert occupancy_reference([91], [130], [1.0], [1.0], [1.0], n_c, 17, 17, 100, 228).size == 0
    assert np.array_equal(got, occupancy_brute(_dense_ok(n_r, n_c, np.array([99]), np.array([130]), np.array([1.0]),
                                                         np.ones(n_r), np.ones(n_c)), 17, 17, 100, 228))


@pytest.mark.parametrize("n_r,n_c,budget,halo", [
    (1000, 500, 100 * 512 * 8, 8),
    (1000, 500, 10 ** 12, 8),
    (24_900, 24_200, 1 << 30, 8),
    (57, 3000, 3000 * 8 * 20, 8),
    (12_000, 200_000, 8 << 30, 16),
    (249_000, 242_000, 1 << 40, 8),           # budget above 2^31 elements: the element cap cuts
])
def test_strip_plan(n_r, n_c, budget, halo):
    strips = pipeline.plan_inter_strips(n_r, n_c, budget, halo)
    owned = np.zeros(n_r, dtype=np.int64)
    ld = (n_c + 15) // 16 * 16
    for a, b in strips:
        assert 0 <= a < b <= n_r
        owned[a:b] += 1
        ra, rb = max(0, a - halo), min(n_r, b + halo)
        assert (rb - ra) * ld * 8 <= budget
        assert (rb - ra) * ld < 2 ** 31
    assert (owned == 1).all()
    assert strips[0][0] == 0 and strips[-1][1] == n_r
    sizes = [b - a for a, b in strips]
    assert max(sizes) - min(sizes) <= max(sizes) // 2 + 1


def test_strip_plan_rejects_bad_budgets():
    for bad in (0, -1, -1e9):
        with pytest.raises(ValueError):
            pipeline.plan_inter_strips(100, 100, bad, 8)
        with pytest.raises(ValueError):
            pipeline._check_budget(bad)
    with pytest.raises(ValueError):
        pipeline.plan_inter_strips(1000, 1000, 1008 * 8 * 10, 8)        # 10 rows cannot hold 1 + 2 x 8
    assert pipeline._check_budget(None) == pipeline.INTER_BUDGET_DEFAULT


def test_detect_and_quantify_take_inter_budget():
    import inspect
    assert "inter_budget" in inspect.signature(pipeline.detect).parameters
    assert "inter_budget" in inspect.signature(pipeline.quantify).parameters
    with pytest.raises(ValueError):
        pipeline.detect({}, {}, inter=True, inter_budget=0)


def test_new_entries_in_header_and_binding():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "chromosight_hip.h").read_text(), flags=re.S)
    for name in ("cs_csr_tile_occupancy", "cs_candidates_tiles"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _lib.ABI_SYMBOLS
    proto = re.search(r"int cs_candidates_tiles\s*\(([^;]*)\)", text).group(1)
    assert "const int32_t* d_tiles, int32_t n_tiles" in proto
    lib = _lib.load_library()
    assert hasattr(lib, "cs_csr_tile_occupancy") and hasattr(lib, "cs_candidates_tiles")


def test_strip_reach_covers_non_square_offsets():
    assert pipeline._strip_reach([np.zeros((17, 17))]) == 17
    assert pipeline._strip_reach([np.zeros((7, 17))]) == 2 * (3 + 5) + 1
    assert pipeline._strip_reach([np.zeros((21, 5)), np.zeros((9, 9))]) == 2 * (10 + 8) + 1
