"""The staging geometry has one owner and it is right (no GPU): pipeline.intra_geometry against the independent statement
of tests/staging_cases.geometry, the trans pitch pipeline._inter_ld against what plan_inter_strips budgets with, and a
StagedBlock that declares its fields and refuses any other."""
import itertools

import pytest

import staging_cases as sc
from chromosight_amd import pipeline

MAX_DISTS = (0, 1, 20, 63, 200, 447, 512, 10 ** 6)
LARGEST = (3, 17, 81)


def test_intra_geometry_equals_the_independent_statement():
    cases = list(itertools.product(range(1, 601), MAX_DISTS, LARGEST)) + [(2000, 447, 17)]
    bumped_band = bumped_dense = 0
    for n, max_dist, largest in cases:
        geo = pipeline.intra_geometry(n, max_dist, largest)
        keep, band, band_w, ld = sc.geometry(max_dist, n, largest)
        where = (n, max_dist, largest)
        assert geo.keep == keep and geo.band == band and geo.ld == ld, where
        assert (geo.in_w if geo.band else 0) == band_w, where
        assert geo.n_diags == min(n, geo.keep + 1), where
        assert geo.out_w == min(max_dist, n - 1) + 1 and geo.in_w == min(geo.keep, n - 1) + 1, where
        # the pitch bump: 512 float64 are 4 KiB, so the pitch moves one quantum on
        if geo.band and 449 <= geo.in_w <= 512:
            assert geo.ld == 576, where
            bumped_band += 1
        if not geo.band and 497 <= n <= 512:
            assert geo.ld == 528, where
            bumped_dense += 1
    assert bumped_band >= 1 and bumped_dense >= 1, (bumped_band, bumped_dense)
    assert pipeline.intra_geometry(600, 447, 17)[2:5] == (465, 448, False)        # (1200 > 600: that one is dense)
    with pytest.raises(AttributeError):
        pipeline.intra_geometry(600, 447, 17).keep = 0                           # immutable


@pytest.mark.parametrize("n_c", [1, 15, 16, 17, 260])
def test_strips_are_budgeted_by_the_trans_pitch(n_c):
    ld = pipeline._inter_ld(n_c)
    assert ld % 16 == 0 and 0 <= ld - n_c < 16
    n_r = 1000
    for k in (1, 2, 7, 64, 999, 1000, 1001):
        strips = pipeline.plan_inter_strips(n_r, n_c, k * ld * 8, 0)
        assert max(b - a for a, b in strips) <= k, (n_c, k)
        assert strips[0][0] == 0 and strips[-1][1] == n_r and all(p[1] == q[0] for p, q in zip(strips, strips[1:]))
        # one byte less holds one row less: the budget is counted in rows of exactly this pitch
        if k > 1:
            assert max(b - a for a, b in pipeline.plan_inter_strips(n_r, n_c, k * ld * 8 - 1, 0)) <= k - 1, (n_c, k)


DECLARED = {"buffer32": None, "shared": None, "d_law": None, "n_diags": None, "smooth": False, "genome": None, "parent": None,
            "view": None, "view_row0": None, "strip_pool": None, "row_window": None, "sig32": None, "restage": None, "buffer": None,
            "pool": None}


def test_a_staged_block_declares_its_fields_and_refuses_others():
    block = pipeline.StagedBlock("c0", object(), (5, 5), None, None, 3, False, 20)
    for field, default in DECLARED.items():
        assert getattr(block, field) is default, field
    assert (block.name, block.shape, block.max_dist, block.inter, block.keep) == ("c0", (5, 5), 3, False, 20)
    with pytest.raises(AttributeError):
        block.row_windw = (0, 1)
    assert not hasattr(block, "__dict__")
    for field in DECLARED:                                  # every declared field can be set
        setattr(block, field, getattr(block, field))
