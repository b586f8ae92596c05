"""tests/label_util.label_reference -- the plain reference the device labelling is held to (tests/test_gpu_label_foci.py) -- pinned
to oracle/foci_oracle.pick_foci_dense, itself pinned to the reference's own pick_foci on tests/golden/nms.npz.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import foci_oracle
from tests import label_util as lu


def _list_of(conv, pearson):
    rows, cols = np.nonzero((conv >= pearson) & (conv != 0))
    return rows, cols, conv[rows, cols]


def test_reference_matches_the_oracle_on_the_golden_maps(golden):
    g = golden("nms")
    tags = sorted({k[:-len("_pearson")] for k in g if k.endswith("_pearson")})
    assert len(tags) == 15
    seen = 0
    for tag in tags:
        conv = sp.coo_matrix((g[f"{tag}_conv_val"], (g[f"{tag}_conv_row"], g[f"{tag}_conv_col"])),
                             shape=tuple(g[f"{tag}_conv_shape"])).toarray()
        pearson = float(g[f"{tag}_pearson"])
        rows, cols, vals = _list_of(conv, pearson)
        fr, fc, fs = lu.label_reference(conv.shape, rows, cols, vals, min_size=2)
        want = g[f"{tag}_foci"].reshape(-1, 2)
        assert np.array_equal(np.column_stack([fr, fc]).reshape(-1, 2), want), tag
        assert np.array_equal(want, foci_oracle.pick_foci_dense(conv, pearson)), tag
        assert (fs >= 2).all()
        seen += len(fr)
    assert seen > 0


@pytest.mark.parametrize("seed,shape,density,min_size", [(0, (40, 60), 0.3, 2), (1, (64, 64), 0.5, 1), (2, (33, 7), 0.6, 3),
                                                         (3, (1, 90), 0.5, 2), (4, (90, 1), 0.5, 2), (5, (50, 50), 0.9, 5)])
def test_reference_matches_the_oracle_on_random_maps(seed, shape, density, min_size):
    """Values from a handful of levels, so maxima tie; the list is shuffled (the reference takes any order) and sits at a row
    offset in a taller matrix (only the bounding rows are held densely)."""
    rng = np.random.default_rng(seed)
    conv = np.where(rng.random(shape) < density, rng.choice([-2.0, -0.5, 0.25, 1.0, 3.0], size=shape), 0.0)
    want = foci_oracle.pick_foci_dense(conv, -np.inf, min_size=min_size)
    rows, cols, vals = _list_of(conv, -np.inf)
    perm = rng.permutation(rows.size)
    fr, fc, fs = lu.label_reference(shape, rows[perm], cols[perm], vals[perm], min_size=min_size)
    assert np.array_equal(np.column_stack([fr, fc]).reshape(-1, 2), want)
    labels, _ = foci_oracle.ndi.label(conv != 0, structure=foci_oracle.FOUR)
    assert np.array_equal(fs, np.bincount(labels.ravel())[labels[fr, fc]])
    off = 1000
    fr2, fc2, fs2 = lu.label_reference((shape[0] + 2 * off, shape[1]), rows[perm] + off, cols[perm], vals[perm], min_size=min_size)
    assert np.array_equal(fr2, fr + off) and np.array_equal(fc2, fc) and np.array_equal(fs2, fs)
    for d in (1, 3):
        dr, dc, ds = lu.label_reference(shape, rows, cols, vals, min_size=min_size, diag_only=d)
        assert np.array_equal(dr, fc + (d >> 1)) and np.array_equal(dc, fc) and np.array_equal(ds, fs)


def test_generators_give_distinct_row_major_lists():
    for shape, rows, cols in (lu.solid(5, 7), lu.snake(9, 6), lu.comb(6, 9), lu.spiral(11), lu.column(9), lu.row(9),
                              lu.checkerboard(5, 4), lu.diagonal_touch(3), lu.random_pixels(100, 0.3, 0), lu.corner_l(300, 7),
                              lu.corner_l(65537, 1), lu.corner_l(65536, 65536)):
        keys = rows * shape[1] + cols
        assert (np.diff(keys) > 0).all() and rows.max() < shape[0] and cols.max() < shape[1]
    one = np.ones(8192)
    assert [len(lu.label_reference(s, r, c, one[:len(r)], 1)[0]) for s, r, c in
            (lu.snake(129, 125), lu.comb(63, 255), lu.spiral(127), lu.checkerboard(128, 128), lu.diagonal_touch(64))] == [1, 1, 1, 8192, 2]
    # the corner L and its wrap pair: one focus of 8 pixels, two single pixels that do NOT join
    s, r, c = lu.corner_l(65535, 65537)
    fr, fc, fs = lu.label_reference(s, r, c, np.arange(1.0, len(r) + 1), 1)
    assert fs.tolist() == [1, 1, 8] and (fr[-1], fc[-1]) == (65534, 65536)
