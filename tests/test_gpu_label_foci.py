"""The three hand-written forms of the device focus labelling, each given candidate lists of known shape through
cs_label_foci_route and held to the plain reference of tests/label_util.py (scipy.ndimage.label, 4-neighbourhood):

  route 0  the kernel chain (link / flatten / stats / argbest / flag / emit): what cs_label_foci runs, any n
  route 1  foci_small_body, one workgroup on global arrays, after the same device sort: n <= 65 536
  route 2  foci_small_lds_body, one workgroup with its arrays in LDS, on the sorted list: n <= 8192, ms * ns <= 2^32 - 1
  route 3  the same on the list as given (sorted in LDS by lds_sort_pairs)

Every case runs on every route that takes its size; rows, columns and sizes of the foci must EQUAL the reference's, in order.

Contract of a list: distinct in-range pixels with finite nonzero float64 values, in any order (the lists are shuffled with a seed;
route 2 gets them sorted).  Duplicate pixels and values of +-0 or NaN are outside the contract: the callers concatenate disjoint
row windows of candidates that passed the threshold (value >= pearson and != 0).
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

from chromosight_amd import engine
from chromosight_amd._lib import get_device
from tests import label_util as lu

pytestmark = pytest.mark.gpu

ALL, GLOBAL, CHAIN = (0, 1, 2, 3), (0, 1), (0,)
LIMIT = {0: None, 1: 65536, 2: 8192, 3: 8192}          # kSmallMax, kSmallLds


def _normal(n, seed):
    v = np.random.default_rng(seed).normal(size=n)
    v[v == 0.0] = 1.0
    return v


# ---- shapes for the ties-and-signs cases: two blobs, values by rule -------------------------------------------------------------
def _two_blobs():
    mask = np.zeros((9, 19), dtype=bool)
    mask[1:7, 2:9] = True                                  # a 6 x 7 rectangle
    mask[2:8, 12] = True                                   # a cross, several rows high
    mask[4, 10:17] = True
    return lu._from_mask(mask)


def _plateau_vals(shape, rows, cols):
    """2.0 on a plateau that spans several rows of each blob, its first row-major pixel NOT its first column; 1.0 elsewhere."""
    v = np.ones(rows.size)
    for r, c in ((3, 7), (4, 3), (5, 2), (6, 8),           # rectangle: (3, 7) wins
                 (4, 15), (5, 12), (7, 12)):               # cross: (4, 15) wins
        v[(rows == r) & (cols == c)] = 2.0
    return v


def _extreme_vals(shape, rows, cols):
    return np.random.default_rng(7).choice([1e-300, -1e-300, 1e300, -1e300], size=rows.size)


def _sized(min_size):
    """Bars and bent pieces of min_size - 1, min_size and min_size + 1 pixels, one per 9 x 9 cell of the matrix."""
    pieces = []
    for k in (min_size - 1, min_size, min_size + 1):
        if k < 1:
            continue
        pieces.append([(0, x) for x in range(k)])                          # horizontal bar
        pieces.append([(y, 0) for y in range(k)])                          # vertical bar
        a = (k + 1) // 2
        pieces.append([(0, x) for x in range(a)] + [(y, a - 1) for y in range(1, k - a + 1)])   # bent
    px = []
    for i, piece in enumerate(pieces):
        oy, ox = 9 * (i // 3) + 1, 9 * (i % 3) + 2
        px += [(oy + y, ox + x) for y, x in piece]
    px = sorted(set(px))
    shape = (9 * ((len(pieces) + 2) // 3) + 1, 30)
    return shape, np.array([p[0] for p in px], dtype=np.int64), np.array([p[1] for p in px], dtype=np.int64)


def _wrap_pairs():
    """(r, ns - 1) and (r + 1, 0): consecutive keys that are no neighbours, on several rows, beside true neighbours."""
    px = [(0, 6), (1, 0), (2, 5), (2, 6), (3, 0), (3, 1), (5, 6), (6, 0), (6, 6), (7, 6), (8, 0)]
    return (9, 7), np.array([p[0] for p in px], dtype=np.int64), np.array([p[1] for p in px], dtype=np.int64)


def _one_column():
    rows = np.array([0, 1, 2, 4, 6, 7, 9, 20, 21, 22, 23, 49], dtype=np.int64)      # ns = 1: the lower neighbour has key + 1
    return (50, 1), rows, np.zeros_like(rows)


def _one_row():
    cols = np.array([0, 1, 2, 4, 6, 7, 9, 20, 21, 22, 23, 49], dtype=np.int64)
    return (1, 50), np.zeros_like(cols), cols


def _pixels(shape, *px):
    return shape, np.array([p[0] for p in px], dtype=np.int64), np.array([p[1] for p in px], dtype=np.int64)


# name -> (builder of (shape, rows, cols), value rule or None (seeded normal), min_size, diag_only, routes)
CASES = {}


def _add(name, build, routes=ALL, vals=None, min_size=2, diag_only=0):
    assert name not in CASES
    CASES[name] = (build, vals, min_size, diag_only, routes)


# shapes that break a union-find, at about 8190 pixels (all routes); snake and comb also at ~65 500 and ~70 000
_add("solid_8190", lambda: lu.solid(90, 91))
_add("snake_8189", lambda: lu.snake(129, 125))
_add("comb_8191", lambda: lu.comb(63, 255))
_add("spiral_8191", lambda: lu.spiral(127))
_add("column_8190", lambda: lu.column(8190))
_add("row_8190", lambda: lu.row(8190))
_add("checkerboard_8192_min1", lambda: lu.checkerboard(128, 128), min_size=1)
_add("checkerboard_8192_min2", lambda: lu.checkerboard(128, 128), min_size=2)
_add("diagonal_touch_8192", lambda: lu.diagonal_touch(64))
_add("snake_65521", lambda: lu.snake(361, 361), GLOBAL)
_add("comb_65535", lambda: lu.comb(255, 511), GLOBAL)
_add("snake_69937", lambda: lu.snake(373, 373), CHAIN)
_add("comb_70223", lambda: lu.comb(263, 531), CHAIN)
# adjacency edges
_add("wrap_pairs", _wrap_pairs, min_size=1)
_add("wrap_pairs_min2", _wrap_pairs, min_size=2)
_add("one_column", _one_column, min_size=1)
_add("one_row", _one_row, min_size=1)
_add("n0", lambda: _pixels((5, 5)), min_size=1)
_add("n1", lambda: _pixels((5, 5), (4, 4)), min_size=1)
_add("n1_min2", lambda: _pixels((5, 5), (0, 0)), min_size=2)
_add("n2_joined", lambda: _pixels((5, 5), (2, 4), (3, 4)), min_size=2)
_add("n2_apart", lambda: _pixels((5, 5), (2, 4), (3, 0)), min_size=1)
# sizes around min_size, with the row rule of the 1-D patterns
for _m in (1, 2, 5):
    for _d in (0, 1, 3):
        _add(f"sized_min{_m}_diag{_d}", functools.partial(_sized, _m), min_size=_m, diag_only=_d)
# ties and signs
_add("plateau", _two_blobs, vals=_plateau_vals)
_add("max_last", _two_blobs, vals=lambda s, r, c: np.arange(1.0, r.size + 1))
_add("all_equal", _two_blobs, vals=lambda s, r, c: np.full(r.size, 1.5))
_add("all_negative", _two_blobs, vals=lambda s, r, c: -0.1 - np.random.default_rng(3).random(r.size))
_add("all_negative_equal", _two_blobs, vals=lambda s, r, c: np.full(r.size, -2.0))
_add("mixed_signs", _two_blobs, vals=lambda s, r, c: _normal(r.size, 4))
_add("extremes_1e300", _two_blobs, vals=_extreme_vals)
# list lengths at the forms' limits (30 % of a square matrix); 2400 and 4097: no powers of two for the unpadded bitonic network
for _n, _routes in ((1023, ALL), (1024, ALL), (1025, ALL), (2400, ALL), (4097, ALL), (8191, ALL), (8192, ALL), (8193, GLOBAL),
                    (65535, GLOBAL), (65536, GLOBAL), (65537, CHAIN)):
    _add(f"random_{_n}", functools.partial(lu.random_pixels, _n, 0.3, _n), _routes)
# key widths: ms * ns = 2^16 - 1, 2^16, 2^16 + 1 (a prime: one column, one row), 2^24 - 1, 2^24 + 1, 2^32 - 1, 2^32
for _ms, _ns, _routes in ((255, 257, ALL), (256, 256, ALL), (65537, 1, ALL), (1, 65537, ALL), (4095, 4097, ALL), (24929, 673, ALL),
                          (65535, 65537, ALL), (65536, 65536, GLOBAL)):
    _add(f"corner_{_ms}x{_ns}", functools.partial(lu.corner_l, _ms, _ns), _routes, min_size=1)
_add("random_16671", functools.partial(lu.random_pixels, 16671, 0.3, 16671), GLOBAL)      # (the length of the split on record)

PAIRS = [(name, route) for name, spec in CASES.items() for route in spec[4]]


class Case:
    def __init__(self, name):
        build, vals, self.min_size, self.diag_only, self.routes = CASES[name]
        self.name = name
        self.shape, rows, cols = build()
        v = _normal(rows.size, 11) if vals is None else np.asarray(vals(self.shape, rows, cols), dtype=np.float64)
        assert np.isfinite(v).all() and (v != 0).all()
        perm = np.random.default_rng(rows.size + 1).permutation(rows.size)
        self.sorted = (rows, cols, v)
        self.shuffled = (rows[perm], cols[perm], v[perm])
        self.ref = lu.label_reference(self.shape, *self.shuffled, min_size=self.min_size, diag_only=self.diag_only)
        for a in self.sorted + self.shuffled + self.ref:
            a.setflags(write=False)
        self.n = rows.size

    def takes(self, route):
        return (LIMIT[route] is None or self.n <= LIMIT[route]) and (route < 2 or self.shape[0] * self.shape[1] <= 2**32 - 1)

    def label(self, dev, route, cap=None):
        rows, cols, vals = self.sorted if route == 2 else self.shuffled
        return engine.run_label_foci(dev, self.shape, rows, cols, vals, min_size=self.min_size, diag_only=self.diag_only,
                                     route=route, cap=cap)

    def check(self, got, what=""):
        for g, w, field in zip(got, self.ref, ("rows", "cols", "sizes")):
            assert g.shape == w.shape and np.array_equal(g, w), (
                f"{self.name}{what}: {field} differ from the reference ({g.size} foci, reference {w.size})")


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@pytest.mark.parametrize("name,route", PAIRS)
def test_route_equals_reference(name, route):
    c = case(name)
    assert c.takes(route)
    got = c.label(get_device(), route)
    print(f"{name} route {route}: {c.n} pixels, {got[0].size} foci")
    c.check(got, f" route {route}")
    if name == "checkerboard_8192_min1":
        assert got[0].size == c.n                          # every pixel a focus: n_foci == cap
    if name == "checkerboard_8192_min2":
        assert got[0].size == 0


def test_every_route_ran_every_case_it_takes():
    """The table above leaves a route out only where the form refuses the list."""
    for name, spec in CASES.items():
        c = case(name)
        assert tuple(r for r in ALL if c.takes(r)) == spec[4], name


@pytest.mark.parametrize("name,route", [("random_8193", 2), ("random_8193", 3), ("random_65537", 1), ("random_65537", 2),
                                        ("corner_65536x65536", 2), ("corner_65536x65536", 3)])
def test_lists_a_form_does_not_take_are_refused(name, route):
    c = case(name)
    assert not c.takes(route)
    with pytest.raises(NotImplementedError):               # CS_ERR_UNSUPPORTED
        c.label(get_device(), route)


def test_unknown_routes_and_zero_values_are_invalid():
    dev = get_device()
    c = case("wrap_pairs")
    for route in (-1, 4, 7):
        with pytest.raises(ValueError):                    # CS_ERR_INVALID
            c.label(dev, route)
    rows, cols, vals = c.shuffled
    for zero in (0.0, -0.0):
        v = vals.copy()
        v[3] = zero
        for route in (1, 2, 3):                            # the one-workgroup forms would drop the pixel
            with pytest.raises(ValueError):
                engine.run_label_foci(dev, c.shape, rows, cols, v, min_size=1, route=route)
    # an empty list is answered by every known route, and the route is still checked
    assert all(engine.run_label_foci(dev, (5, 5), [], [], [], min_size=1, route=r)[0].size == 0 for r in ALL)
    with pytest.raises(ValueError):
        engine.run_label_foci(dev, (5, 5), [], [], [], min_size=1, route=4)


@pytest.mark.parametrize("route", ALL)
def test_output_room(route):
    """A cap below the number of foci: CS_ERR_OVERFLOW with *n_foci set; the exact cap passes."""
    dev = get_device()
    shape, rows, cols = lu.checkerboard(10, 10)
    r32, c32 = rows.astype(np.int32), cols.astype(np.int32)
    vals = _normal(rows.size, 5)
    for cap, want_rc in ((49, -4), (0, -4), (50, 0)):
        out = [np.full(max(cap, 1), -7, np.int32) for _ in range(3)]
        n = C.c_int64(-1)
        rc = dev.lib.cs_label_foci_route(dev.ctx, None, shape[0], shape[1], r32.ctypes.data, c32.ctypes.data, vals.ctypes.data,
                                         rows.size, 1, 0, route, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, cap,
                                         C.byref(n))
        assert (rc, n.value) == (want_rc, 50), (cap, rc, n.value)
        if rc == 0:
            assert np.array_equal(out[0], rows) and np.array_equal(out[1], cols) and (out[2] == 1).all()
        else:
            assert all((o == -7).all() for o in out)       # nothing written


# ---- repeats: a concurrent algorithm gives ONE answer ---------------------------------------------------------------------------
# Ordinary runs of correct inputs, 100 each.  On an MI355X 100 labellings of a case take 0.02 - 0.2 s (printed per case), far
# below the 3 s at which a count would have to come down.  A green run does not show that a race is absent, only that it is rare;
# before the one-workgroup forms flattened with the read-only uf_root, the snake failed 72 / 55 / 38 of 100 on routes 1 / 2 / 3.
REPEATS = 100
REPEAT_CASES = [(name, route) for name in ("snake_8189", "comb_8191", "solid_8190", "random_8191", "random_16671")
                for route in CASES[name][4]]


@pytest.mark.parametrize("name,route", REPEAT_CASES)
def test_repeated_labelling_gives_one_answer(name, route):
    dev = get_device()
    c = case(name)
    bad = 0
    t0 = time.perf_counter()
    for k in range(REPEATS):
        got = c.label(dev, route)
        bad += not all(np.array_equal(g, w) for g, w in zip(got, c.ref))
    seconds = time.perf_counter() - t0
    print(f"{name} route {route}: {c.n} pixels, {c.ref[0].size} foci, {REPEATS} labellings in {seconds:.3f} s, {bad} differ")
    assert bad == 0, f"{name} route {route}: {bad} of {REPEATS} labellings differ from the reference"
