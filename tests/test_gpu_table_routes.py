"""Every route to a resident pixel table ends in DeviceCool._set_table, so every route to the SAME table leaves the same object:
the constructor over a path, from_cool_file, from_pairs + set_weights, merged() of one table and coarsened(1), on the example .cool.
Attribute sets are compared as they are right after construction; counts and weights are compared bit for bit."""
import numpy as np
import pytest

from chromosight_amd import io as cio
from chromosight_amd import pipeline
from tests import cload_util as cu
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

EXAMPLE = GOLDEN / "example.cool"


@pytest.fixture(scope="module")
def routes():
    """name -> (DeviceCool, the names of its attributes right after construction)."""
    cool = cio.load_cool(str(EXAMPLE))
    first = pipeline.DeviceCool(str(EXAMPLE))
    made = {"constructor": first, "from_cool_file": pipeline.DeviceCool.from_cool_file(str(EXAMPLE)),
            "from_pairs": pipeline.DeviceCool.from_pairs(cu.pairs_of_table(cool, seed=1), cu.chromsizes_of(cool), int(cool["binsize"])),
            "merged": first.merged(), "coarsened": first.coarsened(1)}
    names = {route: set(vars(dcool)) for route, dcool in made.items()}
    made["from_pairs"].set_weights(cool["weight"])
    return {route: (dcool, names[route]) for route, dcool in made.items()}


def _same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _table(dcool):
    n = dcool.nnz                                   # (a coarsened table's buffers have room for more, in 8-byte slots)
    return dcool.indptr.download(), dcool.indices.download()[:n], dcool.data.download().view(dcool.val_dtype)[:n]


ROUTES = ["from_cool_file", "from_pairs", "merged", "coarsened"]


@pytest.mark.parametrize("route", ROUTES)
def test_every_route_leaves_the_same_object(routes, route):
    want, want_names = routes["constructor"]
    got, got_names = routes[route]
    assert got_names == want_names
    assert set(vars(got)) == set(vars(want))                    # ... and still, with weights set and tables downloaded
    # the geometry
    assert got.names == want.names and got.binsize == want.binsize and got.n_bins == want.n_bins
    assert _same_bytes(got.offsets, want.offsets)
    assert _same_bytes(got.bin_start, want.bin_start) and _same_bytes(got.bin_end, want.bin_end)
    # the table
    assert got.nnz == want.nnz > 0 and got.val_dtype is want.val_dtype and got._counts_exact is want._counts_exact is True
    assert got.upper is want.upper is True and got.counts_ok is want.counts_ok is True
    assert got.upload_bytes == want.upload_bytes
    for a, b in zip(_table(got), _table(want)):
        assert _same_bytes(a, b)
    # the weights
    for name in ("weight", "miss", "det"):
        assert _same_bytes(getattr(got, name).download(), getattr(want, name).download()), name
    assert _same_bytes(got.miss_host, want.miss_host) and _same_bytes(got.host_weight, want.host_weight)
    assert want.dropped is None and got.dropped == (0 if route == "from_pairs" else None)


def test_no_chunks_leave_a_valid_empty_table(routes):
    sizes = (("x", 7000), ("y", 1), ("z", 11500))               # a chromosome of one bin, and one with a short last bin
    empty = pipeline.DeviceCool.from_pairs(iter(()), sizes, 1000)
    assert set(vars(empty)) == routes["constructor"][1]
    assert empty.names == ["x", "y", "z"] and empty.offsets.tolist() == [0, 7, 8, 20] and empty.n_bins == 20 and empty.binsize == 1000
    assert empty.bin_start.tolist() == [*range(0, 7000, 1000), 0, *range(0, 12000, 1000)]
    assert empty.bin_end.tolist() == [*range(1000, 8000, 1000), 1, *range(1000, 12000, 1000), 11500]
    assert empty.nnz == 0 and empty.val_dtype is np.float32 and empty.upper is True and empty.dropped == 0
    assert not empty.has_weights and empty.host_weight is None and empty.counts_ok is False
    assert _same_bytes(empty.indptr.download(), np.zeros(21, dtype=np.int64))
    for key in ("bin1_id", "bin2_id", "count"):
        assert _same_bytes(empty.host[key], np.zeros(0, dtype=np.int64)), key
    assert empty.host["weight"] is None
    # it is a table like any other: merged with one that has pixels it gives that table, and it takes weights
    c, p = np.asarray([0, 2], dtype=np.int32), np.asarray([1, 11500], dtype=np.int64)
    some = pipeline.DeviceCool.from_pairs((c, p, c, p), sizes, 1000)
    both = empty.merged(some)
    assert both.nnz == some.nnz == 2 and all(_same_bytes(a, b) for a, b in zip(_table(both), _table(some)))
    assert both.host["bin1_id"].tolist() == both.host["bin2_id"].tolist() == [0, 19]
    empty.set_weights(np.ones(20))
    assert empty.has_weights and empty.counts_ok is True
