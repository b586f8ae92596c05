"""The compile-time instances of the 8-wave dense 17 x 17 tile kernel (chromosight_amd/csrc/cs_corr_mfma_dense8.inc) and the
addressing of its inner tiles.

The kernel is a template over what a launch fixes -- coefficient or plain cross-correlation, float32 or float64 output --
and an inner tile (every staged pixel exists; every output pixel is stored) fetches and stores through a buffer descriptor:
a uniform base per tile plus 32-bit lane offsets formed once.  Rim tiles keep the clamped transfers and the per-pixel
stores.  Per pixel nothing changed, so every instance must agree bit for bit with the 4-wave instance
(CHROMOSIGHT_HIP_MFMA_WAVES4=1), which has neither, and stay within the suite's tolerance of the oracle.

192 x 192 is the smallest map with an inner tile: 3 x 3 tiles, the centre one alone takes the unclamped fetch and the plain
store.  260 x 328 (5 x 6 tiles, columns a multiple of 4, neither side a multiple of 64) has rim tiles on every edge."""
import ctypes as C

import numpy as np
import pytest

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd import engine
from chromosight_amd._lib import LAYOUT_DENSE, CsMatrix, get_device, np_dtype_code
from oracle import c_oracle
from oracle import pearson_oracle as orc
from parity_util import assert_parity

pytestmark = pytest.mark.gpu

KERNEL_MFMA_DENSE = 4
SWITCH = "CHROMOSIGHT_HIP_MFMA_WAVES4"
SHAPES = [(192, 192), (260, 328)]
THRESHOLD = 1e-4


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


def loops():
    return np.asarray(ck.loops["kernels"][0], dtype=np.float64)


def served_by(waves):
    dev = get_device()
    assert dev.lib.cs_last_kernel(dev.ctx) == KERNEL_MFMA_DENSE
    assert dev.lib.cs_last_dense_waves(dev.ctx) == waves


def _signal(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    return rng.gamma(4.0, 0.25, size=shape).astype(np.float32)


def _slab(sig, window, pitch):
    """The input rows a row window reaches, at a row pitch, on the device: (buffer, CsMatrix)."""
    dev = get_device()
    n, cols = sig.shape
    a, b = window or (0, n)
    ra, rb = (max(0, a - 8), min(n, b + 8)) if window else (0, n)
    ld = pitch or cols
    host = np.full((rb - ra, ld), np.float32(7.5))          # (what lies between the rows is not zero)
    host[:, :cols] = sig[ra:rb]
    buf = dev.to_device(host)
    return buf, CsMatrix(buf.ptr, np_dtype_code(np.float32), LAYOUT_DENSE, ld, 0, 0, ra)


def coefficients(sig, *, full, out_dtype=np.float32, window=None, pitch=None, out_pitch=None):
    """cs_normxcorr2 on a device-resident float32 map into a device-resident map of `out_dtype`."""
    dev = get_device()
    n, cols = sig.shape
    a, b = window or (0, n)
    buf, d_sig = _slab(sig, window, pitch)
    ld_out = out_pitch or cols
    d_out = dev.zeros((b - a) * ld_out, out_dtype)
    engine.run_normxcorr2(dev, d_sig, (n, cols), engine.KernelSpec(loops(), None),
                          CsMatrix(d_out.ptr, np_dtype_code(out_dtype), LAYOUT_DENSE, ld_out, 0, 0, a), full=full,
                          sym_upper=False, max_dist=None, precision="f32", row_window=window)
    got = d_out.download().reshape(b - a, ld_out)
    assert np.all(got[:, cols:] == 0)                          # nothing is stored between the rows
    return got[:, :cols]


def cross_correlation(sig, out_dtype):
    """cs_xcorr2 on a device-resident float32 map into a device-resident map of `out_dtype`."""
    dev = get_device()
    n, cols = sig.shape
    buf, d_sig = _slab(sig, None, None)
    d_out = dev.zeros(n * cols, out_dtype)
    d_mat = CsMatrix(d_out.ptr, np_dtype_code(out_dtype), LAYOUT_DENSE, cols, 0, 0, 0)
    w = np.ascontiguousarray(loops())
    with dev.lock:
        dev._check(dev.lib.cs_xcorr2(dev.ctx, None, C.byref(d_sig), n, cols, w.ctypes.data_as(C.POINTER(C.c_double)), 17, 17,
                                     THRESHOLD, engine.compute_code("f32"), C.byref(d_mat)))
    return d_out.download().reshape(n, cols)


@pytest.fixture(scope="module")
def references():
    """Per shape: the signal, the oracle's coefficients for full = True / False and its cross-correlation.  Computed once."""
    ref = {}
    for shape in SHAPES:
        sig = _signal(shape)
        s64 = sig.astype(np.float64)
        ref[shape] = {"sig": sig, "xcorr": orc.xcorr2_oracle(s64, loops(), threshold=0)}
        for full in (True, False):
            ref[shape][full] = c_oracle.normxcorr2_rows(s64, loops(), 0, shape[0], full=full)
    return ref


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_coefficient_instances(references, shape, full, out_dtype, monkeypatch):
    sig = references[shape]["sig"]
    got8 = coefficients(sig, full=full, out_dtype=out_dtype)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    got4 = coefficients(sig, full=full, out_dtype=out_dtype)
    served_by(4)
    assert got8.dtype == out_dtype and np.abs(got4[64:128, 64:128]).max() > 0.01
    assert np.array_equal(got8, got4)
    want, cond = references[shape][full]
    assert_parity(got8, want, cond, "f32", f"dense8 {shape} full={full} {np.dtype(out_dtype).name} out")


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_correlation_instances(references, shape, out_dtype, monkeypatch):
    sig = references[shape]["sig"]
    got8 = cross_correlation(sig, out_dtype)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    got4 = cross_correlation(sig, out_dtype)
    served_by(4)
    assert got8.dtype == out_dtype and np.abs(got4[64:128, 64:128]).max() > 0.01
    assert np.array_equal(got8, got4)
    want = references[shape]["xcorr"]
    near = np.abs(np.abs(want) - THRESHOLD) < 1e-5
    ref = np.where(np.abs(want) < THRESHOLD, 0.0, want)
    assert np.abs(got8 - ref)[~near].max() < 3e-6 * np.abs(want).max()          # (the bound of tests/test_gpu_mfma_dense8.py)
    assert np.all(got8[:8] == 0) and np.all(got8[:, :8] == 0) and np.all(got8[-8:] == 0) and np.all(got8[:, -8:] == 0)


WINDOW = (70, 200)


def _one_scale_signal(references):
    """The 260 x 328 map with one tile scale.  A row window's tiles begin at its first row, the whole map's at row 0, and a tile
    is scaled by the power of two of its largest pixel: clipped below 3.9 and with 3.95 at every 16th row and column, the map's
    largest pixel is 3.95 in every tile wherever the tiles begin."""
    sig = np.minimum(references[(260, 328)]["sig"], np.float32(3.9))
    sig[::16, ::16] = np.float32(3.95)
    return sig


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
def test_row_pitch_and_window(references, out_dtype, monkeypatch):
    """Pitches larger than the width -- the input's no multiple of 4: rows at every 4-byte alignment -- and a row window that
    starts and ends inside a tile, from a slab of the rows it reaches: the first rows of input and output are not 0."""
    sig = _one_scale_signal(references)
    a, b = WINDOW
    whole = coefficients(sig, full=True, out_dtype=out_dtype, pitch=341, out_pitch=332)
    served_by(8)
    part8 = coefficients(sig, full=True, out_dtype=out_dtype, window=WINDOW, pitch=341, out_pitch=332)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    part4 = coefficients(sig, full=True, out_dtype=out_dtype, window=WINDOW, pitch=341, out_pitch=332)
    served_by(4)
    assert np.abs(part4).max() > 0.01
    assert np.array_equal(part8, part4)
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, sig.shape[0], full=True)
    assert_parity(whole, want, cond, "f32", f"dense8 pitched {np.dtype(out_dtype).name} out")
    assert_parity(part8, want[a:b], cond[a:b], "f32", f"dense8 pitched rows {a}:{b} {np.dtype(out_dtype).name} out")
    # against the same rows of the whole map: the bound of tests/test_gpu_mfma_dense8.py::test_row_windows.  On this map the two
    # are not equal bit for bit in any instance (see test_row_window_equals_the_rows_of_the_whole_map)
    assert np.abs(part8.astype(np.float64) - whole[a:b]).max() <= 2e-6


def _counts_signal():
    """A 260 x 328 map of contact counts 1 .. 15, with 15 at every 16th row and column.

    On such a map a pixel's coefficient does not depend on where the tiles begin, which it does on a map of arbitrary floats:
    a row window's tiles begin at its first row, so an output row lies at another row of its tile than in the whole-map call,
    and the vertical pass of the box sums contracts its 17 partial sums from other slots of the matrix instruction -- a float32
    sum whose last place depends on the slots (measured on a gamma-distributed map of one tile scale: 32 109 of the window's
    42 640 pixels differ from the whole map's by at most 2.1e-7, in the 4-wave instance and in the kernel before this file's
    instances exactly as now).  With counts every step is exact in every order.  The largest pixel of every tile is 15, so
    every tile is scaled by 2^3; the scaled pixels (multiples of 8 up to 120) and their scaled squares (2 x^2 <= 450) are
    float16 values with zero tails; a row's 17-sums (<= 2040 and <= 7650) are integers, so their float16 heads and tails are
    exact; and the vertical sums stay below 2^24, where float32 adds integers exactly.  The cross term is accumulated per
    pixel in the same order in any tile (template row by template row; the columns of a tile do not move with a row window),
    and no window is empty or constant, so every wave takes the lean form of the coefficient in both calls."""
    rng = np.random.default_rng(260328)
    sig = rng.integers(1, 15, size=(260, 328)).astype(np.float32)
    sig[::16, ::16] = np.float32(15.0)
    return sig


@pytest.mark.parametrize("out_dtype", [np.float32, np.float64])
def test_row_window_equals_the_rows_of_the_whole_map(out_dtype, monkeypatch):
    """The rows 70 .. 199 computed as a row window (input pitch 341, output pitch 332, a slab of the rows the window reaches:
    first rows of input and output not 0), bit for bit against the same rows of the whole-map call and against the 4-wave
    instance, on a map of counts (_counts_signal: the map on which that equality can hold at all).  A transfer or a store at a
    wrong base moves whole pixels and shows in either comparison."""
    sig = _counts_signal()
    a, b = WINDOW
    whole = coefficients(sig, full=True, out_dtype=out_dtype, pitch=341, out_pitch=332)
    served_by(8)
    part = coefficients(sig, full=True, out_dtype=out_dtype, window=WINDOW, pitch=341, out_pitch=332)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    part4 = coefficients(sig, full=True, out_dtype=out_dtype, window=WINDOW, pitch=341, out_pitch=332)
    served_by(4)
    diff = np.abs(part.astype(np.float64) - whole[a:b])
    print(f"row window {a}:{b} against the whole map, {np.dtype(out_dtype).name} out: {int((diff > 0).sum())} of {diff.size} pixels "
          f"differ, largest difference {diff.max():.3e}, largest coefficient {np.abs(whole[a:b]).max():.3f}")
    assert np.abs(part4).max() > 0.01
    assert np.array_equal(part, part4)
    assert np.array_equal(part, whole[a:b])
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, sig.shape[0], full=True)
    assert_parity(part, want[a:b], cond[a:b], "f32", f"dense8 counts rows {a}:{b} {np.dtype(out_dtype).name} out")


def test_candidate_range_keeps_the_literal_path(monkeypatch):
    """A call with cand_cmin > 0 (candidate mode: the literal form of the coefficient with the candidate screen) on the
    smallest map with an inner tile: the same candidates with the same float64 coefficients as through the 4-wave instance."""
    shape, pearson = (192, 192), 0.3
    sig = _signal(shape)
    kz = loops()
    for i0, j0 in ((40, 150), (96, 96), (100, 120), (170, 30)):              # patterns on the rim and in the inner tile
        sig[i0 - 8:i0 + 9, j0 - 8:j0 + 9] += (3.0 * (kz - kz.min())).astype(np.float32)
    dev = get_device()

    def candidates():
        buf, d_sig = _slab(sig, None, None)
        return engine.run_candidates(dev, d_sig, shape, engine.KernelSpec(kz), (0, shape[0]), pearson=pearson,
                                     lo_diag=-(shape[0] - 1), hi_diag=shape[1] - 1, inter=True, full=True, sym_upper=False,
                                     max_dist=-1)
    rows8, cols8, vals8 = candidates()
    monkeypatch.setenv(SWITCH, "1")
    rows4, cols4, vals4 = candidates()
    assert rows8.size >= 4 and np.any((rows8 >= 64) & (rows8 < 128) & (cols8 >= 64) & (cols8 < 128))
    assert np.array_equal(rows8, rows4) and np.array_equal(cols8, cols4) and np.array_equal(vals8, vals4)
    want, _ = c_oracle.normxcorr2_rows(sig.astype(np.float64), kz, 0, shape[0], full=True)
    assert np.abs(vals8 - want[rows8, cols8]).max() < 1e-7
