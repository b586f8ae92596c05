"""The 8-wave dense instance after its per-tile work was trimmed (chromosight_amd/csrc/cs_corr_mfma_dense8.inc): the tile walk
carried without divisions, staging without lane masks, the wave maximum on bit patterns.  None of it may change a value:
on maps whose tile sequences exercise the carried state, the 8-wave result equals the 4-wave instance's
(CHROMOSIGHT_HIP_MFMA_WAVES4=1), which still derives every tile's origin with a division, bit for bit.

Grids are min(tiles, 2 x CUs) = 512 workgroups on a 256-CU part:
  (3072, 2048)  48 x 32 tiles, three per workgroup; tiles_x = 32 divides the XCD step of 64, so dense_tile_skew picks 1 and the
                carried column wraps twice per workgroup
  (2240, 1024)  35 x 16 tiles, skew 1; the XCD ranges of 70 tiles begin in mid-row, the second tile of a workgroup is 4 rows down
  (2112, 1032)  33 x 17 tiles, skew 0, the last tile column 8 pixels wide: rim tiles in every tile row
  (200, 264)    the row window (37, 165): 2 x 5 = 10 tiles, row_begin != 0, every tile on the rim (clamped transfers, masked
                values); grid = 10, not a multiple of 8, one tile per workgroup
On a 256-CU part a grid that is not a multiple of 8 has fewer than 512 tiles and therefore one tile per workgroup, so the
steps of that branch of the walk are covered by the host test only (tests/test_dense8_walk_host.py)."""
import numpy as np
import pytest

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd import engine
from chromosight_amd._lib import LAYOUT_DENSE, CsMatrix, get_device, np_dtype_code

pytestmark = pytest.mark.gpu

KERNEL_MFMA_DENSE = 4
SWITCH = "CHROMOSIGHT_HIP_MFMA_WAVES4"


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


def served_by(waves):
    dev = get_device()
    assert dev.lib.cs_last_kernel(dev.ctx) == KERNEL_MFMA_DENSE
    assert dev.lib.cs_last_dense_waves(dev.ctx) == waves


def device_map(sig, window=None):
    """cs_normxcorr2 (full) on a device-resident float32 map into a float32 buffer; window = (a, b): the rows a .. b - 1 only,
    from a slab of the input rows they reach."""
    dev = get_device()
    n, cols = sig.shape
    kspec = engine.KernelSpec(np.asarray(ck.loops["kernels"][0], dtype=np.float64), None)
    code = np_dtype_code(np.float32)
    a, b = window or (0, n)
    ra, rb = (max(0, a - 8), min(n, b + 8)) if window else (0, n)
    d_sig = dev.to_device(np.ascontiguousarray(sig[ra:rb]))
    d_out = dev.zeros((b - a) * cols, np.float32)
    engine.run_normxcorr2(dev, CsMatrix(d_sig.ptr, code, LAYOUT_DENSE, cols, 0, 0, ra), (n, cols), kspec,
                          CsMatrix(d_out.ptr, code, LAYOUT_DENSE, cols, 0, 0, a), full=True, sym_upper=False,
                          max_dist=None, precision="f32", row_window=window)
    return d_out.download().reshape(b - a, cols)


@pytest.mark.parametrize("shape,window", [((3072, 2048), None), ((2240, 1024), None), ((2112, 1032), None), ((200, 264), (37, 165))])
def test_trimmed_walk_is_bit_identical_to_the_4_wave_instance(shape, window, monkeypatch):
    rng = np.random.default_rng(shape[0] + shape[1])
    sig = rng.gamma(4.0, 0.25, size=shape).astype(np.float32)
    dv8 = device_map(sig, window)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    dv4 = device_map(sig, window)
    served_by(4)
    assert dv8.shape == ((window[1] - window[0]) if window else shape[0], shape[1])
    assert np.abs(dv4).max() > 0.01 and np.isfinite(dv4).all()
    assert np.array_equal(dv8, dv4)
