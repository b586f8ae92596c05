"""The 8-wave instance of the dense 17 x 17 tile kernel (chromosight_amd/csrc/cs_corr_mfma_dense8.inc).

Unmasked dense float32 maps with 16-byte tile transfers and the mirrored 17 x 17 loops template run the 64 x 64 tile with
eight waves (four per SIMD); CHROMOSIGHT_HIP_MFMA_WAVES4=1 keeps the 4-wave instance, which serves every other dense
call.  Both are kernel id 4; cs_last_dense_waves says which ran.  Every pixel sees the same operations in the same order
in both, so on data without near-threshold windows the maps are equal bit for bit; the one per-wave decision (lean or
literal form of the coefficient: a wave covers 16 x 32 pixels instead of 16 x 64) is held to the CPU oracle instead."""
import numpy as np
import pytest

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd import engine
from chromosight_amd._lib import LAYOUT_DENSE, CsMatrix, get_device, np_dtype_code
from chromosight_amd.utils import detection as cud
from oracle import c_oracle
from parity_util import assert_parity

pytestmark = pytest.mark.gpu

KERNEL_MFMA_DENSE = 4
SWITCH = "CHROMOSIGHT_HIP_MFMA_WAVES4"


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


def loops():
    return np.asarray(ck.loops["kernels"][0], dtype=np.float64)


def served_by(waves):
    """The dense tile kernel served the last call, with `waves` waves per workgroup."""
    dev = get_device()
    assert dev.lib.cs_last_kernel(dev.ctx) == KERNEL_MFMA_DENSE
    assert dev.lib.cs_last_dense_waves(dev.ctx) == waves


def _positive(rng, shape, kind):
    if kind == "gamma":
        return rng.gamma(4.0, 0.25, size=shape).astype(np.float32)
    return np.minimum(rng.gamma(20, 0.05, size=shape), 10.0).astype(np.float32)      # "hic" of test_gpu_mfma.py


def device_map(sig, *, full=True, sym_upper=False, window=None, pitch=None, out_cols=None):
    """cs_normxcorr2 on a device-resident float32 map into a float32 buffer, as bench.py calls it.  window = (a, b): the
    rows a .. b - 1 only, from a slab of the input rows they reach."""
    dev = get_device()
    n, cols = sig.shape
    kspec = engine.KernelSpec(loops(), None)
    code = np_dtype_code(np.float32)
    a, b = window or (0, n)
    ra, rb = (max(0, a - 8), min(n, b + 8)) if window else (0, n)
    ld = pitch or cols
    host = np.zeros((rb - ra, ld), np.float32)
    host[:, :cols] = sig[ra:rb]
    d_sig = dev.to_device(host)
    ld_out = out_cols or cols
    d_out = dev.zeros((b - a) * ld_out, np.float32)
    engine.run_normxcorr2(dev, CsMatrix(d_sig.ptr, code, LAYOUT_DENSE, ld, 0, 0, ra), (n, cols), kspec,
                          CsMatrix(d_out.ptr, code, LAYOUT_DENSE, ld_out, 0, 0, a), full=full, sym_upper=sym_upper,
                          max_dist=None, precision="f32", row_window=window)
    return d_out.download().reshape(b - a, ld_out)[:, :cols]


# (200, 264): 4 x 5 tiles -- inner tiles with the unclamped DMA form, every edge and corner; (1536, 1600): 600 tiles on a grid
# of 512 -- a workgroup runs two tiles: prefetch into the squares' planes, deferred epilogue; (1280, 2048): tiles_x = 32
# divides the XCD step -- the skewed tile walk
@pytest.mark.parametrize("kind", ["gamma", "hic"])
@pytest.mark.parametrize("shape,full", [((200, 264), True), ((200, 264), False), ((1536, 1600), True), ((1280, 2048), True)])
def test_bit_identical_to_the_4_wave_instance(shape, full, kind, monkeypatch):
    rng = np.random.default_rng(shape[0] + shape[1] + (kind == "hic"))
    sig = _positive(rng, shape, kind)
    py8, _ = cud.normxcorr2(sig, loops(), full=full)                 # the Python surface: float64 container
    served_by(8)
    dv8 = device_map(sig, full=full)
    served_by(8)
    monkeypatch.setenv(SWITCH, "1")
    py4, _ = cud.normxcorr2(sig, loops(), full=full)
    served_by(4)
    dv4 = device_map(sig, full=full)
    served_by(4)
    assert py8.dtype == np.float64 and dv8.dtype == np.float32
    assert np.abs(dv4).max() > 0.01
    assert np.array_equal(dv8, dv4)
    assert np.array_equal(py8, py4)


@pytest.mark.parametrize("scale", ["tiny", "huge"])
def test_oracle_scales(scale):
    rng = np.random.default_rng(256 + (scale == "huge"))
    sig = (rng.gamma(2.0, 1.0, size=(256, 256)) * (3e-7 if scale == "tiny" else 7e8)).astype(np.float32)
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), full=full)
        served_by(8)
        want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 256, full=full)
        assert_parity(got, want, cond, "f32", f"dense8 {scale} full={full}")


def test_oracle_sym_upper():
    rng = np.random.default_rng(9)
    sig = np.triu(rng.gamma(2.0, 1.0, size=(260, 260))).astype(np.float32)
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), sym_upper=True, full=full)
        served_by(8)
        want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 260, sym_upper=True, full=full)
        assert_parity(got, want, cond, "f32", f"dense8 sym_upper full={full}")
        assert np.all(np.tril(got, -1) == 0)
        dv = device_map(sig, full=full, sym_upper=True)
        served_by(8)
        assert_parity(dv, want, cond, "f32", f"dense8 sym_upper float32 out full={full}")


def test_oracle_signed():
    rng = np.random.default_rng(130)
    sig = rng.normal(size=(130, 64)).astype(np.float32)
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), full=full)
        served_by(8)
        want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 130, full=full)
        assert_parity(got, want, cond, "f32", f"dense8 signed full={full}")


def test_oracle_empty_and_constant_blocks():
    """All-zero blocks (windows without signal) and a constant block (windows without variance): the waves that hold such
    a window take the literal form of the coefficient, their neighbours the lean one.  The windows that lie wholly inside one
    of the three flat 100 x 100 blocks -- 3 x 84 x 84 of 96 000 pixels, 22 % -- are ill-defined for the oracle (parity_util.py)."""
    rng = np.random.default_rng(300)
    sig = np.minimum(rng.gamma(20, 0.05, size=(300, 320)), 10.0)
    sig[20:120, 30:130] = 0.0
    sig[150:250, 200:300] = 0.0
    sig[180:280, 40:140] = 1.25
    sig = sig.astype(np.float32)
    want = {full: c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 300, full=full) for full in (True, False)}
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), full=full)
        served_by(8)
        assert_parity(got, want[full][0], want[full][1], "f32", f"dense8 blocks full={full}", max_ill_frac=0.23)
        dv = device_map(sig, full=full)
        served_by(8)
        assert_parity(dv, want[full][0], want[full][1], "f32", f"dense8 blocks float32 out full={full}", max_ill_frac=0.23)
        assert np.all(dv[60:80, 70:90] == 0)


def test_xcorr2():
    from oracle import pearson_oracle as orc
    rng = np.random.default_rng(264)
    sig = rng.gamma(2.0, 1.0, size=(200, 264)).astype(np.float32)
    got = cud.xcorr2(sig, loops(), threshold=1e-4)
    served_by(8)
    want = orc.xcorr2_oracle(sig.astype(np.float64), loops(), threshold=0)
    near = np.abs(np.abs(want) - 1e-4) < 1e-5
    ref = np.where(np.abs(want) < 1e-4, 0.0, want)
    assert np.abs(got - ref)[~near].max() < 3e-6 * np.abs(want).max()
    assert np.all(got[:8] == 0) and np.all(got[:, :8] == 0) and np.all(got[-8:] == 0) and np.all(got[:, -8:] == 0)


def test_row_windows():
    """Row windows that start and end inside a tile (slab inputs): the rows of the whole map."""
    rng = np.random.default_rng(4)
    n, cols = 330, 200
    sig = rng.gamma(2.0, 1.0, size=(n, cols)).astype(np.float32)
    whole = device_map(sig)
    served_by(8)
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, n, full=True)
    assert_parity(whole, want, cond, "f32", "dense8 whole map")
    for a, b in [(0, 37), (37, 200), (200, 201), (201, 325), (325, 330)]:
        got = device_map(sig, window=(a, b))
        served_by(8)
        assert_parity(got, want[a:b], cond[a:b], "f32", f"dense8 rows {a}:{b}")
        assert np.abs(got - whole[a:b]).max() <= 2e-6, (a, b)


def test_other_dense_calls_keep_the_4_wave_instance():
    """Rows that are no multiple of 4 long, or an output pitch that is none, take 4-byte transfers; other template sizes and a
    template whose rows do not mirror have no 8-wave instance."""
    rng = np.random.default_rng(70)
    sig = rng.gamma(2.0, 1.0, size=(130, 70)).astype(np.float32)          # ns % 4 != 0
    got = device_map(sig)
    served_by(4)
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 130, full=True)
    assert_parity(got, want, cond, "f32", "4-wave instance, ns % 4 != 0")
    sig = rng.gamma(2.0, 1.0, size=(130, 72)).astype(np.float32)          # output rows not 16-byte aligned
    got = device_map(sig, out_cols=73)
    served_by(4)
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, 130, full=True)
    assert_parity(got, want, cond, "f32", "4-wave instance, output pitch 73")
    got = device_map(sig)
    served_by(8)
    assert_parity(got, want, cond, "f32", "8-wave instance, same map")
    skew = loops().copy()
    skew[0, 3] += 0.01                                                    # rows no longer mirror
    got, _ = cud.normxcorr2(sig, skew, full=True)
    served_by(4)
    got, _ = cud.normxcorr2(sig, loops()[1:-1, 1:-1], full=True)          # 15 x 15
    served_by(4)
