"""The persistent dense kernel's epilogue on tile-scaled sums (cs_corr_mfma_body.inc, unmasked `emit`).

The coefficient is formed from the tile's scaled box sums with the 1e-4 and eps thresholds moved into the tile's
units; tiles whose scaled thresholds leave the normal float range, plain xcorr2, candidate mode and waves that hold a
near-threshold window take the literal per-pixel form.  Both must give the float64 oracle's map, and a map scaled by a
power of two must give the same coefficients while its windows stay clear of the thresholds."""
import numpy as np
import pytest

import chromosight_amd
import chromosight_amd.kernels as ck
from chromosight_amd._lib import get_device
from chromosight_amd.utils import detection as cud
from oracle import c_oracle
from parity_util import assert_parity

pytestmark = pytest.mark.gpu

KERNEL_MFMA_DENSE = 4


@pytest.fixture(autouse=True)
def f32_precision():
    old = chromosight_amd.get_precision()
    chromosight_amd.set_precision("f32")
    yield
    chromosight_amd.set_precision(old)


def last_kernel():
    dev = get_device()
    return dev.lib.cs_last_kernel(dev.ctx)


def loops():
    return np.asarray(ck.loops["kernels"][0], dtype=np.float64)


@pytest.mark.parametrize("full", [True, False])
def test_power_of_two_scales_give_the_same_map(full):
    """Maps scaled by 2^10, 2^20, 2^40: the same coefficients (to an ulp or two); 2^-10 and 2^-40 (windows under the
    reference's 1e-4 zeroing threshold: the literal per-pixel form), 2^50 (tiles near the overflow bound of the lean
    form) and 2^-70 (tiles whose scaled thresholds leave the float range: the gate sends them to the literal form)
    against the oracle."""
    rng = np.random.default_rng(71)
    sig = rng.gamma(2.0, 1.0, size=(333, 250)).astype(np.float32)          # not multiples of 64
    base, _ = cud.normxcorr2(sig, loops(), full=full)
    assert last_kernel() == KERNEL_MFMA_DENSE
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, sig.shape[0], full=full)
    assert_parity(base, want, cond, "f32", f"scale 1 full={full}")
    for e in (10, 20, 40):
        got, _ = cud.normxcorr2(sig * np.float32(2.0 ** e), loops(), full=full)
        assert np.abs(got - base).max() <= 2.5e-7, e
    for e in (-10, -40, 50, -70):
        s = sig * np.float32(2.0 ** e)
        got, _ = cud.normxcorr2(s, loops(), full=full)
        want, cond = c_oracle.normxcorr2_rows(s.astype(np.float64), loops(), 0, s.shape[0], full=full)
        assert_parity(got, want, cond, "f32", f"scale 2^{e} full={full}")


def test_tiles_of_different_scales():
    """Row bands 2^44 apart, separated by zero rows wider than a tile with its halo (a tile never holds two scales):
    every band's tiles have their own scale, and the zero rows' windows have no signal."""
    rng = np.random.default_rng(72)
    n = 512
    sig = rng.gamma(4.0, 0.25, size=(n, 300))
    sig[:64] *= 2.0 ** 40
    sig[64:224] = 0.0
    sig[224:288] *= 2.0 ** -4
    sig[288:448] = 0.0
    sig[448:] *= 2.0 ** 20
    sig = sig.astype(np.float32)
    got, _ = cud.normxcorr2(sig, loops(), full=True)
    assert last_kernel() == KERNEL_MFMA_DENSE
    want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, n, full=True)
    assert_parity(got, want, cond, "f32", "tiles of different scales")


def test_threshold_and_flat_windows():
    """Windows with mean exactly at the zeroing threshold, constant windows (zero variance: the eps cut) and empty
    windows, beside ordinary ones in the same tiles."""
    rng = np.random.default_rng(73)
    sig = rng.gamma(2.0, 1.0, size=(260, 270))
    sig[20:60, 30:90] = 1e-4                  # window mean at thr
    sig[100:150, 100:200] = 3.0               # zero variance
    sig[180:230, 10:120] = 0.0                # no signal
    sig[200:240, 150:260] = 2e-4              # mean square under thr, mean above
    sig = sig.astype(np.float32)
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), full=full)
        assert last_kernel() == KERNEL_MFMA_DENSE
        want, cond = c_oracle.normxcorr2_rows(sig.astype(np.float64), loops(), 0, sig.shape[0], full=full)
        assert_parity(got, want, cond, "f32", f"thresholds full={full}", max_ill_frac=0.2)
        assert np.all(got[120:130, 125:175] == 0.0)      # inside the flat patch
        assert np.all(got[190:220, 30:100] == 0.0)       # inside the empty patch


def test_sym_upper_and_f64_containers():
    rng = np.random.default_rng(74)
    sig = np.triu(rng.gamma(2.0, 1.0, size=(300, 300)))               # float64 container
    for full in (True, False):
        got, _ = cud.normxcorr2(sig, loops(), sym_upper=True, full=full)
        assert last_kernel() == KERNEL_MFMA_DENSE
        want, cond = c_oracle.normxcorr2_rows(sig, loops(), 0, 300, sym_upper=True, full=full)
        assert_parity(got, want, cond, "f32", f"sym_upper f64 container full={full}", max_ill_frac=0.5)
        assert np.all(np.tril(got, -1) == 0)


def test_xcorr2_keeps_its_form():
    """Plain xcorr2 (no box sums) on tiles of far different scales."""
    from oracle import pearson_oracle as orc
    rng = np.random.default_rng(75)
    sig = rng.gamma(2.0, 1.0, size=(200, 330))
    sig[:100] *= 2.0 ** 30
    sig = sig.astype(np.float32)
    k = rng.normal(size=(17, 17))
    got = cud.xcorr2(sig, k, threshold=1e-4)
    assert last_kernel() == KERNEL_MFMA_DENSE
    want = orc.xcorr2_oracle(sig.astype(np.float64), k, threshold=0)
    for rows in (slice(0, 64), slice(128, 200)):                       # tiles of one scale
        w, g = want[rows], got[rows]
        near = np.abs(np.abs(w) - 1e-4) < 1e-5
        ref = np.where(np.abs(w) < 1e-4, 0.0, w)
        assert np.abs(g - ref)[~near].max() < 3e-6 * np.abs(w).max()


def test_dense_candidate_mode():
    """Candidate mode (cand_cmin > 0) on an unmasked dense float32 map: the tile kernel keeps the literal per-pixel
    epilogue (with the candidate screen) but runs the new head / tail splits.  The candidates, re-scored in float64, are
    exactly the pixels whose float64 coefficient passes."""
    from chromosight_amd import engine
    from chromosight_amd._lib import LAYOUT_DENSE, CsMatrix, np_dtype_code
    rng = np.random.default_rng(76)
    ms, ns, pearson = 300, 270, 0.3
    a = rng.gamma(2.0, 1.0, size=(ms, ns)).astype(np.float32)
    kz = loops()
    for i0, j0 in ((60, 70), (200, 180), (150, 40)):
        a[i0 - 8:i0 + 9, j0 - 8:j0 + 9] += (3.0 * (kz - kz.min())).astype(np.float32)
    a[240:] *= np.float32(2.0 ** 30)                     # tiles of their own scale
    dev = get_device()
    ld = (ns + 15) // 16 * 16
    host = np.zeros((ms, ld), dtype=np.float32)
    host[:, :ns] = a
    buf = dev.to_device(host)
    sig = CsMatrix(buf.ptr, np_dtype_code(np.float32), LAYOUT_DENSE, ld, 0, 0)
    rows, cols, vals = engine.run_candidates(dev, sig, (ms, ns), engine.KernelSpec(kz), (0, ms), pearson=pearson,
                                             lo_diag=-(ms - 1), hi_diag=ns - 1, inter=True, full=True, sym_upper=False,
                                             max_dist=-1)
    del buf
    want, _ = c_oracle.normxcorr2_rows(a.astype(np.float64), kz, 0, ms, full=True)
    got = np.zeros((ms, ns), dtype=bool)
    got[rows, cols] = True
    exp = (want >= pearson) & (want != 0)
    edge = np.abs(want - pearson) < 1e-9
    assert exp.sum() > 10
    assert np.array_equal(got & ~edge, exp & ~edge), (int(got.sum()), int(exp.sum()))
    assert np.abs(vals - want[rows, cols]).max() < 1e-7
