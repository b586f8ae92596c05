"""--subsample on the device, host side: the C structs against the header, the entry's symbol, the argument checks of the
wrapper, and the exact-pmf helper the GPU tests check the device draws against (tests/subsample_util.py)."""
import ctypes
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

from chromosight_amd import _lib
from chromosight_amd import subsample as css
from tests.subsample_util import block_pmf, chi2_against_pmf, two_sample_chi2

ROOT = pathlib.Path(__file__).resolve().parents[1]


def test_subsample_abi_symbol_declared_and_exported():
    text = (ROOT / "include" / "chromosight_hip.h").read_text()
    assert "int cs_subsample(" in text
    assert "cs_subsample" in _lib.ABI_SYMBOLS
    assert hasattr(_lib.load_library(), "cs_subsample")


def test_subsample_struct_layouts_match_header(tmp_path):
    assert ctypes.sizeof(_lib.CsSubsampleParams) == 24
    assert ctypes.sizeof(_lib.CsSubsampleBlock) == 24 == css.BLOCK_DTYPE.itemsize
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = [("cs_subsample_params", _lib.CsSubsampleParams), ("cs_subsample_block", _lib.CsSubsampleBlock)]
    fields = [(name, f) for name, s in pairs for f, _ in s._fields_]
    src = tmp_path / "ss.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s%s    return 0;\n}\n' % (
        ROOT / "include" / "chromosight_hip.h",
        "".join(f'    printf("%zu\\n", sizeof({name}));\n' for name, _ in pairs),
        "".join(f'    printf("%zu\\n", offsetof({name}, {f}));\n' for name, f in fields)))
    exe = tmp_path / "ss"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), str(src)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:2] == [ctypes.sizeof(s) for _, s in pairs]
    assert out[2:] == [getattr(s, f).offset for name, s in pairs for f, _ in s._fields_]
    # the numpy view of the block table has the same fields at the same offsets
    assert [css.BLOCK_DTYPE.fields[f][1] for f, _ in _lib.CsSubsampleBlock._fields_] == \
        [getattr(_lib.CsSubsampleBlock, f).offset for f, _ in _lib.CsSubsampleBlock._fields_]


@pytest.mark.parametrize("sample,msg", [(-0.1, "Subsample must be strictly positive."), (1.5, "Subsample cannot be above 1"),
                                        (float("nan"), "proportion")])
def test_sample_checks_use_the_host_messages(sample, msg):
    with pytest.raises(ValueError, match=msg):
        css.check_sample(sample)
    assert css.check_sample(0) == 0.0 and css.check_sample(1) == 1.0


def test_block_pmf_is_a_distribution_with_the_right_support():
    pmf = block_pmf([3, 2, 1], [False, True, False], 0.5)        # pool 3 + 2 + 1 + mirror 2 = 8, keep 4
    assert abs(sum(pmf.values()) - 1.0) < 1e-12
    for x in pmf:
        assert all(0 <= a <= c for a, c in zip(x, [3, 2, 1]))
    # the trans form: no mirror, every stored vector sums to keep
    pmf = block_pmf([2, 2, 1], [False, False, False], 0.6)
    assert all(sum(x) == 3 for x in pmf)


@pytest.mark.parametrize("counts,mirrored,sample", [([3, 2, 1], [False, True, False], 0.5), ([2, 1, 2], [False, False, False], 0.6),
                                                     ([4, 1], [True, False], 0.3)])
def test_block_pmf_agrees_with_numpys_sampler(counts, mirrored, sample):
    """The pmf the GPU tests use is the distribution of the host path's draw (numpy multivariate_hypergeometric over the pool,
    upper copies stored)."""
    rng = np.random.default_rng(7)
    pool = np.array(list(counts) + [c for c, m in zip(counts, mirrored) if m], dtype=np.int64)
    keep = int(sample * pool.sum())
    draws = rng.multivariate_hypergeometric(pool, keep, size=20000, method="marginals")[:, :len(counts)]
    pmf = block_pmf(counts, mirrored, sample)
    assert chi2_against_pmf([tuple(d) for d in draws], pmf) > 1e-3
    # and a wrong pmf (no mirror copies) is told apart
    if any(mirrored):
        assert chi2_against_pmf([tuple(d) for d in draws], block_pmf(counts, [False] * len(counts), sample)) < 1e-3


def test_two_sample_chi2_tells_samples_apart():
    rng = np.random.default_rng(3)
    a = rng.hypergeometric(400, 500, 450, size=4000)
    assert two_sample_chi2(a, rng.hypergeometric(400, 500, 450, size=4000)) > 1e-3
    assert two_sample_chi2(a, rng.hypergeometric(410, 490, 450, size=4000)) < 1e-3
