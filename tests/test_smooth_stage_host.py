"""--smooth-trend in the one-call staging (cs_stage_blocks_opt, CS_STAGE_SMOOTH): what can be checked without a GPU -- the
entry is declared, exported and bound, the pinned struct sizes did not move, and the genome drivers take `smooth`."""
import ctypes
import inspect
import pathlib
import re
import types

import numpy as np

from chromosight_amd import _lib, parallel, pipeline, plan
from chromosight_amd.utils import preprocessing as preproc

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _header():
    text = (ROOT / "include" / "chromosight_hip.h").read_text()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_stage_blocks_opt_is_declared_exported_and_bound():
    text = _header()
    assert re.search(r"\bint\s+cs_stage_blocks_opt\s*\(", text)
    assert re.search(r"\bCS_STAGE_SMOOTH\s*=\s*1\b", text)
    assert "cs_stage_blocks_opt" in _lib.ABI_SYMBOLS
    assert _lib.STAGE_SMOOTH == 1
    lib = _lib.load_library()
    assert hasattr(lib, "cs_stage_blocks_opt") and hasattr(lib, "cs_stage_blocks")
    # the flags are the seventh argument, behind the arguments of cs_stage_blocks
    assert _lib._PROTOTYPES["cs_stage_blocks_opt"][1][:6] == _lib._PROTOTYPES["cs_stage_blocks"][1]
    assert _lib._PROTOTYPES["cs_stage_blocks_opt"][1][6] is ctypes.c_uint32
    assert "cs_stage_blocks_opt" in _lib._CAPTURED


def test_struct_sizes_did_not_move():
    assert ctypes.sizeof(_lib.CsStageBlock) == 80
    assert ctypes.sizeof(_lib.CsCall) == 176


def test_smoothed_staging_is_replayed_through_the_staging_call_number():
    fn, kinds = plan._SLOTS["cs_stage_blocks_opt"]
    assert fn == _lib.CALL_STAGE_BLOCKS == plan._SLOTS["cs_stage_blocks"][0]
    assert kinds == plan._SLOTS["cs_stage_blocks"][1] + "i"
    call = _lib.CsCall()
    plan._fill(call, fn, kinds, (1, 2, 3, 4, 23, 10.0, _lib.STAGE_SMOOTH), 0)
    assert (call.i[0], call.i[1], call.d[0]) == (23, 1, 10.0)
    plain = _lib.CsCall()
    plan._fill(plain, *plan._SLOTS["cs_stage_blocks"], (1, 2, 3, 4, 23, 10.0), 0)
    assert plain.i[1] == 0                                   # what cs_run_calls reads as "no flags"


def test_genome_drivers_take_smooth():
    for fn in (parallel.genome_step, parallel.detect_patterns, parallel.stage_genome, parallel.detect_genome, pipeline.detect,
               pipeline.quantify, pipeline.DeviceCool._stage_fast):
        p = inspect.signature(fn).parameters.get("smooth")
        assert p is not None and p.default is False, fn.__qualname__


def test_a_smoothed_step_is_plannable_like_a_plain_one():
    genome = types.SimpleNamespace(view_for=lambda *a: None, dev=types.SimpleNamespace(pinned_empty=lambda *a: None))
    loops = dict(max_dist=2_000_000, max_iterations=1, kernels=[np.ones((17, 17))])
    borders = dict(max_dist=0, max_iterations=1, kernels=[np.ones((17, 17))] * 3)
    for cfgs in ([loops], [borders], [loops, borders]):
        assert plan.plannable(genome, cfgs, None)
        assert plan.plannable(genome, cfgs, None, smooth=True)
    assert not plan.plannable(genome, [dict(loops, max_iterations=2)], None, smooth=True)
    assert not plan.plannable(genome, [loops], 0.999, smooth=True)


def test_trailing_zeros_never_pool():
    """Why the device fits the n_diags kept entries and not all n of the block (the reference's input has zeros behind the
    kept diagonals): a law is never negative, so the zeros behind it change nothing in front of them."""
    rng = np.random.default_rng(5)
    for n_diags, n in ((3, 9), (64, 70), (1000, 1640)):
        law = rng.random(n_diags) * np.linspace(2.0, 0.1, n_diags)
        law[rng.random(n_diags) < 0.1] = 0.0
        full = np.zeros(n)
        full[:n_diags] = law
        assert np.array_equal(preproc._isotonic_non_increasing(full)[:n_diags], preproc._isotonic_non_increasing(law))
