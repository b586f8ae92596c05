"""bench.py's contract: a plain run measures its headline figure and nothing else; --full adds the reported extras."""
import json
import pathlib
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

# what a plain line holds: the headline and what the timed run itself yields (no leg of its own)
HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
# the reported extras of the default c2 command, --full only
FULL_KEYS = {"gpu_state", "north_star_c4p", "c3_from_csr", "wide_templates", "sharded_genome", "detect_wallclock", "quantify_c5",
             "c2_f64", "api_call_ms", "cpu_baseline"}


def test_full_is_opt_in(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    args = bench.parse()
    assert not args.full and not args.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` in a fresh process: one line with the headline fields and
    none of --full's legs, the last step's map dumped, and little time spent outside the steps."""
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    run = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert run.returncode == 0, run.stderr[-4000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-4000:]
    line = json.loads(lines[0])
    assert HEADLINE_KEYS <= line.keys()
    assert not FULL_KEYS & line.keys(), sorted(FULL_KEYS & line.keys())
    assert line["steps"] == steps and line["warmup"] == warmup and line["value"] > 0 and line["ms_per_step"] > 0
    assert list(line["dumped_outputs"]) == ["c2_corr"]
    corr = np.load(tmp_path / "c2_corr.npy")
    assert list(corr.shape) == line["dumped_outputs"]["c2_corr"] and corr.shape[1] == 4096 and corr.dtype == np.float32
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"
