"""bench.py on the GPU: a plain run prints the headline line and nothing it had to take extra runs for; `--full` adds the
roofline (and, without the trimming options, the CPU baseline, the in-run parity check and the side lines)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
BEYOND = ("roofline", "cpu_baseline", "speedup_vs_cpu_port", "parity_in_run", "converged_fit", "f32_side_line",
          "baseline_configs_side_line", "small_n_side_line", "concurrent_fits_side_line")


def _bench(tmp_path, *extra):
    # n = 1024: evaluations take the task-queue path of the headline size, in a fraction of a second per fit
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n", "1024",
                          *extra], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    out = _bench(tmp_path)
    assert all(k in out for k in HEADLINE), out
    assert out["value"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["evals_per_fit"] > 0
    assert not set(out) & set(BEYOND), sorted(set(out) & set(BEYOND))


@pytest.mark.gpu
def test_full_run_adds_the_roofline(tmp_path):
    out = _bench(tmp_path, "--full", "--no-side-lines")
    assert all(k in out for k in HEADLINE), out
    assert out["roofline"]["kernels"] and out["roofline"]["achieved"] > 0
    assert not set(out) & (set(BEYOND) - {"roofline"})
