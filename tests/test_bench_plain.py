"""bench.py without --full: the headline alone (set-up, warm-up, the timed steps, --dump-outputs, the line); every other leg
runs under --full only (tests/test_gpu_multi_device.py runs the N > 1 legs that way)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run_bench(argv, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def _line(out):
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


@pytest.mark.parametrize("argv", [["--extra", "metrics"], ["--check-union"]])
def test_legs_of_full_are_refused_without_it(argv):
    """--extra and --check-union pick legs that only --full runs: without it they are an error, not a silent no-op."""
    out = _run_bench(["--dry-run"] + argv)
    assert out.returncode == 2 and "--full" in out.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone(tmp_path):
    j = _line(_run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]))
    assert j["full"] is False and j["n_gpus"] == 1 and j["steps"] == 3 and j["warmup"] == 1
    assert j["unit"] == "distances/s" and j["value"] > 0 and j["ms_per_step"] > 0 and j["dtype"] == "f32"
    assert j["roofline"]["kernel_ms"] > 0 and j["roofline"]["achieved"] > 0
    assert j["cpu_baseline"] is None and j["build"] is None and j["build_10m"] is None
    assert not {"rerank", "bq_scan", "search", "extra"} & set(j)
    assert j["roofline"]["measured_read_only_gb_per_s"] is None  # the device's ceilings are a leg of --full
    import numpy as np
    assert np.load(tmp_path / "distances.npy").shape == (1_000_000,)


@pytest.mark.gpu
def test_plain_line_of_two_virtual_devices():
    """The N > 1 thread path without --full: the dataset replicated, both device threads timed, no build."""
    j = _line(_run_bench(["--gpus", "2", "--virtual", "--steps", "3", "--warmup", "1"]))
    assert j["full"] is False and j["n_gpus"] == 2 and "2 host threads" in j["config"]["launch"]
    assert j["replicate_1m"]["replicas"] == 1 and j["build"] is None and j["build_10m"] is None
