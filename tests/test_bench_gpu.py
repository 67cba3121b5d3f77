"""bench.py end to end on the GPU: a plain run times the very ticks a --full run times (same dumped outputs of the last timed step),
without the parity gate; the --full run still gates on the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, tmp_path, tag):
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", "6", "--warmup", "2", "--dump-outputs", str(out)] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0]), np.load(out / "out_vap.npy")


def test_plain_run_times_the_ticks_of_the_full_run(tmp_path):
    plain, got = run_bench([], tmp_path, "plain")
    full, want = run_bench(["--full", "--configs=", "--no-latency", "--no-cpu-baseline", "--full-record", str(tmp_path / "full.json")],
                           tmp_path, "full")
    for line in (plain, full):
        assert line["value"] > 0 and line["unit"] == "frames/s" and line["dtype"] == "f32" and line["steps"] == 6 and line["warmup"] == 2
        assert line["config"]["workload"].startswith("c2:")
    assert "parity_gate" not in plain and "full_record" not in plain
    assert full["parity_gate"]["ok"] is True and full["full_record"] == str(tmp_path / "full.json")
    assert json.load(open(tmp_path / "full.json"))["parity_gate"]["worst_abs"] <= 1e-4
    assert got.shape == (256, want.shape[1]) and np.array_equal(got, want)
