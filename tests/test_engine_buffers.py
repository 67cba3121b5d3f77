"""The engine's buffer table (csrc/engine_buffers.h) tiles every scratch buffer: tests/native/engine_buffers_check.cpp includes
only that header and holds its per-slot sizes, its poison / follower-release / peek sets and Scratch::slice against figures written
out by hand, for frame_hz in {5, 10, 20, 50}, T in {1, 64, 65, 250, 512}, B in {1, 77, 1000} and 1 .. 8 overlap groups, under
Address + UndefinedBehaviour sanitizers.  The same program holds vapx_peek's refusal rules (peek_refusal) against a hand-written table:
every peek name after a step, a prefill and the fused conv tail, "x0" either side of T = 64, the last layer's buffers in vap / nod mode
with and without VAPX_FLAG_FULL_LAST_LAYER, "comb" in one and two groups, a released buffer.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "engine_buffers_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_buffer_table_tiles_every_buffer(tmp_path):
    exe = tmp_path / "engine_buffers_check"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", str(exe), SRC], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    for m in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert m not in log, log[-6000:]
    assert r.returncode == 0 and log.startswith("ok: 32 buffers"), log[-3000:]
