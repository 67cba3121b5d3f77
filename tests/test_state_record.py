"""A stream's state record (csrc/state_record.h) is described once: tests/native/state_record_check.cpp includes only that header and
holds state_layout against offsets written out by hand - T in {1, 50, 512}, leader and follower, a resampler history of 0, 28, 56 and 80
floats, with and without the cache: every section 16-byte aligned, in the order header, lstm, carry, history, ring, cache, the total the
formula of include/vapx.h - and state_header_check against one header per rule and against headers that break two rules, which pins the
order the rules are evaluated in.  Under Address + UndefinedBehaviour sanitizers.  No GPU involved."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "state_record_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_state_record_layout_and_header_rules(tmp_path):
    exe = tmp_path / "state_record_check"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", str(exe), SRC], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0 and not cc.stderr.strip(), cc.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    for m in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert m not in log, log[-6000:]
    assert r.returncode == 0 and log.startswith("ok: 48 layouts, 27 headers"), log[-3000:]
