"""A/B of the native front-end's frame parser between two trees, on the CPU: builds tools/frontend_feed_bench.cpp against the
``ingest.cpp`` of a git revision (default: HEAD~1) and against the working tree's, runs the two programs alternately, and prints every
run's JSON line, the per-leg table and the gate:

    per leg, median(new) <= median(parent) + (max(parent) - min(parent))

The parent's own range over its runs is the only noise figure there is; where it exceeds the difference under test, lengthen the legs
(--seconds) and repeat instead of reading a verdict out of it.

    python tools/frontend_feed_ab.py [--parent HEAD~1] [--pairs 5] [--seconds 1.0] [--core 2] [--frame-hz 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "frontend_feed_bench.cpp")
NEEDS = ["include", "vap-realtime_amd/csrc/ingest.cpp", "vap-realtime_amd/csrc/pcm_tables.h"]


def build(exe, ingest_cpp):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wno-subobject-linkage", f'-DINGEST_CPP="{ingest_cpp}"', SRC, "-o", exe])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="HEAD~1", help="git revision whose ingest.cpp is the baseline")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0, help="feed() time per leg and run")
    ap.add_argument("--core", type=int, default=2, help="the feeding thread's core; the front-end's threads take the next three")
    ap.add_argument("--frame-hz", type=int, default=20, help="5: four times the bytes per frame hand-over, closer to the parser's own cost")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent] + NEEDS, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        exes = {"parent": os.path.join(tmp, "feed_parent"), "new": os.path.join(tmp, "feed_new")}
        build(exes["parent"], os.path.join(tmp, NEEDS[1]))
        build(exes["new"], os.path.join(ROOT, NEEDS[1]))
        runs = {"parent": [], "new": []}
        for k in range(a.pairs):
            for tree in ("parent", "new"):
                out = subprocess.check_output([exes[tree], "--seconds", str(a.seconds), "--core", str(a.core), "--frame-hz", str(a.frame_hz)], text=True)
                runs[tree].append(json.loads(out))
                print(json.dumps({"tree": tree, "run": k + 1, "ns_per_wire_byte": runs[tree][-1]}), flush=True)
    ok = True
    print("\n| leg | parent median | parent min .. max | new median | new min .. max | gate (median <= parent median + parent range) |")
    print("|---|---|---|---|---|---|")
    for leg in runs["parent"][0]:
        p, n = [r[leg] for r in runs["parent"]], [r[leg] for r in runs["new"]]
        bound = statistics.median(p) + max(p) - min(p)
        good = statistics.median(n) <= bound
        ok &= good
        print(f"| {leg} | {statistics.median(p):.4f} | {min(p):.4f} .. {max(p):.4f} | {statistics.median(n):.4f} | {min(n):.4f} .. {max(n):.4f} | "
              f"{statistics.median(n):.4f} <= {bound:.4f}: {'holds' if good else 'MISSED'} |")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
