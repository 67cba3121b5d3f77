#!/usr/bin/env python3
"""What attaching to a call in progress costs: ONE ``vapx_prefill`` of a full context window against the only way in that existed before
it, T ``vapx_step`` calls of a library build WITHOUT the call (the parent commit's libvapx.so).

    python tools/prefill_cost.py --parent-lib /path/to/parent/libvapx.so [--out profiles/prefill/prefill_cost.json]

Every measurement is a fresh child process (a library is chosen once per process, VAPX_LIBRARY), in the order rotation of tools/ab_lib.sh
taken twice: steps, prefill, prefill, steps.  This process never touches the GPU.  A child builds one engine of ``--max-streams`` slots
(max_batch the same: the scratch of a loaded engine, so one stream's window is one chunk), keeps the audio on the device, and times, after
one untimed round, ``--reps`` rounds of
    prefill   reset the streams, one prefill of n streams x T frames, synchronise
    steps     reset the streams, T device-resident steps of the n streams, synchronise
by the host's clock around the calls (what the tick thread of a server would lose).  Cases: (20 Hz, T 50), (20 Hz, T 200), (50 Hz, T 250),
fp32 and split-precision, n = 1 and n = 64.  The report gives the medians, the ratio, and the prefill against the tick period of a loaded
20 Hz engine (50 ms): does an attach fit in the slack of one tick."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(20, 2.5), (20, 10.0), (50, 5.0)]
TICK_MS = 50.0


def child(args) -> int:
    sys.path.insert(0, ROOT)
    import torch
    from vap_realtime_amd import engine, synth, weights as W
    rows = []
    for hz, ctx in CASES:
        T, hop = int(ctx * hz), 16000 // hz
        cpc, vap = W.synthetic_weights(0, hz, "vap")
        blob = W.pack_blob(cpc, vap)
        for split in (False, True):
            eng = engine.Engine(blob, hz, ctx, max_streams=args.max_streams, split_f16=split)
            for n in (1, 64):
                audio = torch.from_numpy(synth.dialogue_batch(list(range(n)), hop * T)).cuda().contiguous()      # [n, 2, T * hop]
                frames = audio.reshape(n, 2, T, hop).permute(2, 0, 1, 3).contiguous()                               # [T, n, 2, hop]
                out = torch.empty(n, engine.OUT_STRIDE, device="cuda")
                ms = []
                for rep in range(args.reps + 1):
                    for s in range(n):
                        eng.reset_stream(s)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if args.child == "prefill":
                        eng.prefill_device(n, audio.data_ptr(), T)
                    else:
                        for f in range(T):
                            eng.step_device(n, frames[f].data_ptr(), hop, out.data_ptr())
                    torch.cuda.synchronize()
                    if rep:
                        ms.append((time.perf_counter() - t0) * 1e3)
                fill = int(engine.split_state(eng.export_streams([0]), T)["n_frames"][0])
                assert fill == T, (fill, T)
                rows.append({"frame_hz": hz, "T": T, "path": "split" if split else "fp32", "streams": n, "what": args.child,
                             "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms), "reps": args.reps})
            eng.close()
    print(json.dumps({"child": args.child, "library": "parent libvapx.so" if os.environ.get("VAPX_LIBRARY") else "built", "rows": rows}))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", help="libvapx.so of the parent commit (the steps run on it)")
    ap.add_argument("--max-streams", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["prefill", "steps"], default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("--parent-lib: the parent commit's libvapx.so is needed")
    runs = []
    for what in ("steps", "prefill", "prefill", "steps"):
        env = dict(os.environ)
        env.pop("VAPX_LIBRARY", None)
        if what == "steps":
            env["VAPX_LIBRARY"] = os.path.abspath(args.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, "--max-streams", str(args.max_streams),
                            "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:                       # nothing more is started on the GPU after a child that ended badly
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            return p.returncode or 1
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    table = []
    for r in runs[1]["rows"]:
        key = {k: r[k] for k in ("frame_hz", "T", "path", "streams")}
        pick = lambda run: next(x for x in run["rows"] if all(x[k] == v for k, v in key.items()))   # noqa: E731
        pre, stp = [pick(runs[1])["ms_median"], pick(runs[2])["ms_median"]], [pick(runs[0])["ms_median"], pick(runs[3])["ms_median"]]
        p_ms, s_ms = sum(pre) / 2, sum(stp) / 2
        table.append(dict(key, prefill_ms=round(p_ms, 3), prefill_runs_ms=[round(x, 3) for x in pre], steps_ms=round(s_ms, 3),
                          steps_runs_ms=[round(x, 3) for x in stp], ratio_steps_over_prefill=round(s_ms / p_ms, 2),
                          prefill_share_of_50ms_tick=round(p_ms / TICK_MS, 3)))
    report = {"order": ["steps(parent)", "prefill", "prefill", "steps(parent)"], "max_streams": args.max_streams, "reps": args.reps,
              "table": table, "runs": runs}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
    for t in table:
        print(json.dumps(t))
    return 0


if __name__ == "__main__":
    sys.exit(main())
