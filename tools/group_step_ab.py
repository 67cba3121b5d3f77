#!/usr/bin/env python3
"""A/B of the two ways to step a trunk group from the host, in ONE process on ONE set of engines:

  separate   the leader's host-output vapx_step, then one host-output vapx_step per follower (TrunkGroup.step's calls): every model
             copies n x 784 floats to the host and synchronises
  wire       one vapx_step_group (TrunkGroup.step_wire): every model device-resident, wire_pack_kernel, one compact copy, one sync

Page-locked host buffers on both sides, alternating blocks of ticks after a warm-up that fills the context window; prints the
median of every block, the per-variant median over all timed ticks and the spread between blocks of the same variant (the noise a
difference has to beat), as one JSON line.  Default shape: BASELINE configuration 5 (bc + nod, 4096 streams, 20 Hz, T = 50).

    python tools/group_step_ab.py [--mode bc+nod] [--streams 4096] [--hz 20] [--ctx-sec 2.5] [--groups 2] [--blocks 6] [--ticks 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", default="bc+nod")
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hz", type=int, default=20)
    ap.add_argument("--ctx-sec", type=float, default=2.5)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6, help="timed blocks per variant")
    ap.add_argument("--ticks", type=int, default=50, help="ticks per block")
    ap.add_argument("--split-f16", action="store_true")
    args = ap.parse_args()
    from vap_realtime_amd import engine, weights as W
    names = args.mode.split("+")
    S = args.streams
    blobs = {m: W.pack_blob(*W.synthetic_weights(0, args.hz, m), m) for m in names}
    grp = engine.TrunkGroup(blobs, args.hz, args.ctx_sec, max_streams=S, groups=args.groups, split_f16=args.split_f16)
    hop = grp.hop
    rng = np.random.default_rng(0)
    pool = 8                                                    # frames of audio, cycled
    audio = engine.pinned_empty((pool, S, 2, hop))
    audio[:] = 0.05 * rng.standard_normal((pool, S, 2, hop)).astype(np.float32)
    outs = {m: engine.pinned_empty((S, engine.OUT_STRIDE)) for m in names}
    per = grp.leader.group_wire_floats()
    wire_block = engine.pinned_empty(S * per)
    tick = [0]

    def separate():
        a = audio[tick[0] % pool]
        grp.leader.step(a, out=outs[names[0]])
        for m in names[1:]:
            grp.engines[m].step_follow(S, out=outs[m])

    def wire():
        grp.step_wire(audio[tick[0] % pool], out=wire_block)

    def run(fn, n):
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()                                                # both variants end in a stream synchronise inside the library
            ms.append((time.perf_counter() - t0) * 1e3)
            tick[0] += 1
        return ms

    warm = grp.T + 10                                           # the window is full: every later tick costs the same
    run(separate, warm // 2)
    run(wire, warm - warm // 2)
    blocks = {"separate": [], "wire": []}
    for b in range(args.blocks):
        for name, fn in (("separate", separate), ("wire", wire)) if b % 2 == 0 else (("wire", wire), ("separate", separate)):
            blocks[name].append(run(fn, args.ticks))
    res = {"mode": args.mode, "streams": S, "frame_hz": args.hz, "ctx_frames": grp.T, "overlap_groups": args.groups,
           "precision": "split" if args.split_f16 else "fp32", "ticks_per_variant": args.blocks * args.ticks,
           "bytes_to_host_per_tick": {"separate": len(names) * S * engine.OUT_STRIDE * 4, "wire": S * per * 4}}
    for name in blocks:
        meds = [statistics.median(b) for b in blocks[name]]
        res[f"{name}_block_medians_ms"] = [round(m, 4) for m in meds]
        res[f"{name}_ms"] = round(statistics.median([v for b in blocks[name] for v in b]), 4)
        res[f"{name}_block_spread_ms"] = round(max(meds) - min(meds), 4)
    res["step_wire_ms"] = res["wire_ms"]
    res["wire_minus_separate_ms"] = round(res["wire_ms"] - res["separate_ms"], 4)
    grp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
