#!/usr/bin/env python3
"""A/B of the two ways to step a trunk group from the host, in ONE process on ONE set of engines:

  separate   the leader's host-output vapx_step, then one host-output vapx_step per follower (TrunkGroup.step's calls): every model
             copies n x 784 floats to the host and synchronises
  wire       one vapx_step_group (TrunkGroup.step_wire): every model device-resident, wire_pack_kernel, one compact copy, one sync

Page-locked host buffers on both sides, alternating blocks of ticks after a warm-up that fills the context window; prints the
median of every block, the per-variant median over all timed ticks and the spread between blocks of the same variant (the noise a
difference has to beat), as one JSON line.  Default shape: BASELINE configuration 5 (bc + nod, 4096 streams, 20 Hz, T = 50).

    python tools/group_step_ab.py [--mode bc+nod] [--streams 4096] [--hz 20] [--ctx-sec 2.5] [--groups 2] [--blocks 6] [--ticks 50]

--vs-standalone measures what the shared trunk is worth for a MIXED group (models with rates and windows of their own, --hzs / --ctx-secs,
one value per model): one vapx_step_group per leader tick on the group, against one stand-alone engine per model of the same build stepping
the same audio at its own rate (host output, page-locked) — both as milliseconds of GPU + host time per SECOND of audio
(rate x ms per tick), in one process, in alternating blocks.  Also prints the per-launch time of the slower followers' collect / scatter
kernels (profile class trunk_collect) and the board's clock and watts during the timed blocks.

    python tools/group_step_ab.py --vs-standalone --mode vap+bc+nod --hzs 20,20,10 --ctx-secs 2.5,5,10 --streams 1024 [--split-f16]
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
    ap.add_argument("--vs-standalone", action="store_true", help="mixed group against one stand-alone engine per model, per second of audio")
    ap.add_argument("--hzs", default="", help="--vs-standalone: one frame rate per model, comma-separated (default: --hz for all)")
    ap.add_argument("--ctx-secs", default="", help="--vs-standalone: one window per model, comma-separated (default: --ctx-sec for all)")
    args = ap.parse_args()
    if args.vs_standalone:
        return vs_standalone(args)
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


def vs_standalone(args):
    from vap_realtime_amd import engine, weights as W
    names = args.mode.split("+")
    hzs = [int(v) for v in args.hzs.split(",")] if args.hzs else [args.hz] * len(names)
    ctxs = [float(v) for v in args.ctx_secs.split(",")] if args.ctx_secs else [args.ctx_sec] * len(names)
    S = args.streams
    blobs = {m: W.pack_blob(*W.synthetic_weights(0, hz, m), m) for m, hz in zip(names, hzs)}
    grp = engine.TrunkGroup(blobs, hzs, ctxs, max_streams=S, groups=args.groups, split_f16=args.split_f16)
    solo = {m: engine.Engine(blobs[m], grp.hz[m], grp.ctx[m], max_streams=S, mode=m, groups=args.groups, split_f16=args.split_f16) for m in names}
    rng = np.random.default_rng(0)
    pool, hop_l = 8, grp.hop
    Rmax = max(grp.R.values())
    long_audio = 0.05 * rng.standard_normal((S, 2, pool * Rmax * hop_l)).astype(np.float32)    # one signal, cut at every model's hop
    cuts = {}
    for hop in {hop_l} | set(grp.hop_of.values()):
        n = long_audio.shape[2] // hop
        blk = engine.pinned_empty((n, S, 2, hop))
        blk[:] = long_audio.reshape(S, 2, n, hop).transpose(2, 0, 1, 3)
        cuts[hop] = blk
    wire_block = engine.pinned_empty(S * grp.leader.group_wire_floats())
    outs = {m: engine.pinned_empty((S, engine.OUT_STRIDE)) for m in names}
    tick = {"group": 0, **{m: 0 for m in names}}

    def group_tick():
        a = cuts[hop_l]
        grp.step_wire(a[tick["group"] % len(a)], out=wire_block)
        tick["group"] += 1

    def solo_tick(m):
        a = cuts[grp.hop_of[m]]
        solo[m].step(a[tick[m] % len(a)], out=outs[m])
        tick[m] += 1

    def timed(fn, n):
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    for _ in range(max(grp.T_of[m] * grp.R[m] for m in names) + 2 * Rmax):      # every window full, group and stand-alone alike
        group_tick()
    for m in names:
        for _ in range(grp.T_of[m] + 2):
            solo_tick(m)
    slow = [m for m in names if grp.R[m] > 1]
    for m in slow:
        grp.engines[m].profile_enable([15])
    ticks = (args.ticks + Rmax - 1) // Rmax * Rmax                               # whole follower frames per block
    g_blocks, s_blocks = [], {m: [] for m in names}
    board = None
    try:
        sys.path.insert(0, ROOT)
        from bench import BoardWatch
        watch = BoardWatch()
    except Exception:                                                            # noqa: BLE001 - no hwmon files: the numbers stand without them
        watch = None
    import contextlib
    with (watch if watch is not None else contextlib.nullcontext()):
        for b in range(args.blocks):
            order = ["group"] + names if b % 2 == 0 else names + ["group"]
            for who in order:
                if who == "group":
                    g_blocks.append(timed(group_tick, ticks))
                else:
                    s_blocks[who].append(timed(lambda: solo_tick(who), max(1, ticks // grp.R[who])))
    if watch is not None:
        board = watch.record()
    res = {"mode": args.mode, "streams": S, "frame_hz": grp.hz, "ctx_frames": grp.T_of, "leader": grp.order[0], "R": grp.R,
           "overlap_groups": args.groups, "precision": "split" if args.split_f16 else "fp32", "leader_ticks_per_block": ticks, "blocks": args.blocks}
    g_means = [statistics.fmean(b) for b in g_blocks]                           # the mean: ticks with and without a slower model's frame alternate
    res["group_ms_per_leader_tick"] = round(statistics.median(g_means), 4)
    res["group_block_spread_ms"] = round(max(g_means) - min(g_means), 4)
    res["group_ms_per_audio_second"] = round(grp.hz[grp.order[0]] * res["group_ms_per_leader_tick"], 3)
    total = 0.0
    res["standalone"] = {}
    for m in names:
        means = [statistics.fmean(b) for b in s_blocks[m]]
        per_tick = statistics.median(means)
        res["standalone"][m] = {"ms_per_tick": round(per_tick, 4), "block_spread_ms": round(max(means) - min(means), 4),
                                "ms_per_audio_second": round(grp.hz[m] * per_tick, 3)}
        total += grp.hz[m] * per_tick
    res["standalone_ms_per_audio_second"] = round(total, 3)
    res["group_over_standalone"] = round(res["group_ms_per_audio_second"] / total, 4)
    res["trunk_collect"] = {}
    for m in slow:
        pr = grp.engines[m].profile_read().get("trunk_collect")
        if pr:
            res["trunk_collect"][m] = {"launches": int(pr[1]), "ms_total": round(pr[0], 3), "us_per_launch": round(1e3 * pr[0] / pr[1], 2)}
    res["board"] = board
    for e in solo.values():
        e.close()
    grp.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
