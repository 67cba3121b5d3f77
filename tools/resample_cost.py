#!/usr/bin/env python3
"""What an input rate costs per step, in ONE process on ONE box: three engines of the same shape — input rate unset (16 kHz), 8000 and
48000 — stepped in alternating blocks after a warm-up that fills the context window.

  device legs   audio already on the device (VAPX_AUDIO_DEVICE | VAPX_OUT_DEVICE): HIP events around each block of steps; the difference
                to the unset engine is input_classes_kernel (the engine's one input launch per step, here resampling fp32 input) plus
                what the different input size does to the tick
  host legs     audio in page-locked host memory, output in page-locked host memory (the serving path): host clock around a step, which
                ends in a stream synchronise inside the library; the H2D bytes per tick are printed next to each leg

Prints one JSON line: per leg the median ms per step over all timed steps, the block medians and their spread (the noise a difference
has to beat), the differences against the unset engine of the SAME run, and the board's watts and shader clock during the timed blocks.
Default shape: 4096 streams x 20 Hz x T 50.

    python tools/resample_cost.py [--streams 4096] [--hz 20] [--ctx-sec 2.5] [--groups 2] [--blocks 4] [--steps 50] [--rates 8000,48000]
"""
import argparse
import contextlib
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
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hz", type=int, default=20)
    ap.add_argument("--ctx-sec", type=float, default=2.5)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=4, help="timed blocks per leg")
    ap.add_argument("--steps", type=int, default=50, help="steps per block (blocks x steps timed steps per leg)")
    ap.add_argument("--rates", default="8000,48000", help="input rates to hold against the unset engine")
    ap.add_argument("--split-f16", action="store_true")
    args = ap.parse_args()
    import torch
    from vap_realtime_amd import engine, weights as W
    S, pool = args.streams, 4
    blob = W.pack_blob(*W.synthetic_weights(0, args.hz, "vap"), "vap")
    rates = [16000] + [int(r) for r in args.rates.split(",") if r]
    rng = np.random.default_rng(0)
    legs = {}
    for r in rates:
        eng = engine.Engine(blob, args.hz, args.ctx_sec, max_streams=S, groups=args.groups, split_f16=args.split_f16, input_hz=r)
        host = engine.pinned_empty((pool, S, 2, eng.hop_in))
        host[:] = 0.05 * rng.standard_normal((pool, S, 2, eng.hop_in)).astype(np.float32)
        legs[r] = {"eng": eng, "host": host, "dev": torch.from_numpy(np.array(host)).cuda(), "out_host": engine.pinned_empty((S, engine.OUT_STRIDE)),
                   "out_dev": torch.empty((S, engine.OUT_STRIDE), device="cuda"), "tick": 0}

    def step_dev(L):
        a = L["dev"][L["tick"] % pool]
        L["eng"].step_device(S, a.data_ptr(), L["eng"].hop_in, L["out_dev"].data_ptr())
        L["tick"] += 1

    def step_host(L):
        L["eng"].step(L["host"][L["tick"] % pool], out=L["out_host"])
        L["tick"] += 1

    def block_dev(L, n):                                   # device events around the block: ms per step
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            step_dev(L)
        b.record()
        b.synchronize()
        return [a.elapsed_time(b) / n] * n

    def block_host(L, n):                                  # the step ends in a stream synchronise inside the library
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            step_host(L)
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    T = legs[16000]["eng"].T
    for L in legs.values():                                # every window full, both paths warm
        block_dev(L, T + 5)
        block_host(L, 5)
    try:
        from bench import BoardWatch
        watch = BoardWatch()
    except Exception:                                      # noqa: BLE001 - no hwmon files: the numbers stand without them
        watch = None
    res = {"streams": S, "frame_hz": args.hz, "ctx_frames": T, "overlap_groups": args.groups, "precision": "split" if args.split_f16 else "fp32",
           "timed_steps_per_leg": args.blocks * args.steps, "blocks": args.blocks}
    for kind, fn in (("device", block_dev), ("host", block_host)):
        blocks = {r: [] for r in rates}
        with (watch if watch is not None else contextlib.nullcontext()):
            for b in range(args.blocks):
                for r in (rates if b % 2 == 0 else rates[::-1]):      # interleaved, the order alternates
                    blocks[r].append(fn(legs[r], args.steps))
        out = {}
        for r in rates:
            meds = [statistics.median(x) for x in blocks[r]]
            e = legs[r]["eng"]
            out["unset" if r == 16000 else str(r)] = {
                "ms_per_step": round(statistics.median([v for x in blocks[r] for v in x]), 4),
                "block_medians_ms": [round(m, 4) for m in meds], "block_spread_ms": round(max(meds) - min(meds), 4),
                "input_bytes_per_tick": S * 2 * e.hop_in * 4,
                "resampler_bytes_per_tick": 0 if r == 16000 else S * 2 * (e.hop_in + e.hop) * 4}
        base = out["unset"]["ms_per_step"]
        for r in rates[1:]:
            out[str(r)]["minus_unset_ms"] = round(out[str(r)]["ms_per_step"] - base, 4)
        if watch is not None:
            out["board"] = watch.record()
            watch = BoardWatch()
        res[kind] = out
    for L in legs.values():
        L["eng"].close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
