"""Times the bulk state path (vapx_export_streams / vapx_import_streams) against the per-stream vapx_set_state loop, in one process on
one board, and what a background drain costs the tick.  Numbers and the command that produced them: profiles/state_bulk/README.md.

    python tools/state_bulk_bench.py --streams 4096 --hz 50 --ctx 5.0 --json out.json

(a) the existing set_state loop over every stream; (b) one import without cache (LayerNorm + GEMM rebuild, chunks of max_batch);
(c) one import with cache; (d) one export to device memory; (e) one export to page-locked host memory; then ticks of all streams with an
export of 64 streams to device memory after every tick, against the same ticks without it.  Every figure is the median of --reps
repetitions after --warmup unmeasured ones, with min / max as the spread; (b) - (d) are timed with events on the stream the work runs on,
(a) and (e) on the host clock (they end synchronised).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": xs[len(xs) // 2], "min_ms": xs[0], "max_ms": xs[-1], "reps": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hz", type=int, default=50)
    ap.add_argument("--ctx", type=float, default=5.0)
    ap.add_argument("--max_batch", type=int, default=0, help="0 = streams")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop_reps", type=int, default=3, help="repetitions of the set_state loop (a)")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--json", type=str, default=None)
    args = ap.parse_args()
    import torch
    from vap_realtime_amd import engine, synth, weights as W
    S, hz = args.streams, args.hz
    hop = 16000 // hz
    cpc, vap = W.synthetic_weights(0, hz, "vap")
    blob = W.pack_blob(cpc, vap)
    small = engine.Engine(blob, hz, args.ctx, max_streams=1, split_f16=args.split)
    T = small.T
    a1 = synth.dialogue_batch([0], hop * (T + 5))
    for f in range(T + 5):                                           # a full window that has slid: the ring is rotated
        small.step(a1[:, :, f * hop:(f + 1) * hop])
    st = small.get_state(0)
    small.close()
    big = engine.Engine(blob, hz, args.ctx, max_streams=S, max_batch=args.max_batch or S, groups=2, split_f16=args.split)
    side = torch.cuda.Stream()
    res = {"streams": S, "frame_hz": hz, "ctx_frames": T, "max_batch": big.max_batch, "split_f16": args.split,
           "device": torch.cuda.get_device_name(0)}

    # (a) the per-stream loop
    ts = []
    for _ in range(args.loop_reps):
        t0 = time.perf_counter()
        for k in range(S):
            big.set_state(k, st)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    res["a_set_state_loop"] = stats(ts)

    fl, flc = big.state_floats(False), big.state_floats(True)
    d_rec = torch.empty(S * fl, dtype=torch.float32, device="cuda")
    d_recc = torch.empty(S * flc, dtype=torch.float32, device="cuda")

    def timed(fn, n):
        out = []
        for i in range(args.warmup + n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            fn()
            e1.record(side)
            side.synchronize()
            if i >= args.warmup:
                out.append(e0.elapsed_time(e1))
        return stats(out)

    s_ = side.cuda_stream
    # (d) export to device memory: bytes moved = read + written
    for name, buf, cache, f_ in (("d_export_device_cache", d_recc, True, flc), ("d_export_device_nocache", d_rec, False, fl)):
        r = timed(lambda: big.export_streams_device(S, buf.data_ptr(), cache=cache, stream=s_), args.reps)
        r["bytes_moved"] = 2 * S * f_ * 4
        r["GBps"] = r["bytes_moved"] / (r["median_ms"] * 1e-3) / 1e9
        res[name] = r
    # (b) / (c) import from device records
    res["b_import_device_nocache"] = timed(lambda: big.import_streams_device(S, d_rec.data_ptr(), cache=False, stream=s_), args.reps)
    r = timed(lambda: big.import_streams_device(S, d_recc.data_ptr(), cache=True, stream=s_), args.reps)
    r["bytes_moved"] = 2 * S * flc * 4
    r["GBps"] = r["bytes_moved"] / (r["median_ms"] * 1e-3) / 1e9
    res["c_import_device_cache"] = r
    # (e) export to page-locked host memory (host clock: the call ends synchronised)
    pinned = engine.pinned_empty((S, flc))
    ts = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        big.export_streams(None, cache=True, out=pinned)
        if i >= args.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    r = stats(ts)
    r["bytes_to_host"] = S * flc * 4
    r["GBps_to_host"] = r["bytes_to_host"] / (r["median_ms"] * 1e-3) / 1e9
    res["e_export_pinned_cache"] = r
    del pinned

    # what a background drain costs the tick: every tick synchronised, with and without a 64-stream export behind it
    audio = torch.from_numpy(synth.noise_batch(S, hop, seed=1)).cuda()
    d_out = torch.empty(S, engine.OUT_STRIDE, device="cuda")
    n64 = min(64, S)
    d_ids = torch.arange(S, dtype=torch.int32, device="cuda")
    d_part = torch.empty(n64 * flc, dtype=torch.float32, device="cuda")

    def ticks(with_export):
        out = []
        for i in range(args.warmup + args.ticks):
            t0 = time.perf_counter()
            big.step_device(S, audio.data_ptr(), hop, d_out.data_ptr(), stream=s_)
            if with_export:
                k0 = (i * n64) % (S - n64 + 1)
                big.export_streams_device(n64, d_part.data_ptr(), ids_ptr=d_ids.data_ptr() + 4 * k0, cache=True, stream=s_)
            side.synchronize()
            if i >= args.warmup:
                out.append((time.perf_counter() - t0) * 1e3)
        return stats(out)

    res["tick_plain"] = ticks(False)
    res["tick_with_export64"] = ticks(True)
    res["tick_plain_again"] = ticks(False)
    big.close()
    line = json.dumps(res, indent=1)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
