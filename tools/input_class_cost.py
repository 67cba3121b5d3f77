#!/usr/bin/env python3
"""What input classes cost per step, in ONE process on ONE board (vapx_set_input_classes, csrc/input_classes.hip).  Legs run in
alternating blocks, the block order reversed every block, after a warm-up that fills the context window.

  --part a   a ONE-CLASS table against input_hz + input_format: three engines of the same shape - `table` (input_classes =
             [(format, rate)]), `uniform` (input_hz + input_format) and `unset` (fp32 at 16 kHz, no input kernel at all, whose spread
             between blocks is the noise a difference has to beat).  Since the engine has one input path these are two spellings of the
             SAME launch of input_classes_kernel: the table leg adds the slot descriptors the host builds and uploads per tick, the
             uniform leg computes its offsets in the kernel (profiles/input_classes holds the record of when `uniform` was two launches,
             a decoder and a resampler).  The second
             engine a process creates steps slower whatever it is (profiles/pcm_input/README.md), so a DISCARDED one-stream engine is
             created second and kept alive; --first names the leg created first.
  --part b   ONE mixed engine of S streams, split evenly over the classes, against one uniform engine of S / n streams per class,
             stepped back to back in the same process on the same audio; ms per tick of audio for both and the device memory each holds.

  --part c   a class per CHANNEL against a class per stream, same table, same bytes per tick: `split` (half the streams of --pair's first
             class, half of its second, set by vapx_set_stream_class: the path of before), `pair` (every stream (first, second), set by
             vapx_set_stream_channel_classes) and `unset`.  --tree DIR imports the package (and its library) from another checkout, e.g.
             the parent commit's, which has no `pair` leg; --first and the discarded second engine as in part a.

  device legs   audio already on the device: HIP events around each block of steps
  host legs     audio and output in page-locked host memory (the serving path): host clock around a step (a tick of part b's uniform
                side is the sum of its engines' steps)

Prints one JSON line, with the board's watts and shader clock during the timed blocks.

    python tools/input_class_cost.py --part a [--streams 4096] [--hz 20] [--ctx-sec 2.5] [--class mulaw@8000] [--first table]
    python tools/input_class_cost.py --part b [--classes f64@16000,mulaw@8000,s16@16000,s16@48000]
    python tools/input_class_cost.py --part c [--pair mulaw@8000+s16@48000] [--first pair] [--tree ../parent] [--kinds dev]
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
    ap.add_argument("--part", choices=["a", "b", "c"], required=True)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hz", type=int, default=20)
    ap.add_argument("--ctx-sec", type=float, default=2.5)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=4, help="timed blocks per leg")
    ap.add_argument("--steps", type=int, default=50, help="steps per block")
    ap.add_argument("--class", dest="cls", default="mulaw@8000", help="part a: the one class")
    ap.add_argument("--first", choices=["table", "uniform", "unset", "split", "pair"], default=None,
                    help="parts a and c: the leg whose engine is created first (default: table, split)")
    ap.add_argument("--pair", default="mulaw@8000+s16@48000", help="part c: the two classes")
    ap.add_argument("--tree", default=None, help="part c: import vap_realtime_amd from this checkout instead of the tool's own")
    ap.add_argument("--kinds", default="dev,host", help="which legs to time: dev, host or both")
    ap.add_argument("--classes", default="f64@16000,mulaw@8000,s16@16000,s16@48000", help="part b: the mix, evenly split")
    args = ap.parse_args()
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from vap_realtime_amd import engine, ingest, pcm, weights as W
    S, pool, hz = args.streams, 4, args.hz
    blob = W.pack_blob(*W.synthetic_weights(0, hz, "vap"), "vap")
    rng = np.random.default_rng(0)

    def held():                                            # device memory in use, MiB
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2.0 ** 20

    def make(n, **kw):
        before = held()
        e = engine.Engine(blob, hz, args.ctx_sec, max_streams=n, groups=args.groups, **kw)
        return e, round(held() - before, 1)

    def audio(cls, n):                                     # [pool][n][2][hop_in] samples of the class, page-locked, and their device copy
        f, r = cls
        host = engine.pinned_empty((pool, n, 2, r // hz), pcm.DTYPES[f])
        host[:] = pcm.encode(f, 0.05 * rng.standard_normal(host.shape)) if f != "f32" else 0.05 * rng.standard_normal(host.shape)
        return host, torch.from_numpy(np.array(host)).cuda()

    legs = {}                                              # name -> {"dev": fn(tick), "host": fn(tick), "mem": MiB, "bytes": input bytes per tick}
    keep = []
    if args.part == "a":
        cls = ingest.parse_input_class(args.cls)[0]
        f, r = cls
        first = args.first or "table"
        order = [first] + [x for x in ("table", "uniform", "unset") if x != first]
        for i, name in enumerate(order):
            kw = {"table": {"input_classes": [cls]}, "uniform": {"input_hz": r, "input_format": f}, "unset": {}}[name]
            e, mem = make(S, **kw)
            if i == 0:
                keep.append(make(1)[0])                    # the discarded second engine of the process
            c = ("f32", 16000) if name == "unset" else cls
            host, dev = audio(c, S)
            out_h, out_d = engine.pinned_empty((S, engine.OUT_STRIDE)), torch.empty((S, engine.OUT_STRIDE), device="cuda")
            ids = np.arange(S, dtype=np.int32)
            if name == "table":                            # the uniform block IS the packed block of a one-class table
                dfn = lambda t, e=e, dev=dev, out_d=out_d: e.step_packed_device(None, dev[t % pool].data_ptr(), out_d.data_ptr(), n=S)
                hfn = lambda t, e=e, host=host, out_h=out_h: e.step(host[t % pool].reshape(-1).view(np.uint8), ids, out=out_h)
            else:
                dfn = lambda t, e=e, dev=dev, out_d=out_d, c=c: e.step_device(S, dev[t % pool].data_ptr(), c[1] // hz, out_d.data_ptr())
                hfn = lambda t, e=e, host=host, out_h=out_h: e.step(host[t % pool], out=out_h)
            legs[name] = {"dev": dfn, "host": hfn, "mem": mem, "bytes": int(host[0].nbytes), "eng": [e]}
    elif args.part == "c":
        pair = [ingest.parse_input_class(t)[0] for t in args.pair.split("+")]
        assert len(pair) == 2 and pair[0] != pair[1] and S % 2 == 0, "--pair names two different classes, --streams is even"
        names_c = ["split", "pair", "unset"] if hasattr(engine.Engine, "set_stream_channel_classes") else ["split", "unset"]
        first = args.first or "split"
        assert first in names_c, f"--first {first}: this tree has the legs {names_c}"
        ids = np.arange(S, dtype=np.int32)
        for i, name in enumerate([first] + [x for x in names_c if x != first]):
            e, mem = make(S, **({} if name == "unset" else {"input_classes": pair}))
            if i == 0:
                keep.append(make(1)[0])                    # the discarded second engine of the process
            out_h, out_d = engine.pinned_empty((S, engine.OUT_STRIDE)), torch.empty((S, engine.OUT_STRIDE), device="cuda")
            if name == "unset":
                host, dev = audio(("f32", 16000), S)
                dfn = lambda t, e=e, dev=dev, out_d=out_d: e.step_device(S, dev[t % pool].data_ptr(), 16000 // hz, out_d.data_ptr())
                hfn = lambda t, e=e, host=host, out_h=out_h: e.step(host[t % pool], out=out_h)
                nbytes = int(host[0].nbytes)
            else:
                if name == "split":                        # S / 2 slots of [2][hop_in] of the first class, then S / 2 of the second
                    for s_ in range(S):
                        e.set_stream_class(s_, s_ // (S // 2))
                    parts = [audio(c, S // 2)[0] for c in pair]
                    rows = [np.concatenate([h[p_].reshape(-1).view(np.uint8) for h in parts]) for p_ in range(pool)]
                else:                                      # S slots of the first class's row, then the second's
                    for s_ in range(S):
                        e.set_stream_channel_classes(s_, 0, 1)
                    parts = [audio(c, S)[0][:, :, 0, :] for c in pair]
                    rows = [np.concatenate([np.ascontiguousarray(h[p_]).view(np.uint8).reshape(S, -1) for h in parts], axis=1).reshape(-1)
                            for p_ in range(pool)]
                nbytes = int(rows[0].size)
                packed_h = engine.pinned_empty((pool, nbytes), np.uint8)
                for p_ in range(pool):
                    packed_h[p_] = rows[p_]
                packed_d = torch.from_numpy(np.array(packed_h)).cuda()
                dfn = lambda t, e=e, d=packed_d, out_d=out_d: e.step_packed_device(ids, d[t % pool].data_ptr(), out_d.data_ptr())
                hfn = lambda t, e=e, h=packed_h, out_h=out_h: e.step(h[t % pool], ids, out=out_h)
            legs[name] = {"dev": dfn, "host": hfn, "mem": mem, "bytes": nbytes, "eng": [e]}
    else:
        classes = [ingest.parse_input_class(t)[0] for t in args.classes.split(",")]
        n_c = len(classes)
        per = S // n_c
        assert per * n_c == S, "--streams must divide evenly over the classes"
        mixed, mem = make(S, input_classes=classes)
        keep.append(make(1)[0])
        for s in range(S):
            mixed.set_stream_class(s, s // per)
        parts = [audio(c, per) for c in classes]          # the same audio for both sides
        nbytes = sum(int(h[0].nbytes) for h, _ in parts)
        packed_h = engine.pinned_empty((pool, nbytes), np.uint8)
        for p in range(pool):
            packed_h[p] = np.concatenate([h[p].reshape(-1).view(np.uint8) for h, _ in parts])
        packed_d = torch.from_numpy(np.array(packed_h)).cuda()
        ids = np.arange(S, dtype=np.int32)
        out_h, out_d = engine.pinned_empty((S, engine.OUT_STRIDE)), torch.empty((S, engine.OUT_STRIDE), device="cuda")
        legs["mixed"] = {"dev": lambda t: mixed.step_packed_device(ids, packed_d[t % pool].data_ptr(), out_d.data_ptr()),
                         "host": lambda t: mixed.step(packed_h[t % pool], ids, out=out_h), "mem": mem, "bytes": nbytes, "eng": [mixed]}
        uni, umem = [], 0.0
        for c in classes:
            e, m = make(per, **({} if c == ("f32", 16000) else {"input_hz": c[1], "input_format": c[0]}))
            uni.append(e)
            umem += m
        uo_h = [engine.pinned_empty((per, engine.OUT_STRIDE)) for _ in classes]
        uo_d = [torch.empty((per, engine.OUT_STRIDE), device="cuda") for _ in classes]

        def uni_dev(t):
            for e, c, (h, d), o in zip(uni, classes, parts, uo_d):
                e.step_device(per, d[t % pool].data_ptr(), c[1] // hz, o.data_ptr())

        def uni_host(t):
            for e, (h, d), o in zip(uni, parts, uo_h):
                e.step(h[t % pool], out=o)
        legs["uniform_x%d" % n_c] = {"dev": uni_dev, "host": uni_host, "mem": round(umem, 1), "bytes": nbytes, "eng": uni}
    names = list(legs)
    ticks = {n: 0 for n in names}

    def block(name, kind, n):
        fn = legs[name][kind]
        if kind == "dev":
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn(ticks[name])
                ticks[name] += 1
            b.record()
            b.synchronize()
            return [a.elapsed_time(b) / n] * n
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn(ticks[name])
            ms.append((time.perf_counter() - t0) * 1e3)
            ticks[name] += 1
        return ms

    T = int(args.ctx_sec * hz)
    for n in names:                                        # every window full, both paths warm
        block(n, "dev", T + 5)
        block(n, "host", 5)
    try:
        from bench import BoardWatch
        watch = BoardWatch()
    except Exception:                                      # noqa: BLE001 - no hwmon files: the numbers stand without them
        watch = None
    res = {"part": args.part, "streams": S, "frame_hz": hz, "ctx_frames": T, "overlap_groups": args.groups, "precision": "fp32",
           "timed_steps_per_leg": args.blocks * args.steps, "blocks": args.blocks, "creation_order": names,
           "second_engine_of_the_process": "a discarded 1-stream engine, kept alive"}
    if args.part == "a":
        res["class"] = args.cls
    elif args.part == "c":
        res["pair"], res["tree"] = args.pair, os.path.basename(os.path.abspath(args.tree)) if args.tree else "."
        res["library"] = os.path.relpath(os.path.realpath(engine.load_library()._name), os.path.realpath(args.tree or ROOT))
    else:
        res["classes"] = args.classes.split(",")
    for kind in [k for k in ("dev", "host") if k in args.kinds.split(",")]:
        blocks = {n: [] for n in names}
        with (watch if watch is not None else contextlib.nullcontext()):
            for b in range(args.blocks):
                for n in (names if b % 2 == 0 else names[::-1]):
                    blocks[n].append(block(n, kind, args.steps))
        out = {}
        for n in names:
            meds = [statistics.median(x) for x in blocks[n]]
            out[n] = {"ms_per_tick": round(statistics.median([v for x in blocks[n] for v in x]), 4), "block_medians_ms": [round(m, 4) for m in meds],
                      "block_spread_ms": round(max(meds) - min(meds), 4), "input_bytes_per_tick": legs[n]["bytes"], "device_memory_mib": legs[n]["mem"]}
        if args.part == "a":
            out["table_minus_uniform_ms"] = round(out["table"]["ms_per_tick"] - out["uniform"]["ms_per_tick"], 4)
            out["noise_unset_block_spread_ms"] = out["unset"]["block_spread_ms"]
        elif args.part == "c":
            for n in names:
                if n != "unset":
                    out[n + "_minus_unset_ms"] = round(out[n]["ms_per_tick"] - out["unset"]["ms_per_tick"], 4)
            out["noise_unset_block_spread_ms"] = out["unset"]["block_spread_ms"]
        else:
            out["mixed_over_uniform"] = round(out[names[0]]["ms_per_tick"] / out[names[1]]["ms_per_tick"], 4)
        if watch is not None:
            out["board"] = watch.record()
            watch = BoardWatch()
        res["device" if kind == "dev" else "host"] = out
    for L in legs.values():
        for e in L["eng"]:
            e.close()
    for e in keep:
        e.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
