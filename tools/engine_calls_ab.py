#!/usr/bin/env python3
"""Two builds of libvapx.so in one process: the same bits and the same speed?

    python tools/engine_calls_ab.py <parent.so> <new.so> [--pairs 5] [--iters 100] [--out record.json]

1. One seeded program through each build - host and device steps at 1, 8 and 64 streams, a prefill of 40 entries, export and import of
   64 streams with and without the Q|K|V cache, a two-model vapx_step_group - and every output block and every exported record must be
   bit-identical.  Then the per-stream state calls (state_program): on an fp32 and a split engine at T = 50 and T = 70, an 8 kHz engine, a
   two-class engine and a vap 20 Hz + nod 10 Hz trunk group, four streams with window fills 0, 3, T and T + 7: every vapx_get_state
   array, then vapx_set_state into a fresh engine, its vapx_export_streams with the cache (vapx_get_state where the bulk calls are
   refused) and three more ticks (four in the group).
2. The two builds timed alternately, `--pairs` pairs per leg (a sample is the median of `--iters` calls, of `--iters` / 5 for the two
   bulk legs): the host-inclusive step at 1, 8 and 64 streams ending in a synchronise (what tools/latency_small_batches.py measures),
   export + import of 64 streams through pageable memory, the prefill, and vapx_get_state + vapx_set_state over 64 streams.  Gate per leg: median(new) <= median(parent) + (max(parent)
   - min(parent)).  A leg whose parent samples disagree by more than the two medians differ says so: lengthen it (--iters) and repeat.

Both builds export the same symbols, and a build calls some of its own functions (the vapx_engine constructor among them) through the
PLT: opened the plain way, the second build would run the first one's constructor on its own, differently laid out engine.  So each is
opened RTLD_DEEPBIND first - its own definitions win - and only then handed to engine.load_library(path) for the prototypes."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the libraries: one HIP runtime in the process)
from vap_realtime_amd import engine, synth, weights as W  # noqa: E402

HZ, CTX, HOP = 20, 2.5, 800


def open_build(path):
    path = os.path.abspath(path)
    ctypes.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    return engine.load_library(path)


class Build:
    """Engines of one build: `engine.Engine` takes the library `load_library()` returns, so that is switched around every construction."""

    def __init__(self, name, lib):
        self.name, self.lib = name, lib
        cpc, vap = W.synthetic_weights(0, HZ, "vap")
        self.blob = W.pack_blob(cpc, vap)
        self.blobs = {m: W.pack_blob(*W.synthetic_weights(0, HZ, m), m) for m in ("vap", "bc")}

    def make(self, ctor, *a, **kw):
        engine._lib = self.lib
        obj = ctor(*a, **kw)
        assert (obj.leader if hasattr(obj, "leader") else obj).lib is self.lib
        return obj

    def engine(self, S, **kw):
        return self.make(engine.Engine, self.blob, HZ, CTX, max_streams=S, **kw)


def program(b):
    """The seeded program; returns {name: array}."""
    res = {}
    for S in (1, 8, 64):
        audio = synth.noise_batch(S, HOP * 6, seed=20 + S)
        eng = b.engine(S, groups=2)
        res[f"host{S}"] = np.stack([eng.step(audio[:, :, t * HOP:(t + 1) * HOP]).copy() for t in range(6)])
        d_audio = torch.from_numpy(audio).cuda()
        d_out = torch.zeros(6, S, engine.OUT_STRIDE, device="cuda")
        for t in range(6):
            blk = d_audio[:, :, t * HOP:(t + 1) * HOP].contiguous()
            eng.step_device(S, blk.data_ptr(), HOP, d_out[t].data_ptr())
        torch.cuda.synchronize()
        res[f"device{S}"] = d_out.cpu().numpy()
        if S == 64:
            eng.reset_stream(5)
            eng.prefill(synth.noise_batch(8, HOP * 5, seed=31), np.arange(8, 16))   # 8 streams x 5 frames: one chunk of 40 entries
            for cache in (False, True):
                rec = eng.export_streams(cache=cache)
                res[f"export_cache{int(cache)}"] = rec
                other = b.engine(S)
                other.import_streams(None, rec, cache)
                res[f"import_cache{int(cache)}_step"] = other.step(audio[:, :, :HOP]).copy()
                res[f"import_cache{int(cache)}_export"] = other.export_streams(cache=True)
                other.close()
        eng.close()
    grp = b.make(engine.TrunkGroup, b.blobs, HZ, {"vap": CTX, "bc": 5.0}, max_streams=8)
    audio = synth.noise_batch(8, HOP * 4, seed=40)
    for t in range(4):
        wire = grp.step_wire(audio[:, :, t * HOP:(t + 1) * HOP])
        for m, rows in wire.items():
            res[f"group_{m}_{t}"] = rows.copy()
    grp.close()
    return res


def state_program(b):
    """vapx_get_state / vapx_set_state on every kind of engine that moves state through them; returns {name: array}."""
    res = {}
    cpc20 = W.synthetic_weights(0, HZ, "vap")[0]
    nod10 = W.pack_blob(cpc20, W.synthetic_weights(0, 10, "nod")[1], "nod")
    rng = np.random.default_rng(77)
    mulaw = rng.integers(0, 256, (4, 2, 400 * 80), dtype=np.uint8)
    wide, narrow = synth.noise_batch(4, HOP * 80, seed=51), synth.noise_batch(4, 400 * 80, seed=52)

    def plain(T, **kw):
        return lambda: b.make(engine.Engine, b.blob, HZ, T / HZ, max_streams=4, **kw)

    def classes2():
        e = plain(50, input_classes=[("f32", 16000), ("mulaw", 8000)])()
        for s in (1, 3):
            e.set_stream_class(s, 1)
        return e

    def group():
        return b.make(engine.TrunkGroup, {"vap": b.blobs["vap"], "nod": nod10}, {"vap": 20, "nod": 10}, {"vap": 2.5, "nod": 3.0}, max_streams=4)

    hop16 = lambda t, ids: wide[ids, :, t * HOP:(t + 1) * HOP]
    kinds = {f"{name}_T{T}": (plain(T, split_f16=name == "split"), T, hop16) for T in (50, 70) for name in ("fp32", "split")}
    kinds["in8k_T50"] = (plain(50, input_hz=8000), 50, lambda t, ids: narrow[ids, :, t * 400:(t + 1) * 400])
    kinds["classes2_T50"] = (classes2, 50, lambda t, ids: [(mulaw[s, :, t * 400:(t + 1) * 400] if s % 2 else wide[s, :, t * HOP:(t + 1) * HOP]).copy()
                                                           for s in ids])
    kinds["follow_20_10"] = (group, 50, hop16)
    for kind, (make, T, block) in kinds.items():
        fills = [0, 3, T, T + 7]
        engines = lambda o: list(o.engines.items()) if isinstance(o, engine.TrunkGroup) else [("", o)]
        src = make()
        for t in range(T + 7):
            ids = [s for s in range(4) if t >= T + 7 - fills[s]]
            if ids:
                src.step(block(t, ids), ids)
        dst = make()
        grouped = isinstance(dst, engine.TrunkGroup)
        for (m, a), (_, d) in zip(engines(src), engines(dst)):
            got = []
            for s in range(4):
                st = a.get_state(s)
                got += [np.float32([st["n_frames"]])] + [st[k].ravel() for k in ("ring", "lstm", "carry") if st[k] is not None]
                d.set_state(s, st)
            res[f"{kind}{m}_get"] = np.concatenate(got)
            bulk = not d.input_classes and not (grouped and dst.R[m] > 1)       # else vapx_export_streams is refused
            res[f"{kind}{m}_after_set"] = d.export_streams(cache=True) if bulk else np.concatenate([d.get_state(s)["ring"].ravel() for s in range(4)])
        ticks = []
        for t in range(T + 7, T + 7 + (4 if grouped else 3)):
            o = dst.step(block(t, [0, 1, 2, 3]), [0, 1, 2, 3])
            ticks.append({m: o[m].copy() for m in o} if grouped else {"": o.copy()})
        for m in ticks[0]:
            res[f"{kind}{m}_ticks"] = np.stack([o[m] for o in ticks])
        src.close(); dst.close()
    return res


def stepper(eng, audio):
    """One host step per call, walking the eight hops of `audio` round and round."""
    k = [0]

    def step():
        t = k[0] % 8
        k[0] += 1
        eng.step(audio[:, :, t * HOP:(t + 1) * HOP])
    return step


def legs(b, iters):
    """{leg: callable() -> median ms of one call} on engines of build `b` that live as long as the run."""
    out, keep = {}, []

    def median_ms(call, n):
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    for S in (1, 8, 64):
        eng = b.engine(S)
        audio = synth.noise_batch(S, HOP * 8)
        step = stepper(eng, audio)
        for _ in range(60):
            step()
        out[f"step_{S}"] = lambda step=step: median_ms(step, iters)
        keep.append(eng)
    eng = keep[-1]
    rec = np.empty((64, eng.state_floats()), np.float32)                          # pageable
    out["export_import_64"] = lambda: median_ms(lambda: eng.import_streams(None, eng.export_streams(out=rec), False), max(iters // 5, 5))
    history, ids = synth.noise_batch(8, HOP * 5, seed=31), np.arange(8, 16)
    out["prefill_40"] = lambda: median_ms(lambda: eng.prefill(history, ids), max(iters // 5, 5))

    def get_set_64():
        for s in range(64):
            eng.set_state(s, eng.get_state(s))
    out["get_set_state_64"] = lambda: median_ms(get_set_64, max(iters // 5, 5))
    return out, keep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.pairs >= 5, "at least five pairs per leg"
    builds = [Build("parent", open_build(args.parent)), Build("new", open_build(args.new))]

    got = [{**program(b), **state_program(b)} for b in builds]
    assert sorted(got[0]) == sorted(got[1])
    differ = [k for k in sorted(got[0]) if got[0][k].shape != got[1][k].shape or got[0][k].tobytes() != got[1][k].tobytes()]
    dead = [k for k in sorted(got[0]) if not np.isfinite(got[0][k]).all() or not np.abs(got[0][k]).max() > 0]
    print(f"bit-identity: {len(got[0])} blocks, {sum(v.size for v in got[0].values())} floats, differing: {differ or 'none'}, "
          f"non-finite or all-zero: {dead or 'none'}", flush=True)

    timed = [legs(b, args.iters) for b in builds]
    samples = {leg: {b.name: [] for b in builds} for leg in timed[0][0]}
    for leg in samples:
        for p in range(args.pairs):
            for b, (calls, _) in zip(builds, timed):
                ms = calls[leg]()
                samples[leg][b.name].append(ms)
                print(f"raw {leg} pair {p} {b.name} {ms:.4f} ms", flush=True)
    failed = []
    print(f"{'leg':<18}{'parent median':>14}{'parent spread':>14}{'new median':>12}{'bound':>10}  verdict")
    for leg, s in samples.items():
        pm, nm, spread = float(np.median(s["parent"])), float(np.median(s["new"])), max(s["parent"]) - min(s["parent"])
        ok = nm <= pm + spread
        noisy = spread > abs(nm - pm)
        if not ok:
            failed.append(leg)
        print(f"{leg:<18}{pm:>14.4f}{spread:>14.4f}{nm:>12.4f}{pm + spread:>10.4f}  {'pass' if ok else 'FAIL'}"
              f"{' (parent spread exceeds the difference of the medians)' if noisy else ''}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"blocks": len(got[0]), "differing": differ, "dead": dead, "samples": samples, "failed": failed,
                       "pairs": args.pairs, "iters": args.iters}, f, indent=1)
    for _, keep in timed:
        for e in keep:
            e.close()
    if differ or dead or failed:
        sys.exit(f"engine_calls_ab: differing blocks {differ}, dead blocks {dead}, legs over the gate {failed}")


if __name__ == "__main__":
    main()
