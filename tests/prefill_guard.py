"""Child process of tests/test_prefill_gpu.py::test_engine_buffers_keep_their_canaries: vapx_prefill under VAPX_GUARD_ZONES=1 (4 KiB
canaries round every device allocation of the engine; the library reads the variable once per process, hence a child).  Prefills that fill
the scratch to its last entry (n * frames_in_chunk = max_batch), leave a remainder chunk, wrap the ring inside the call and name the
engine's last slot, over pageable, page-locked and device audio; then the large-chunk shapes of tests/prefill_classes.py (cases C and G);
prints one JSON line."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import memory_bounds as mb   # noqa: E402  (puts the repository root on the path)


def main() -> int:
    import torch
    from vap_realtime_amd import engine
    assert os.environ.get("VAPX_GUARD_ZONES"), "run with VAPX_GUARD_ZONES=1"
    rng = np.random.default_rng(11)
    run, agree = mb.Run(), True
    for hz, T, split in ((20, 6, False), (50, 9, True)):
        hop = 16000 // hz
        for n, slots, frames in ((4, [10, 0, 5, 3], 2 * T + 3), (3, [10, 1, 6], T + 2), (8, [10, 0, 1, 2, 3, 4, 5, 6], 3)):
            block = mb.noise(rng, (n, 2, frames * hop))
            recs = []
            for route in ("pageable", "pinned", "device"):
                e = run.engine(mb.blob(hz), hz, mb.ctx_sec(T, hz), max_streams=11, max_batch=8, split_f16=split)
                e.step(mb.noise(np.random.default_rng(3), (2, 2, hop)), [10, 0])   # the last slot holds a carry and a ring position of 1
                if route == "device":
                    g, gi = mb.Guarded.of(block, what="prefill audio"), mb.Guarded.of(np.array(slots, np.int32), what="prefill ids")
                    e.prefill_device(n, g.ptr(), frames, ids_ptr=gi.ptr(), stream=torch.cuda.current_stream().cuda_stream)
                    g.check(); gi.check()
                else:
                    src = block
                    if route == "pinned":
                        src = engine.pinned_empty(block.shape)
                        src[...] = block
                    e.prefill(src, slots)
                out = e.step(mb.noise(np.random.default_rng(5), (n, 2, hop)), slots)
                run.finite(out, f"{hz} Hz n={n} {route}")
                recs.append(e.export_streams(cache=True))
            agree = agree and all(np.array_equal(r, recs[0]) for r in recs[1:])
    # the chunk shapes of tests/prefill_classes.py: case C (8 streams x 230 frames = 1840 entries = max_batch exactly: the GEMM chain with
    # conv1 in 128-row tiles, every scratch buffer and the audio staging filled to the last entry; device and pageable audio) and case G
    # (5 Hz, 40 frames of one stream in one chunk: the largest per-entry buffers)
    for hz, T, n, max_batch, frames, routes in ((20, 12, 8, 1840, 230, ("device", "pageable")), (5, 4, 1, 64, 40, ("device",))):
        hop = 16000 // hz
        slots = [n + 2, 0, 5, 3, 1, 7, 9, 4][:n]
        block = mb.noise(rng, (n, 2, frames * hop))
        recs = []
        for route in routes:
            e = run.engine(mb.blob(hz), hz, mb.ctx_sec(T, hz), max_streams=max(max_batch, n + 3), max_batch=max_batch)
            e.step(mb.noise(np.random.default_rng(3), (1, 2, hop)), [n + 2])               # the last slot holds a carry and a ring position of 1
            if route == "device":
                g, gi = mb.Guarded.of(block, what="prefill audio"), mb.Guarded.of(np.array(slots, np.int32), what="prefill ids")
                e.prefill_device(n, g.ptr(), frames, ids_ptr=gi.ptr(), stream=torch.cuda.current_stream().cuda_stream)
                g.check(); gi.check()
            else:
                e.prefill(block, slots)
            run.finite(e.step(mb.noise(np.random.default_rng(5), (n, 2, hop)), slots), f"{hz} Hz n={n} max_batch={max_batch} {route}")
            recs.append(e.export_streams(cache=True))
        agree = agree and all(np.array_equal(r, recs[0]) for r in recs[1:])
    selftest = float(run.live[0].peek("guard_selftest", (1,))[0])
    run.close()
    print(json.dumps({"guard_selftest": selftest, "guard_violations": run.violations, "launches": run.launches, "routes_agree": agree}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
