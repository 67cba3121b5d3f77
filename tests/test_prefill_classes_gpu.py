"""vapx_prefill against float64 in the dispatch classes production engines use (cases, plan and checker: tests/prefill_classes.py; the
CPU proof of that checker: tests/test_prefill_classes.py).

    case  Hz  path          n (distinct)  max_batch  frames              entries per chunk   there for
    A     20  fp32, split   1 (1)         512        300                 300                 fused tail with conv1 in 64-row tiles; fc > T;
                                                                                             1500 LSTM steps in one launch
    B     20  fp32          3 (3)         1024       360                 1023, then 57       GEMM chain, conv1..3 64-row, conv4 / gx 32-row; a
                                                                                             fused chunk after a chain chunk; the chunk boundary
    C     20  fp32, split   8 (3)         1840       230                 1840 = max_batch    conv1 128-row (M = 206080), conv2..4 64-row, gx
                                                                                             128-row; scratch and staging filled to the last entry
    E     50  fp32, split   1 (1)         512        500                 500                 n_cpc = 2, 1000 LSTM steps
    F     10  fp32, split   2 (2)         128        64                  128                 n_cpc = 10: no fused tail at this rate
    G      5  fp32          1 (1)         64         40                  40                  n_cpc = 20: the downsample ring wraps over 20 steps
    H     20  fp32          3 (3)         1024       5 stepped, 200, 150 600; 450            a ring that holds frames and a non-zero first slot;
                                                                                             a second call continuing the first; a stepped twin

Per case: every stream's record (ring rows, Q|K|V cache rows, LSTM h and c at the encoder-stage bound; carry bit for bit; n_frames; zero
rows beyond the fill) after every call, the launch counts of the call, every entry of the last chunk's h0, h1, z, e (h2, h3 where the
chain ran; refusals elsewhere), and three ordinary steps at 1e-4.  Cases A, C and F also take pageable host audio, which must leave the
records of device audio bit for bit.  The figures measured on an MI355X are in profiles/prefill/README.md."""
import json
import time

import numpy as np
import pytest

import prefill_classes as PC

pytestmark = pytest.mark.gpu

_TRUTH: dict = {}
_BLOB: dict = {}
PARAMS = [(c.id, path) for c in PC.CASES.values() for path in c.paths]


def truth(hz):
    """Both oracles over a rate's dialogues, once for every case and path of that rate."""
    if hz not in _TRUTH:
        t0 = time.time()
        _TRUTH[hz] = PC.Truth(hz, [c for c in PC.CASES.values() if c.hz == hz])
        print(f"PREFILL_CLASSES oracle {hz} Hz: {time.time() - t0:.1f} s on the CPU, {len(_TRUTH[hz].stages)} stage blocks")
    return _TRUTH[hz]


def make_engine(case, path):
    from vap_realtime_amd import engine, weights as W
    tr = truth(case.hz)
    if case.hz not in _BLOB:
        _BLOB[case.hz] = W.pack_blob(tr.cpc, tr.vap, "vap")
    eng = engine.Engine(_BLOB[case.hz], case.hz, case.ctx_sec, max_streams=PC.population(case)[2], max_batch=case.max_batch,
                        split_f16=path == "split")
    assert eng.T == case.T
    return eng


def report(case, path, route, what, res, seconds):
    print("PREFILL_CLASSES " + json.dumps({"case": case.id, "path": path, "route": route, "what": what, "seconds": round(seconds, 2),
                                           "continuation": float(f"{res['cont']:.3e}"),
                                           "err/E32": {k: round(f["err/E32"], 2) for k, f in res["figures"].items()},
                                           "err/bound": {k: round(f["err/bound"], 3) for k, f in res["figures"].items()},
                                           "E32": {k: float(f"{f['E32']:.2e}") for k, f in res["figures"].items() if "E32" in f}}))


def test_the_cases_cover_every_class():
    PC.check_coverage(list(PC.CASES.values()))


@pytest.mark.parametrize("cid,path", PARAMS, ids=[f"{c}-{p}" for c, p in PARAMS])
def test_prefilled_state_against_float64(cid, path):
    import torch
    case = PC.CASES[cid]
    tr = truth(case.hz)
    eng = make_engine(case, path)
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        res = PC.run_case(eng, case, path, tr)
        report(case, path, "device", "prefilled", res, time.time() - t0)
    finally:
        eng.close()
    want = {"ring", "cache", "h", "c", "h0", "h1", "z", "e"}
    assert want <= set(res["figures"]), sorted(res["figures"])
    if cid == "C" or case.hz in (10, 5) or path == "split":                                # the chain ran on the last chunk: h2 / h3 were looked at
        assert {"h2", "h3"} <= set(res["figures"]), sorted(res["figures"])


@pytest.mark.parametrize("cid", [c.id for c in PC.CASES.values() if "pageable" in c.routes])
def test_pageable_audio_leaves_the_records_of_device_audio(cid):
    """Chunks of 128 to 1840 entries through the pinned staging block: held against float64 like the device route, and bit-identical to it."""
    case = PC.CASES[cid]
    tr = truth(case.hz)
    recs = {}
    for route in ("device", "pageable"):
        eng = make_engine(case, "fp32")
        try:
            t0 = time.time()
            res = PC.run_case(eng, case, "fp32", tr, route=route, stages=False)
            recs[route] = (res["records"], eng.export_streams(cache=True))
            if route == "pageable":
                report(case, "fp32", route, "prefilled", res, time.time() - t0)
        finally:
            eng.close()
    np.testing.assert_array_equal(recs["pageable"][0], recs["device"][0], err_msg=f"case {cid}: the records after the call")
    np.testing.assert_array_equal(recs["pageable"][1], recs["device"][1], err_msg=f"case {cid}: every slot's record after three further steps")


def test_case_H_next_to_a_stepped_twin():
    """A plain engine of the same size stepped over H's 355 frames: its records under the same checker, prefilled and stepped err / E32 side
    by side.  The twin says what hundreds of frames of the step's own arithmetic cost; the prefill has to stay inside the bound whatever
    the twin does, and a prefill outside it next to a twin inside it is a wrong prefill."""
    case = PC.CASES["H"]
    tr = truth(case.hz)
    slots, owner, _ = PC.population(case)
    audio = tr.audio[owner]
    figs = {}
    for what in ("prefilled", "stepped"):
        eng = make_engine(case, "fp32")
        try:
            if what == "prefilled":
                res = PC.run_case(eng, case, "fp32", tr, stages=False)
                figs[what] = res["figures"]
            else:
                seen, f = 0, {}
                for op, k in case.program:
                    for g in range(seen, seen + k):
                        eng.step(audio[:, :, g * case.hop:(g + 1) * case.hop], slots)
                    seen += k
                    if op == "prefill":
                        PC.check_state(eng, case, tr, slots, owner, seen, "H fp32 stepped twin", f)
                figs[what] = f
        finally:
            eng.close()
    for field in ("ring", "cache", "h", "c"):
        p, s = figs["prefilled"][field], figs["stepped"][field]
        print(f"PREFILL_CLASSES H {field}: err / E32 prefilled {p['err/E32']:.2f} stepped {s['err/E32']:.2f}; err / bound prefilled "
              f"{p['err/bound']:.3f} stepped {s['err/bound']:.3f}; E32 {p['E32']:.2e}")
        assert p["err/bound"] <= 1.0 and s["err/bound"] <= 1.0


def test_peek_after_a_prefill_is_the_last_chunk_until_the_next_step():
    """Five steps of three streams, then a prefill of 7 frames of two others (chunks of 4 and 3 frames at max_batch 8): ``e`` is the last
    chunk's six entries and never the step's three; lstm_out and the transformer's buffers are refused with the reason; a step of one stream
    gives every buffer back, one entry long."""
    from vap_realtime_amd import engine, weights as W
    case = PC.CASES["A"]
    tr = truth(20)
    if 20 not in _BLOB:
        _BLOB[20] = W.pack_blob(tr.cpc, tr.vap, "vap")
    eng = engine.Engine(_BLOB[20], 20, case.ctx_sec, max_streams=8, max_batch=8)
    hop, a = 800, tr.audio
    try:
        for f in range(5):
            eng.step(a[:3, :, f * hop:(f + 1) * hop], [0, 1, 2])
        assert eng.peek("lstm_out", (3, 2, 5, 256)).shape == (3, 2, 5, 256)
        eng.prefill(np.ascontiguousarray(a[:2, :, :7 * hop]), [4, 5])
        e = eng.peek("e", (6, 2, 1, 256))                                                  # V = 2 streams x 3 frames, frame-major
        ring = engine.split_state(eng.export_streams([4, 5], cache=True), case.T)["ring"]  # [2, 2, T, 256], rows 0 .. 6 = frames 0 .. 6
        for v in range(6):
            j, k = v // 2, v % 2
            np.testing.assert_array_equal(e[v, :, 0], ring[k][:, 4 + j], err_msg=f"entry {v}: frame {4 + j} of stream {k}")
        for name in ("h2", "h3"):
            with pytest.raises(engine.VapxError, match="fused conv tail"):
                eng.peek(name, (6, 2, 30, 256))
        for name in PC.REFUSED + ("stereo2", "x0"):
            with pytest.raises(engine.VapxError, match="not written by vapx_prefill"):
                eng.peek(name, (1,))
        eng.step(a[:1, :, 5 * hop:6 * hop], [0])
        assert eng.peek("lstm_out", (1, 2, 5, 256)).shape == (1, 2, 5, 256) and eng.peek("e", (1, 2, 1, 256)).shape == (1, 2, 1, 256)
    finally:
        eng.close()
