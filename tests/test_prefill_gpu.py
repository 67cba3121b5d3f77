"""vapx_prefill on the GPU (include/vapx.h "Prefill"): the state it leaves against a twin engine stepped frame by frame and against the
float64 oracle, the continuation against the reference's golden rows and against the twin, what it must not touch, and its refusals.

Shapes: the golden cases vap20 (20 Hz, T = 50, n_cpc = 5, the short-window class) and vap50 (50 Hz, T = 250, n_cpc = 2), synth.dialogue_batch
audio as in tests/test_state_bulk_gpu.py.  Engines of 11 slots and max_batch = 8:
  three streams in slots [9, 2, 6]   6 LSTM rows (a partial 16-row workgroup), two frames per chunk (a remainder for odd counts)
  eight streams                      16 rows, one frame per chunk
  nine streams, max_batch = 11       18 rows (two workgroups, the second partial); floor(11 / 9) = 1 frame per chunk.  The engine refuses
                                     n > max_batch (vapx.h; test_refusals), so the nine-stream population has a scratch of its own size.

Test 1 holds engine A (stepped, existing code) and engine B (prefilled) against ``VapOracle(dtype=float64)`` driven by ``ServerFramer``
and ``advance`` and prints both errors per case (largest |value - float64| of ring, LSTM and Q|K|V cache rows: 2e-6 .. 8e-6 for either
engine; profiles/prefill/README.md has every figure measured on an MI355X).  The bar the feature was given is "B's error at most twice
A's".  Measured, B is BIT-IDENTICAL to A in all 108 cases, fp32 and split, and so are the ten ticks after it: every row meets the same
arithmetic in both engines - conv0 and the LSTM by construction, and every GEMM of these shapes takes the 32-row tile whatever its row
count (gemm_f32.hip: M < 12000), in which an element's sum runs over K in the same order wherever its row lies.  So the test asserts
equality of the whole records, which implies the bar; the errors against float64 stay in as printed figures and as a sanity bound.  An
engine whose virtual batch crosses a tile threshold that its step does not (thousands of streams) is promised agreement to rounding
only (vapx.h); tests/test_prefill_classes_gpu.py holds those engines - chunks of hundreds to 1840 entries - against float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import Case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_GOLDEN = 1e-4        # tests/test_engine_gpu.py
TOL_TWIN = 1e-5          # tests/test_state_bulk_gpu.py, a migrated stream
POPS = {3: ([9, 2, 6], 8), 8: ([10, 0, 3, 7, 1, 5, 8, 4], 8), 9: ([9, 2, 6, 0, 10, 4, 7, 1, 5], 11)}   # n -> (slots, max_batch)
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        from vap_realtime_amd import weights as W
        c = Case(name)
        _CACHE[name] = (c, W.pack_blob(c.cpc_sd, c.vap_sd, c.mode))
    return _CACHE[name]


def _audio(name):
    """[9, 2, hop * (T + 20)] seeded dialogue audio: every stream of every population reads its row from sample 0."""
    key = ("audio", name)
    if key not in _CACHE:
        from vap_realtime_amd import synth
        c, _ = _case(name)
        _CACHE[key] = synth.dialogue_batch(list(range(60, 69)), c.hop * (c.T + 20))
    return _CACHE[key]


def _engine(name, pop=3, split=False, **kw):
    from vap_realtime_amd import engine
    c, blob = _case(name)
    kw.setdefault("max_streams", 11)
    kw.setdefault("max_batch", POPS[pop][1])
    return engine.Engine(blob, c.frame_hz, c.ctx_sec, mode=c.mode, split_f16=split, **kw)


def _oracle(name):
    """float64 state after every frame count the cases need, all nine streams, computed once: {frames: (ring [9,2,n,256], h, c)}."""
    key = ("oracle", name)
    if key not in _CACHE:
        import torch
        from oracle.vap_oracle import ServerFramer, VapOracle
        c, _ = _case(name)
        o = VapOracle(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, dtype=torch.float64)
        st, fr = o.new_state(9), ServerFramer(9, c.hop)
        a, snaps = _audio(name), {}
        want = {1, 2, 3, 5, 8, c.T - 1, c.T, c.T + 7, c.T + 9}
        for f in range(max(want)):
            o.advance(fr.frame(a[:, :, f * c.hop:(f + 1) * c.hop]), st)
            if f + 1 in want:
                ring = torch.stack(st.ring, dim=2)                                     # [9, 2, n, 256] oldest -> newest
                v = o.v
                xn = torch.nn.functional.layer_norm(ring, (256,), v["ar_channel.layers.0.ln_self_attn.weight"],
                                                    v["ar_channel.layers.0.ln_self_attn.bias"], 1e-5)
                wqkv = torch.cat([v[f"ar_channel.layers.0.mha.{k}.weight"] for k in ("query", "key", "value")])
                snaps[f + 1] = (ring.numpy(), st.h.numpy().copy(), st.c.numpy().copy(), (xn @ wqkv.T).numpy())
        _CACHE[key] = snaps
    return _CACHE[key]


def _step_frames(eng, name, rows, slots, f0, f1):
    c, _ = _case(name)
    a, out = _audio(name), None
    for f in range(f0, f1):
        for i in range(0, len(rows), eng.max_batch):
            out = eng.step(a[rows[i:i + eng.max_batch], :, f * c.hop:(f + 1) * c.hop], slots[i:i + eng.max_batch])
    return out


def _block(name, rows, f0, f1):
    c, _ = _case(name)
    return np.ascontiguousarray(_audio(name)[rows, :, f0 * c.hop:f1 * c.hop])


def _cases(T):
    """(label, frames stepped first, reset queued before the prefill, frames prefilled); with a reset the audio restarts at frame 0."""
    return [(f"fresh_{F}", 0, False, F) for F in (1, 2, 3, T - 1, T, T + 7)] + [
        ("after_3_steps", 3, False, 5), ("after_T+4_steps", T + 4, False, 5), ("reset_queued", 3, True, 5)]


def _errors(eng_rec, snap, rows):
    """Largest |value - float64| of ring, lstm and cache rows of an engine's records against the oracle snapshot."""
    ring64, h64, c64, cache64 = snap
    n = ring64.shape[2]
    err = {"ring": 0.0, "lstm": 0.0, "cache": 0.0}
    for k, r in enumerate(rows):
        assert eng_rec["n_frames"][k] == n
        err["ring"] = max(err["ring"], float(np.abs(eng_rec["ring"][k][:, :n] - ring64[r]).max()))
        err["cache"] = max(err["cache"], float(np.abs(eng_rec["cache"][k][:, :n] - cache64[r]).max()))
        err["lstm"] = max(err["lstm"], float(np.abs(eng_rec["lstm"][k][:, 0] - h64[r]).max()), float(np.abs(eng_rec["lstm"][k][:, 1] - c64[r]).max()))
    return err


# ---- 1. state equals the stepped twin, 2b. and so does the continuation -------------------------------------------------------------
@pytest.mark.parametrize("pop", [3, 8, 9])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
@pytest.mark.parametrize("name", ["vap20", "vap50"])
def test_state_equals_the_stepped_twin_and_the_continuation_follows(name, split, pop):
    from vap_realtime_amd import engine
    c, _ = _case(name)
    T, slots = c.T, POPS[pop][0]
    rows = list(range(pop))
    snaps = _oracle(name)
    for label, pre, reset, F in _cases(T):
        A, B = _engine(name, pop, split), _engine(name, pop, split)
        for e in (A, B):
            _step_frames(e, name, rows, slots, 0, pre)
            if reset:
                for s in slots:
                    e.reset_stream(s)
        f0 = 0 if reset else pre
        _step_frames(A, name, rows, slots, f0, f0 + F)
        assert B.prefill(_block(name, rows, f0, f0 + F), slots) == F
        ra, rb = A.export_streams(slots, cache=True), B.export_streams(slots, cache=True)
        sa, sb = engine.split_state(ra, T), engine.split_state(rb, T)
        n = min(f0 + F, T)
        # header words, the window fill and the carry are equal; so is every ring slot that no frame wrote (records zero them)
        np.testing.assert_array_equal(rb[:, :8].view(np.int32), ra[:, :8].view(np.int32), err_msg=label)
        assert sb["n_frames"].tolist() == [n] * pop, label
        np.testing.assert_array_equal(sb["carry"], sa["carry"], err_msg=f"{label}: carry")
        np.testing.assert_array_equal(sb["ring"][:, :, n:], sa["ring"][:, :, n:])
        np.testing.assert_array_equal(sb["cache"][:, :, n:], sa["cache"][:, :, n:])
        for k, s in enumerate(slots):                                                  # the per-stream call sees the same
            ga, gb = A.get_state(s), B.get_state(s)
            assert ga["n_frames"] == gb["n_frames"] == n
            np.testing.assert_array_equal(gb["carry"], ga["carry"])
            np.testing.assert_array_equal(gb["ring"][:, :n], sb["ring"][k][:, :n])
            np.testing.assert_array_equal(gb["lstm"], sb["lstm"][k])
        ea, eb = _errors(sa, snaps[f0 + F], rows), _errors(sb, snaps[f0 + F], rows)
        same = np.array_equal(ra, rb)
        print("PREFILL_ERR " + json.dumps({"case": name, "path": "split" if split else "fp32", "streams": pop, "what": label,
                                           "stepped": ea, "prefilled": eb, "bit_identical": bool(same)}))
        for k in ea:
            assert eb[k] <= 2 * ea[k], f"{label} {k}: prefilled {eb[k]:.3e} against float64, stepped {ea[k]:.3e}"
            assert ea[k] < 1e-4, f"{label} {k}: the stepped engine itself is {ea[k]:.3e} from float64 - the oracle drive of this test is off"
        np.testing.assert_array_equal(rb, ra, err_msg=f"{label}: the prefilled records are not bit-identical to the stepped twin's")
        # ten further steps of both
        worst = 0.0
        for f in range(f0 + F, f0 + F + 10):
            oa, ob = _step_frames(A, name, rows, slots, f, f + 1), _step_frames(B, name, rows, slots, f, f + 1)
            np.testing.assert_array_equal(ob[:, engine.OUT_NVALID], oa[:, engine.OUT_NVALID], err_msg=f"{label} tick {f}")
            da, db = engine.split_outputs(oa), engine.split_outputs(ob)
            for key in ("p_now", "p_future", "vad", "logits", "e"):
                worst = max(worst, float(np.abs(da[key] - db[key]).max()))
                np.testing.assert_allclose(db[key], da[key], rtol=0, atol=TOL_TWIN, err_msg=f"{label} tick {f} {key}")
        print(f"PREFILL_CONT {name} {'split' if split else 'fp32'} n={pop} {label}: worst |stepped - prefilled| over 10 ticks = {worst:.3e}")
        A.close(); B.close()


# ---- 2a. the continuation is the reference's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,F,split", [("vap20", 53, False), ("vap20", 53, True), ("vap50", 200, False), ("vap50", 200, True)],
                         ids=["vap20-fp32", "vap20-split", "vap50-fp32", "vap50-split"])
def test_continuation_matches_the_reference_golden(name, F, split):
    from vap_realtime_amd import engine
    c, blob = _case(name)
    assert c.framing == "server" and F < c.n_frames and (name != "vap20" or F == c.T + 3)
    eng = engine.Engine(blob, c.frame_hz, c.ctx_sec, max_streams=len(c.streams), mode=c.mode, split_f16=split)
    assert eng.prefill(np.ascontiguousarray(c.audio[:, :, :F * c.hop])) == F
    z, worst = c.z, {}
    es = int(z["meta.e_stride"]) if "meta.e_stride" in z.files else 1
    for f in range(F, c.n_frames):
        o = engine.split_outputs(eng.step(c.new_samples(f)))
        assert np.all(o["n"] == min(f + 1, c.T))
        for k in ("p_now", "p_future", "vad", "logits"):
            worst[k] = max(worst.get(k, 0.0), float(np.abs(o[k] - z[k][f]).max()))
        if f % es == 0:
            worst["e"] = max(worst.get("e", 0.0), float(np.abs(o["e"] - z["e"][f // es]).max()))
    print("PREFILL_GOLDEN", name, "split" if split else "fp32", worst)
    for k, v in worst.items():
        assert v <= TOL_GOLDEN, (name, k, v)
    eng.close()


# ---- 3. nothing else moves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vap20", "vap50"])
def test_unnamed_streams_are_untouched_and_every_route_agrees(name):
    """Every slot holds state (stepped 4 frames); streams [9, 2, 6] are prefilled T + 2 frames (17 chunks at vap20: the ring wraps inside
    the call).  The records of the other eight slots are bit-identical before and after; pageable, page-locked and device audio, each
    between margins of one NaN pattern, leave the same records as plain pageable audio, and the margins stay."""
    import torch
    import memory_bounds as mb
    from vap_realtime_amd import engine
    c, _ = _case(name)
    slots, rows, F = POPS[3][0], [0, 1, 2], c.T + 2
    others = [s for s in range(11) if s not in slots]
    block = _block(name, rows, 4, 4 + F)
    words, margin = block.size, mb.MARGIN_BYTES // 4

    def populated():
        e = _engine(name)
        a = _audio(name)
        for f in range(4):
            e.step(a[:8, :, f * c.hop:(f + 1) * c.hop], list(range(8)))
            e.step(a[[8, 0, 1], :, f * c.hop:(f + 1) * c.hop], [8, 9, 10])
        return e

    def host_margins(buf):
        buf.view(np.uint32)[:] = mb.PATTERN
        inner = buf[margin:margin + words].reshape(block.shape)
        inner[...] = block
        assert inner.ctypes.data % 16 == 0
        return inner

    results = {}
    for route in ("plain", "pageable", "pinned", "device"):
        e = populated()
        before = e.export_streams(others, cache=True)
        if route == "plain":
            e.prefill(block, slots)
        elif route == "device":
            g = mb.Guarded.of(block, what=f"{name} prefill audio")
            ids = mb.Guarded.of(np.array(slots, np.int32), what="prefill ids")
            e.prefill_device(3, g.ptr(), F, ids_ptr=ids.ptr(), stream=torch.cuda.current_stream().cuda_stream)
            g.check(); ids.check()
        else:
            if route == "pinned":
                buf = engine.pinned_empty((words + 2 * margin,))
            else:
                buf = engine.aligned_bytes(4 * (words + 2 * margin)).view(np.float32)
            e.prefill(host_margins(buf), slots)
            mb.check_words(buf, words, what=f"{name} {route} prefill audio")
        np.testing.assert_array_equal(e.export_streams(others, cache=True), before, err_msg=f"{route}: an unnamed stream moved")
        results[route] = e.export_streams(slots, cache=True)
        assert engine.split_state(results[route], c.T)["n_frames"].tolist() == [c.T] * 3
        e.close()
    for route in ("pageable", "pinned", "device"):
        np.testing.assert_array_equal(results[route], results["plain"], err_msg=f"{route} audio against plain pageable audio")


def test_engine_buffers_keep_their_canaries():
    """A child process under VAPX_GUARD_ZONES=1 (the library reads the variable once): prefills over every route and both chunk shapes,
    then ``guard_violations`` must be 0 and ``guard_selftest`` 1 (tests/prefill_guard.py)."""
    env = dict(os.environ, VAPX_GUARD_ZONES="1")
    p = subprocess.run([sys.executable, os.path.join(HERE, "prefill_guard.py")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["guard_selftest"] == 1 and got["guard_violations"] == 0, got
    assert got["launches"]["conv0"] > 0 and got["launches"]["lstm"] > 0 and got["launches"]["gather_ln"] > 0, got
    assert got["routes_agree"] is True, got


def test_prefill_launches_per_chunk_not_per_frame():
    """Three streams, max_batch 8, 57 frames at T = 50: 29 chunks of two frames (the last of one).  One conv0, one LSTM launch per chunk; the
    first three chunks (frames 0 .. 5, all overwritten by frames 50 .. 56) skip the Q|K|V GEMM and the ring fill."""
    e = _engine("vap20")
    e.profile_enable(range(16))
    e.prefill(_block("vap20", [0, 1, 2], 0, 57), POPS[3][0])
    got = {k: v[1] for k, v in e.profile_read().items()}
    from vap_realtime_amd.engine import prefill_chunks
    plan = prefill_chunks(8, 3, 57, 50)
    assert len(plan) == 29 and sum(fills for _, _, fills in plan) == 26
    assert got["conv0"] == 29 and got["lstm"] == 29 and got["gather_ln"] == 26, got
    assert not set(got) & {"attention", "ffn_block", "last_row", "head", "ffn_proj", "gemm_resid", "gemm_resid_ln", "gemm_gelu"}, got
    e.close()


def test_a_history_given_in_several_calls_is_the_history_given_in_one():
    """A prefill starts from the stream's carry and frame counter, so a long history may be split over ticks: 3 + 20 + 34 frames (the ring
    wraps inside the third call) leave the records of one call of 57, bit for bit."""
    one, parts = _engine("vap20"), _engine("vap20")
    slots, rows = POPS[3][0], [0, 1, 2]
    one.prefill(_block("vap20", rows, 0, 57), slots)
    for f0, f1 in ((0, 3), (3, 23), (23, 57)):
        parts.prefill(_block("vap20", rows, f0, f1), slots)
    np.testing.assert_array_equal(parts.export_streams(slots, cache=True), one.export_streams(slots, cache=True))
    one.close(); parts.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def _refused(eng, code, call, match):
    from vap_realtime_amd import engine
    before = eng.export_streams()
    rc = call()
    msg = eng.lib.vapx_last_error(eng._h).decode()
    assert rc == code, (rc, msg)
    assert match in msg and "\n" not in msg, msg
    np.testing.assert_array_equal(eng.export_streams(), before, err_msg=f"a refused call changed state: {msg}")


def test_refusals():
    from vap_realtime_amd import engine
    c, blob = _case("vap20")
    a = _block("vap20", [0, 1, 2], 0, 3)
    E_INVAL, E_RANGE = -1, -4

    def raw(eng, n, ids, audio_ptr, frames, flags=0):
        idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
        return lambda: eng.lib.vapx_prefill(eng._h, n, None if idp is None else idp.ctypes.data, audio_ptr, frames, flags, None)

    eng = _engine("vap20", max_streams=11, max_batch=2)
    eng.step(a[:2, :, :c.hop], [3, 4])                                                 # some state a refused call could damage
    _refused(eng, E_INVAL, raw(eng, 3, [9, 2, 6], a.ctypes.data, 3), "max_batch")
    _refused(eng, E_INVAL, raw(eng, 2, [9, 9], a.ctypes.data, 3), "twice")
    _refused(eng, E_RANGE, raw(eng, 2, [9, 11], a.ctypes.data, 3), "out of range")
    _refused(eng, E_INVAL, raw(eng, 2, [9, 2], a.ctypes.data, 0), "frames")
    _refused(eng, E_INVAL, raw(eng, 2, [9, 2], a.ctypes.data + 4, 2), "16-byte aligned")
    _refused(eng, E_RANGE, raw(eng, 0, None, a.ctypes.data, 3), "n=0")
    eng.close()

    for kw, match in (({"input_hz": 8000}, "input rate"), ({"input_format": "s16"}, "input format"),
                      ({"input_classes": [("f32", 16000), ("mulaw", 8000)]}, "input-class table")):
        eng = engine.Engine(blob, c.frame_hz, c.ctx_sec, max_streams=4, mode=c.mode, **kw)
        rc = raw(eng, 2, [0, 1], a.ctypes.data, 2)()
        msg = eng.lib.vapx_last_error(eng._h).decode()
        assert rc == E_INVAL and match in msg and "\n" not in msg, (kw, rc, msg)
        if "input_classes" not in kw:                                                   # an engine with a table has no state records
            before = eng.export_streams()
            assert raw(eng, 2, [0, 1], a.ctypes.data, 2)() == E_INVAL
            np.testing.assert_array_equal(eng.export_streams(), before)
        eng.close()

    lead = engine.Engine(blob, c.frame_hz, c.ctx_sec, max_streams=4, mode=c.mode)
    fol = engine.Engine(blob, c.frame_hz, c.ctx_sec, max_streams=4, mode=c.mode)
    fol.attach_trunk(lead)
    _refused(lead, E_INVAL, raw(lead, 2, [0, 1], a.ctypes.data, 2), "trunk leader")
    _refused(fol, E_INVAL, raw(fol, 2, [0, 1], a.ctypes.data, 2), "trunk follower")
    with pytest.raises(engine.VapxError, match="trunk leader"):
        lead.prefill(a[:2], [0, 1])
    fol.close(); lead.close()


def test_many_stream_vap_prefill_then_process():
    from vap_realtime_amd.realtime import ManyStreamVAP
    c, _ = _case("vap20")
    a = _audio("vap20")
    m = ManyStreamVAP(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, n_streams=4, mode=c.mode)
    twin = ManyStreamVAP(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, n_streams=4, mode=c.mode)
    assert m.prefill(a[:2, :, :6 * c.hop], [3, 1]) == 6
    for f in range(6):
        twin.process(a[:2, :, f * c.hop:(f + 1) * c.hop], [3, 1])
    ra, rb = twin.process(a[:2, :, 6 * c.hop:7 * c.hop], [3, 1]), m.process(a[:2, :, 6 * c.hop:7 * c.hop], [3, 1])
    assert rb["n"].tolist() == [7, 7]
    for k in ("p_now", "p_future", "vad"):
        np.testing.assert_allclose(rb[k], ra[k], rtol=0, atol=TOL_TWIN)
    # a torch CUDA tensor takes the device route (read in place, on torch's current stream): the same records as the host route
    import torch
    dev = ManyStreamVAP(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, n_streams=4, mode=c.mode)
    assert dev.prefill(torch.from_numpy(np.ascontiguousarray(a[:2, :, :6 * c.hop])).cuda(), [3, 1]) == 6
    dev.process(a[:2, :, 6 * c.hop:7 * c.hop], [3, 1])
    np.testing.assert_array_equal(dev.engine.export_streams(cache=True), m.engine.export_streams(cache=True))
    for x in (m, twin, dev):
        x.engine.close()
