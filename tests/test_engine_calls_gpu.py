"""The order every engine call runs in (csrc/engine.hip: argument checks, enter, settle), the one record of the latest pass
(engine_buffers.h PassRecord) and the one rule for queued resets in a trunk group, on the GPU.

No reference and no tolerance: every expected value is a twin engine's that took the same state-changing calls without the call under
test, compared bit for bit.  The shape is the smallest that forks: 20 Hz, T = 8, 66 slots, 64 streams in two overlap groups of 32."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HZ, T, HOP, L, SLOTS, N = 20, 8, 800, 1120, 66, 64
AUDIO_DEVICE, OUT_DEVICE, DEFER_JOIN = 1, 2, 8
_CACHE = {}


def _blob(mode="vap"):
    if mode not in _CACHE:
        from vap_realtime_amd import weights as W
        cpc, vap = W.synthetic_weights(0, HZ, mode)
        _CACHE[mode] = W.pack_blob(cpc, vap, mode)
    return _CACHE[mode]


def _engine(mode="vap", frames=T, **kw):
    from vap_realtime_amd import engine
    eng = engine.Engine(_blob(mode), HZ, frames / HZ, max_streams=SLOTS, max_batch=N, mode=mode, groups=2, **kw)
    assert eng.T == frames
    return eng


def _ticks(n_ticks, seed=3):
    """[n_ticks] device blocks [N, 2, HOP] of seeded noise."""
    import torch
    from vap_realtime_amd import synth
    a = synth.noise_batch(N, HOP * n_ticks, seed=seed)
    return [torch.from_numpy(np.ascontiguousarray(a[:, :, t * HOP:(t + 1) * HOP])).cuda() for t in range(n_ticks)]


def _ids(*ids):
    return np.asarray(ids, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _refused(eng, rc, code, text):
    assert rc == code, (rc, eng.lib.vapx_last_error(eng._h))
    assert text in eng.lib.vapx_last_error(eng._h).decode()


# the refused calls: (name, call(engine, device scratch, stream) -> rc, error code, words of the error text)
def _refusals():
    dup = np.arange(N, dtype=np.int32)
    dup[40] = 7                                             # stream 7 in batch slots 7 and 40
    far = np.arange(N, dtype=np.int32)
    far[3] = SLOTS                                          # one past the last slot
    two = _ids(3, 3)
    step = lambda e, d, s, ids, out: e.lib.vapx_step(e._h, N, _ptr(ids), d["audio"].data_ptr(), HOP, out, AUDIO_DEVICE | OUT_DEVICE, s)
    return [
        ("step_duplicate_id", lambda e, d, s: step(e, d, s, dup, d["out"].data_ptr()), -1, "stream id 7 appears twice in one call (batch slot 40)"),
        ("step_id_out_of_range", lambda e, d, s: step(e, d, s, far, d["out"].data_ptr()), -4, f"stream id {SLOTS} out of range [0,{SLOTS})"),
        ("step_null_out", lambda e, d, s: step(e, d, s, np.arange(N, dtype=np.int32), None), -1, "null out"),
        ("prefill_duplicate_id", lambda e, d, s: e.lib.vapx_prefill(e._h, 2, _ptr(two), d["audio"].data_ptr(), 1, AUDIO_DEVICE, s), -1,
         "stream id 3 appears twice in one call (batch slot 1)"),
        ("encode_audio_duplicate_id", lambda e, d, s: e.lib.vapx_encode_audio(e._h, 2, _ptr(two), d["frames"].data_ptr(), d["e"].data_ptr(), s), -1,
         "stream id 3 appears twice in one call (batch slot 1)"),
        ("export_duplicate_id", lambda e, d, s: e.lib.vapx_export_streams(e._h, 2, _ptr(two), d["rec"].data_ptr(), OUT_DEVICE, s), -1,
         "stream id 3 appears twice in one call (batch slot 1)"),
    ]


@pytest.mark.parametrize("case", _refusals(), ids=lambda c: c[0])
def test_refused_call_leaves_no_trace(case):
    """A reset queued on stream 5 and a deferred tick in flight; then a call that is refused for its arguments.  The next step and an
    export of every stream are bit-identical to a twin's that never made the refused call, and stream 5 reports one valid frame: the
    refused call neither applied nor lost the queued reset."""
    import torch
    from vap_realtime_amd import engine
    _, call, code, text = case
    audio = _ticks(2)
    side = torch.cuda.Stream()
    got = {}
    for who in ("refused", "twin"):
        eng = _engine()
        d = {"audio": audio[1], "out": torch.zeros(N, engine.OUT_STRIDE, device="cuda"), "frames": torch.zeros(2, 2, L, device="cuda"),
             "e": torch.zeros(2, 2, 256, device="cuda"), "rec": torch.zeros(2, eng.state_floats(), device="cuda")}
        out = torch.zeros(N, engine.OUT_STRIDE, device="cuda")
        rec = torch.zeros(SLOTS, eng.state_floats(True), device="cuda")
        torch.cuda.synchronize()
        eng.step_device(N, audio[0].data_ptr(), HOP, out.data_ptr(), stream=side.cuda_stream, defer_join=True)
        eng.reset_stream(5)
        if who == "refused":
            _refused(eng, call(eng, d, side.cuda_stream), code, text)
        eng.step_device(N, audio[1].data_ptr(), HOP, out.data_ptr(), stream=side.cuda_stream, defer_join=True)
        eng.export_streams_device(SLOTS, rec.data_ptr(), cache=True, stream=side.cuda_stream)
        side.synchronize()
        got[who] = (out.cpu().numpy(), rec.cpu().numpy())
        eng.close()
    rows = got["twin"][0]
    assert rows[5, engine.OUT_NVALID] == 1 and (np.delete(rows[:, engine.OUT_NVALID], 5) == 2).all() and np.isfinite(rows).all()
    np.testing.assert_array_equal(got["refused"][0], rows)
    np.testing.assert_array_equal(got["refused"][1], got["twin"][1])


# ---- the pass record ------------------------------------------------------------------------------------------------------------------
def _program(eng, upto, peeks):
    """The state-changing calls 0 .. upto of the pass-record program on `eng`; after call k, the peeks `peeks` names for k.
    Returns {(k, name): array}."""
    import torch
    from vap_realtime_amd import synth
    audio = synth.noise_batch(N, HOP * 2, seed=5)
    frames = torch.from_numpy(synth.noise_batch(3, L, seed=6)).cuda()
    e_out = torch.zeros(3, 2, 256, device="cuda")
    history = synth.noise_batch(2, HOP * 5, seed=7)
    P2 = 28                                                 # positions after conv2 at 20 Hz (engine_buffers.h geometry)
    shapes = {"e": lambda n: (n, 2, 256), "h2": lambda n: (n, 2, P2 + 2, 256), "o": lambda n: (n, 2, T, 256)}
    calls = [
        (N, lambda: eng.step(audio[:, :, :HOP])),                                                 # 0: a step in two groups
        (3, lambda: eng.encode_audio_device(3, frames.data_ptr(), e_out.data_ptr(), _ids(10, 64, 65))),   # 1: leaves `groups`
        (10, lambda: eng.prefill(history, _ids(64, 65))),                                         # 2: one chunk of 5 frames x 2 streams
        (N, lambda: eng.step(audio[:, :, HOP:])),                                                 # 3
    ]
    got = {}
    for k, (entries, call) in enumerate(calls[:upto + 1]):
        call()
        for name in peeks.get(k, ()):
            got[(k, name)] = eng.peek(name, shapes[name](entries))
    return got


def test_pass_record_follows_the_calls():
    """step (two groups), encode_audio (n = 3), peek "e" and "h2", prefill, peek "e", a refused "lstm_out", step, peek "o": every
    accepted peek has the latest pass's entries and equals the peek of a twin that made the same state-changing calls and no other
    peek; every refusal carries its text.  (VAPX_FLAG_UNFUSED_CONV: "h2" exists.)"""
    from vap_realtime_amd import engine
    eng = _engine(unfused_conv=True)
    peeks = {1: ("e", "h2"), 2: ("e",), 3: ("o",)}
    lib, buf = eng.lib, np.zeros(16, np.float32)

    def refusal(name, text):
        assert lib.vapx_peek(eng._h, name.encode(), _ptr(buf), buf.size) == -1
        assert text in lib.vapx_last_error(eng._h).decode(), lib.vapx_last_error(eng._h)

    got = _program(eng, 2, peeks)
    refusal("lstm_out", '"lstm_out" is not written by vapx_prefill (its LSTM launch keeps lstm_out to itself and no transformer layer runs): '
            'after a prefill only h0 .. h3, z and e of its last chunk exist; step to peek "lstm_out"')
    refusal("o", '"o" is not written by vapx_prefill')
    import torch
    from vap_realtime_amd import synth
    out = eng.step(synth.noise_batch(N, HOP * 2, seed=5)[:, :, HOP:])
    got[(3, "o")] = eng.peek("o", (N, 2, T, 256))
    refusal("x0", '"x0" is read straight from the ring; create the engine with VAPX_FLAG_MATERIALIZE_X0 to peek it')
    refusal("stereo2", '"stereo2" is only materialised with VAPX_FLAG_FULL_LAST_LAYER (default: last layer runs on the newest row only)')
    refusal("comb", '"comb" is only materialised in nod mode (vap / bc: the combinator of the newest row stays inside head_kernel)')
    refusal("qkv", "unknown buffer 'qkv'")
    assert np.isfinite(out).all() and out[10, engine.OUT_NVALID] == 2 and out[0, engine.OUT_NVALID] == 2
    eng.close()
    assert sorted(got) == [(1, "e"), (1, "h2"), (2, "e"), (3, "o")]
    for (k, name), a in got.items():
        twin = _engine(unfused_conv=True)
        want = _program(twin, k, {k: (name,)})[(k, name)]
        twin.close()
        assert np.isfinite(a).all() and np.abs(a).max() > 0, (k, name)
        np.testing.assert_array_equal(a, want, err_msg=f"peek {name!r} after call {k}")
    torch.cuda.synchronize()


def test_fused_tail_and_two_groups_in_the_record():
    """The default engine runs the fused conv tail: "h2" is refused after a step and after an encode_audio; the nod variant's "comb" is
    refused after a step in two groups."""
    from vap_realtime_amd import synth
    buf = np.zeros(16, np.float32)
    eng = _engine()
    eng.step(synth.noise_batch(N, HOP, seed=5))
    assert eng.lib.vapx_peek(eng._h, b"h2", _ptr(buf), buf.size) == -1
    assert '"h2" stays in LDS in the fused conv tail; create the engine with VAPX_FLAG_UNFUSED_CONV to peek it' in eng.lib.vapx_last_error(eng._h).decode()
    assert eng.peek("h1", (N, 2, 56 + 2, 256)).any()
    eng.close()
    nod = _engine("nod")
    nod.step(synth.noise_batch(N, HOP, seed=5))
    assert nod.lib.vapx_peek(nod._h, b"comb", _ptr(buf), buf.size) == -1
    assert ('"comb" is not contiguous when the latest step ran in 2 overlap groups; step with groups = 1 to peek it'
            in nod.lib.vapx_last_error(nod._h).decode())
    nod.step(synth.noise_batch(8, HOP, seed=5))             # 8 streams: one group
    assert nod.peek("comb", (8, T, 256)).any()
    nod.close()


# ---- queued resets in a trunk group -----------------------------------------------------------------------------------------------------
def test_leader_step_with_a_reset_waits_for_a_deferred_follower():
    """A leader (T = 8) and a same-rate follower (T = 12) stepped device-resident on one stream, the follower with VAPX_DEFER_JOIN; a
    reset of stream 5 is queued between ticks.  Four ticks: both models' rows (n_valid among them) are bit-identical to a twin group's
    stepped without deferral."""
    import torch
    from vap_realtime_amd import engine
    ticks = 4
    audio = _ticks(ticks, seed=9)
    side = torch.cuda.Stream()
    got = {}
    for defer in (True, False):
        lead, fol = _engine("vap", T), _engine("bc", 12)
        fol.attach_trunk(lead)
        outs = [[torch.zeros(N, engine.OUT_STRIDE, device="cuda") for _ in range(ticks)] for _ in range(2)]
        torch.cuda.synchronize()
        for t in range(ticks):
            if t == 2:
                lead.reset_stream(5)
            lead.step_device(N, audio[t].data_ptr(), HOP, outs[0][t].data_ptr(), stream=side.cuda_stream)
            rc = fol.lib.vapx_step(fol._h, N, None, None, 0, outs[1][t].data_ptr(), OUT_DEVICE | (DEFER_JOIN if defer else 0), side.cuda_stream)
            assert rc == 0, fol.lib.vapx_last_error(fol._h)
        fol.join(side.cuda_stream)
        side.synchronize()
        got[defer] = [[o.cpu().numpy() for o in model] for model in outs]
        fol.close(); lead.close()
    for m, window in enumerate((T, 12)):
        for t in range(ticks):
            want = got[False][m][t]
            n_valid = np.full(N, min(t + 1, window))
            n_valid[5] = t + 1 if t < 2 else t - 1
            np.testing.assert_array_equal(want[:, engine.OUT_NVALID], n_valid, err_msg=f"model {m}, tick {t}")
            assert np.isfinite(want).all()
            np.testing.assert_array_equal(got[True][m][t], want, err_msg=f"model {m}, tick {t}")
