"""Input at 8 / 32 / 48 kHz on the GPU (vapx_set_input_rate, vapx_resample; csrc/resample.hip).

The whole-signal kernel is held against float64; everything else is bit-equality between an engine with an input rate and a 16 kHz
engine that is fed z, the delayed whole-signal resample of the same audio, under the SAME batches, ids and resets — so the only
difference between the two is where the 16 kHz samples come from.  Synthetic weights (the filter does not care), ctx_frames = 8 so that
the window fills and slides within a dozen frames."""
import ctypes as C
import socket
import struct
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = {8000: (1, 2, 7, 15), 32000: (2, 1, 13, 28), 48000: (3, 1, 19, 41)}      # orig, new, width, K
_CACHE = {}


def _blob(frame_hz, mode="vap"):
    key = ("blob", frame_hz, mode)
    if key not in _CACHE:
        from vap_realtime_amd import weights as W
        _CACHE[key] = W.pack_blob(*W.synthetic_weights(0, frame_hz, mode), mode)
    return _CACHE[key]


def _signal(hz, n, rows=3, seed=0, amp=1.0):
    """[rows, 2, n] float32: seeded noise in [-amp, amp] plus a 300 Hz sine of that amplitude."""
    rng = np.random.default_rng(1000 * seed + hz)
    t = np.arange(n) / hz
    x = rng.uniform(-1, 1, (rows, 2, n)) + np.sin(2 * np.pi * 300.0 * t + rng.uniform(0, 6, (rows, 2, 1)))
    return (amp * x).astype(np.float32)


def _resample_gpu(hz, x, guard=0):
    """vapx_resample of x [rows, n_in] (float32) -> [rows, n_out]; with ``guard`` the floats behind the output are returned too."""
    import torch
    from vap_realtime_amd import engine
    lib = engine.load_library()
    orig, new, _, _ = RATES[hz]
    rows, n_in = x.shape
    n_out = -(-new * n_in // orig)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full((rows * n_out + guard,), 7.0, dtype=torch.float32, device="cuda")
    assert lib.vapx_resample(hz, rows, n_in, xd.data_ptr(), yd.data_ptr(), None) == 0
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    return (y[:rows * n_out].reshape(rows, n_out), y[rows * n_out:]) if guard else y.reshape(rows, n_out)


def _z(hz, x, n_out):
    """The 16 kHz stream an engine at ``hz`` feeds its model for the whole signal x [..., n_in]: the GPU's Y, delayed, zeros in front."""
    from vap_realtime_amd import resample
    flat = x.reshape(-1, x.shape[-1])
    return resample.delayed(_resample_gpu(hz, flat), hz, n_out).reshape(x.shape[:-1] + (n_out,))


def _engine(frame_hz, input_hz=16000, max_streams=3, mode="vap", ctx_frames=8, **kw):
    from vap_realtime_amd import engine
    return engine.Engine(_blob(frame_hz, mode), frame_hz, (ctx_frames + 0.5) / frame_hz, max_streams=max_streams, mode=mode,
                         input_hz=input_hz, **kw)


# ---- 1. the kernel against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hz", sorted(RATES))
def test_whole_signal_kernel_against_float64(hz):
    from vap_realtime_amd import resample
    orig, new, width, K = RATES[hz]
    h = resample.taps(hz)
    for n_in in sorted({1, max(orig - 1, 1), width, 1000, 1001}):
        x = _signal(hz, n_in, rows=3, seed=n_in)[:, 0]
        y, guard = _resample_gpu(hz, x, guard=64)
        want = resample.whole_ref(x.astype(np.float64), hz)                # float64 with the fp32-rounded taps
        assert y.shape == want.shape == (3, -(-new * n_in // orig))
        assert np.all(guard == 7.0), "the kernel wrote past ceil(new * n_in / orig) outputs"
        # K fused multiply-adds, each rounding once to fp32: K * 2^-24 relative to the largest sum of magnitudes an output can have
        bound = K * 2.0 ** -24 * np.abs(h).sum(axis=1).max() * np.abs(x).max()
        err = np.abs(y.astype(np.float64) - want).max()
        print(f"{hz} Hz n_in {n_in}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (hz, n_in, err, bound)


# ---- 2. streaming equals whole-signal, bit for bit ---------------------------------------------------------------------------------
def _run_rate(hz, frame_hz, frames, x, **kw):
    """Engine with input rate ``hz`` stepped ``frames`` ticks on x [S, 2, frames * hop_in]: list of output blocks."""
    eng = _engine(frame_hz, hz, max_streams=x.shape[0], **kw)
    hop_in = hz // frame_hz
    assert eng.hop_in == hop_in and eng.lib.vapx_get_input_rate(eng._h) == hz
    outs = [eng.step(x[:, :, t * hop_in:(t + 1) * hop_in]).copy() for t in range(frames)]
    eng.close()
    return outs


@pytest.mark.parametrize("hz,frame_hz,frames,split", [(8000, 20, 14, False), (48000, 50, 12, False), (32000, 10, 10, False), (8000, 20, 14, True)],
                         ids=["8k_20hz", "48k_50hz", "32k_10hz", "8k_20hz_split"])
def test_streaming_equals_whole_signal_bit_for_bit(hz, frame_hz, frames, split):
    hop_in, hop = hz // frame_hz, 16000 // frame_hz
    x = _signal(hz, frames * hop_in, rows=3, seed=1, amp=0.1)
    got = _run_rate(hz, frame_hz, frames, x, split_f16=split)
    z = _z(hz, x, frames * hop)
    new, d = RATES[hz][1], 7
    assert not z[..., :new * d].any() and z[..., new * d:new * d + 8].any()
    b = _engine(frame_hz, max_streams=3, split_f16=split)
    assert b.lib.vapx_get_input_rate(b._h) == 16000
    for t in range(frames):
        want = b.step(z[:, :, t * hop:(t + 1) * hop])
        assert np.array_equal(got[t], want), f"frame {t}: {np.abs(got[t] - want).max()}"
    assert got[-1][0, 10] == 8.0 and np.abs(got[-1][:, :6]).max() > 0          # the window filled and slid; the rows are not empty
    b.close()


# ---- 3. ragged and permuted batches, resets ----------------------------------------------------------------------------------------
def test_ragged_permuted_batches_and_resets():
    hz, frame_hz, frames = 8000, 20, 12
    hop_in, hop = hz // frame_hz, 16000 // frame_hz
    slots = [4, 1, 6]                                                       # stream k lives in slot slots[k] of a 7-slot engine
    x = _signal(hz, frames * hop_in, rows=3, seed=3, amp=0.1)
    start = {0: 0, 1: 0, 2: 4}                                              # stream 2 joins at frame 4
    resets = {6: (0, "carry"), 7: (1, "stream")}
    # every stream's own stand-alone z: the whole-signal resample of each SEGMENT between its join / resets (a reset starts a new signal)
    z = np.zeros((3, 2, frames * hop), np.float32)
    for k in range(3):
        cuts = [start[k]] + [f for f, (s, _) in sorted(resets.items()) if s == k] + [frames]
        for f0, f1 in zip(cuts[:-1], cuts[1:]):
            z[k, :, f0 * hop:f1 * hop] = _z(hz, x[k, :, f0 * hop_in:f1 * hop_in], (f1 - f0) * hop)
    a, b = _engine(frame_hz, hz, max_streams=7), _engine(frame_hz, max_streams=7)
    rng = np.random.default_rng(5)
    for f in range(frames):
        if f in resets:
            s, kind = resets[f]
            for e in (a, b):
                (e.reset_carry if kind == "carry" else e.reset_stream)(slots[s])
        members = [k for k in range(3) if f >= start[k]]
        order = [members[i] for i in rng.permutation(len(members))]         # ids permuted every tick
        ids = [slots[k] for k in order]
        got = a.step(x[order, :, f * hop_in:(f + 1) * hop_in], ids)
        want = b.step(z[order, :, f * hop:(f + 1) * hop], ids)
        assert np.array_equal(got, want), f"frame {f}, order {order}: {np.abs(got - want).max()}"
    a.close()
    b.close()


# ---- 4. trunk group ----------------------------------------------------------------------------------------------------------------
def test_trunk_group_with_an_input_rate_on_the_leader():
    from vap_realtime_amd import engine
    hz, ticks = 8000, 12
    blobs = {"vap": _blob(20, "vap"), "nod": _blob(10, "nod")}
    ctx = {"vap": 8.5 / 20, "nod": 6.5 / 10}
    ga = engine.TrunkGroup(blobs, {"vap": 20, "nod": 10}, ctx, max_streams=2, input_hz=hz)
    gb = engine.TrunkGroup(blobs, {"vap": 20, "nod": 10}, ctx, max_streams=2)
    assert ga.order == ["vap", "nod"] and ga.T_of == {"vap": 8, "nod": 6} and (ga.hop_in, ga.hop, gb.hop_in) == (400, 800, 800)
    assert ga.leader.lib.vapx_get_input_rate(ga.engines["nod"]._h) == 16000
    x = _signal(hz, ticks * 400, rows=2, seed=4, amp=0.1)
    z = _z(hz, x, ticks * 800)
    for t in range(ticks):
        got = ga.step_wire(x[:, :, t * 400:(t + 1) * 400])
        want = gb.step_wire(z[:, :, t * 800:(t + 1) * 800])
        for m in ("vap", "nod"):
            assert np.array_equal(got[m], want[m]), (t, m)
    assert (got["nod"][:, engine.OUT_STATUS] == 0).all() and got["nod"][0, engine.OUT_NVALID] == 6      # tick 12: nod's 6th frame
    lib = ga.leader.lib
    assert lib.vapx_set_input_rate(ga.engines["nod"]._h, 8000) == -1 and b"leader" in lib.vapx_last_error(ga.engines["nod"]._h)
    assert lib.vapx_set_input_rate(ga.leader._h, 32000) == -1 and b"before its first step" in lib.vapx_last_error(ga.leader._h)
    assert lib.vapx_set_input_rate(gb.leader._h, 8000) == -1 and b"before its first step" in lib.vapx_last_error(gb.leader._h)
    with pytest.raises(engine.VapxError, match="samples_per_ch must be 400"):
        ga.step_wire(z[:, :, :800])
    ga.close()
    gb.close()


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------
def test_state_records_carry_the_history():
    from vap_realtime_amd import engine
    hz, frame_hz, T = 8000, 20, 8
    x = _signal(hz, 14 * 400, rows=3, seed=5, amp=0.1)
    a = _engine(frame_hz, hz)
    for t in range(10):
        a.step(x[:, :, t * 400:(t + 1) * 400])
    assert a.state_floats() == engine.state_record_floats(T, input_hz=hz) == 8 + 1664 + 28 + 2 * T * 256
    assert a.state_floats(True) == engine.state_record_floats(T, True, input_hz=hz)
    rec = a.export_streams(cache=True)
    s = engine.split_state(rec, T, input_hz=hz)
    assert s["bits"].tolist() == [engine.STATE_HAS_LSTM | engine.STATE_HAS_CACHE | engine.STATE_HAS_RESAMPLE] * 3
    assert s["input_hz"].tolist() == [hz] * 3 and s["resample_started"].tolist() == [3] * 3
    np.testing.assert_array_equal(s["resample_hist"], x[:, :, 10 * 400 - 14:10 * 400])      # the last H = 14 input samples
    b = _engine(frame_hz, hz)
    b.import_streams(None, rec, cache=True)
    for t in range(10, 14):                                                  # the next 4 frames: bit-identical to the uninterrupted engine
        hop = x[:, :, t * 400:(t + 1) * 400]
        assert np.array_equal(b.step(hop), a.step(hop)), t
    # a fresh stream's record says so: its first d blocks stay silent after the move as well
    c = _engine(frame_hz, hz)
    fresh = engine.split_state(c.export_streams([1]), T, input_hz=hz)
    assert fresh["resample_started"].tolist() == [0] and not fresh["resample_hist"].any()
    # those records do not go into an engine without a rate (nor the reverse); the field is named and no stream changes
    plain = _engine(frame_hz)
    before = plain.export_streams(cache=True)
    with pytest.raises(engine.VapxError, match="record length"):
        plain.import_streams(None, rec, cache=True)
    rc = plain.lib.vapx_import_streams(plain._h, 3, None, rec.ctypes.data_as(C.c_void_p), engine.STATE_CACHE, None)
    assert rc == -1 and b"input_hz 8000" in plain.lib.vapx_last_error(plain._h)
    pad = np.zeros((3, a.state_floats(True)), np.float32)
    pad[:, :before.shape[1]] = before
    rc = b.lib.vapx_import_streams(b._h, 3, None, pad.ctypes.data_as(C.c_void_p), engine.STATE_CACHE, None)
    assert rc == -1 and b"input_hz 16000" in b.lib.vapx_last_error(b._h)
    np.testing.assert_array_equal(plain.export_streams(cache=True), before)
    # a 16 kHz engine's records are what they were: size, content bits, and header words [6], [7] zero — with 16000 "set" as well
    same = _engine(frame_hz, 16000)
    assert same.lib.vapx_set_input_rate(same._h, 16000) == 0
    for e in (plain, same):
        assert e.state_floats() == 8 + 1664 + 2 * T * 256 and e.state_floats(True) == e.state_floats() + 2 * T * 768
        hd = e.export_streams()[:, :8].view(np.int32)
        assert hd[:, 3].tolist() == [engine.STATE_HAS_LSTM] * 3 and not hd[:, 6:8].any()
    # set_state has no place for the history: it zeroes it, the stream's input continues as a new signal
    st = a.get_state(2)
    a.set_state(2, st)
    after = engine.split_state(a.export_streams([2]), T, input_hz=hz)
    assert after["resample_started"].tolist() == [0] and not after["resample_hist"].any()
    np.testing.assert_array_equal(after["carry"][0], st["carry"])
    for e in (a, b, c, plain, same):
        e.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    from vap_realtime_amd import engine
    with pytest.raises(engine.VapxError, match="44100"):
        _engine(20, 44100)
    e = _engine(20)
    for bad in (44100, 22050, 11025, 0, -8000):
        assert e.lib.vapx_set_input_rate(e._h, bad) == -1
    assert e.lib.vapx_set_input_rate(e._h, 8000) == 0 and e.lib.vapx_get_input_rate(e._h) == 8000
    assert e.lib.vapx_set_input_rate(e._h, 32000) == -1                      # once
    e.close()
    e = _engine(20, 8000)
    for spc in (800, 400 + 320, 800 + 320, 399):                             # hop, hop_in + carry, a full 16 kHz frame, a short hop
        with pytest.raises(engine.VapxError, match="samples_per_ch must be 400"):
            e.step(np.zeros((3, 2, spc), np.float32))
    frames = torch.zeros((3, 2, 1120), device="cuda")
    emb = torch.zeros((3, 2, 256), device="cuda")
    with pytest.raises(engine.VapxError, match="input rate is 8000"):
        e.encode_audio_device(3, frames.data_ptr(), emb.data_ptr())
    out = e.step(np.zeros((3, 2, 400), np.float32))                          # none of the refusals touched the engine
    assert out[0, engine.OUT_NVALID] == 1 and np.isfinite(out).all()
    lib = e.lib
    assert lib.vapx_resample(44100, 1, 10, frames.data_ptr(), emb.data_ptr(), None) == -1
    assert lib.vapx_resample(8000, 0, 10, frames.data_ptr(), emb.data_ptr(), None) == -1
    assert lib.vapx_resample(8000, 1, 0, frames.data_ptr(), emb.data_ptr(), None) == -1
    assert lib.vapx_resample(8000, 1, 10, None, emb.data_ptr(), None) == -1
    e.close()
    from vap_realtime_amd.server import ManyStreamServer

    class Vap:                                                               # the Python twin of the front-end frames 16 kHz only
        hop, hop_in, n_streams, mode = 800, 400, 1, "vap"

        def process(self, new, ids=None):
            raise AssertionError
    with pytest.raises(ValueError, match="16 kHz"):
        ManyStreamServer(Vap(), port_in=0, port_out=0)


# ---- 7. the native front-end -------------------------------------------------------------------------------------------------------
def _read_packet(sock):
    sock.settimeout(20)
    buf = b""
    while len(buf) < 4:
        buf += sock.recv(4 - len(buf))
    ln = struct.unpack("<I", buf)[0]
    payload = b""
    while len(payload) < ln:
        payload += sock.recv(ln - len(payload))
    return payload


def test_front_end_frames_by_the_input_rate():
    """Two dialogues on a 2-stream engine whose max_batch is 1, so that every tick of the front-end steps ONE stream, as the stand-alone
    reference engine does: which rows share a batch is then not left to the timing of two receive threads (an output row's last bit
    depends on the shape of its batch in the kernels behind the resampler; both engines of the other tests see identical batches)."""
    from vap_realtime_amd import engine, ingest, wire
    hz, frame_hz, frames, hop_in = 8000, 20, 20, 400
    x1 = _signal(hz, frames * hop_in, rows=1, seed=7, amp=0.1)
    ref = _engine(frame_hz, hz, max_streams=2, max_batch=1)                  # test 2's engine A, one stream per call
    want = []
    for f in range(frames):
        hop = x1[:, :, f * hop_in:(f + 1) * hop_in]
        want.append([engine.split_outputs(ref.step(hop, [s]).copy()) for s in range(2)])     # both dialogues carry the same audio
    ref.close()
    data = wire.encode_input(x1[0, 0].astype(np.float64), x1[0, 1].astype(np.float64))
    assert len(data) == frames * hop_in * 16
    eng = _engine(frame_hz, hz, max_streams=2, max_batch=1)
    srv = ingest.NativeServer(eng, port_in=0, port_out=0, max_wait_s=0.5)
    try:
        ins = [socket.create_connection(("127.0.0.1", srv.port_in)) for _ in range(2)]
        while srv.stats()["in_connections"] < 2:
            time.sleep(0.01)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in range(2)]
        while srv.stats()["out_connections"] < 2:
            time.sleep(0.01)
        sent1 = 0
        for f in range(frames):
            for p in range(5):                                               # client 0: 10 ms packets of 80 pairs
                ins[0].sendall(data[(f * 5 + p) * 1280:(f * 5 + p + 1) * 1280])
            while sent1 < (f + 1) * hop_in * 16:                             # client 1: the same bytes in 1000-byte writes, across pair and frame boundaries
                ins[1].sendall(data[sent1:sent1 + 1000])
                sent1 += 1000
            for s in range(2):
                r = wire.decode_result(_read_packet(outs[s]))
                assert len(r["x1"]) == hop_in                                # the echo: hop_in samples as received
                np.testing.assert_array_equal(r["x1"], x1[0, 0, f * hop_in:(f + 1) * hop_in].astype(np.float64))
                np.testing.assert_array_equal(r["x2"], x1[0, 1, f * hop_in:(f + 1) * hop_in].astype(np.float64))
                for k in ("p_now", "p_future", "vad"):
                    assert np.array_equal(np.asarray(r[k], np.float64), want[f][s][k][0].astype(np.float64)), (f, s, k)
        st = srv.stats()
        assert st["frames_done"] == 2 * frames and st["numeric_resets"] == 0 and st["rx_bytes"] >= 2 * frames * hop_in * 16
    finally:
        srv.close()
        eng.close()
