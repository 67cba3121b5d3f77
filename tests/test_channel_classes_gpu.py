"""Input classes per channel on the GPU: the two channels of a stream in different sample formats and rates
(vapx_set_stream_channel_classes; csrc/input_classes.hip).

The reference of the whole output row is a PLAIN 16 kHz fp32 engine with no input setting at all, stepped with the same ids in the same
batch order (a row's last bit depends on the shape of its batch) and fed, per channel, the 16 kHz stream that channel's class defines:
the decoded samples (pcm.py), then vapx_resample of the whole signal, delayed (resample.delayed) - the construction of
tests/test_resample_gpu.py::_z.  Every float of every row is compared as uint32.  Per channel the mixed engine is also held against
the code of before: engines whose streams have ONE class, set by vapx_set_stream_class.  Only the TCP front-end is compared at the
project's 1e-4 bar (which rows share a tick is up to the receive threads).  Synthetic weights, frame_hz 20, ctx_frames 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
TABLE = [("f32", 16000), ("mulaw", 8000), ("s16", 48000), ("alaw", 32000)]
FRAME_HZ, HOP, TICKS = 20, 800, 13                                          # more than d + 2 = 9 ticks
# (16 k, 8 k) and (8 k, 16 k): one workgroup of the slot returns early, the other does not.  (48 k, 8 k) and (8 k, 48 k): H = 40 against 14
# in both orders, where a history laid out by the class's own H would overlap.  (32 k, 48 k); a same-class stream set through the new
# call; (16 k, 32 k)
PAIRS = [(0, 1), (1, 0), (2, 1), (1, 2), (3, 2), (1, 1), (0, 3)]
S = len(PAIRS)
EVT, SWAP, RESET = 5, 2, 4                                                  # at tick 5 stream 2 goes (48 k, 8 k) -> (8 k, 48 k) and stream 4 is reset


def _blob(frame_hz=FRAME_HZ, mode="vap", seed=0):
    key = ("blob", frame_hz, mode, seed)
    if key not in _CACHE:
        from vap_realtime_amd import weights as W
        _CACHE[key] = W.pack_blob(*W.synthetic_weights(seed, frame_hz, mode), mode)
    return _CACHE[key]


def _engine(max_streams=S, mode="vap", ctx_frames=8, **kw):
    from vap_realtime_amd import engine
    return engine.Engine(_blob(FRAME_HZ, mode), FRAME_HZ, (ctx_frames + 0.5) / FRAME_HZ, max_streams=max_streams, mode=mode, **kw)


def _raw(fmt, n, seed):
    """n seeded samples of moderate level (|value| < 0.125) in the format's own dtype; zero and both signs occur."""
    from vap_realtime_amd import pcm
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        x = (rng.integers(-4096, 4096, n) / 32768.0 + rng.standard_normal(n) * 1e-3).astype(np.float32)      # not on the s16 grid
        x[:2] = [0.0, -0.0]
        return x
    if fmt == "s16":
        x = rng.integers(-4096, 4096, n).astype(np.int16)
        x[:3] = [0, -1, 1]
        return x
    codes = np.nonzero(np.abs(pcm.TABLES[fmt].astype(np.int64)) < 4096)[0].astype(np.uint8)
    x = codes[rng.integers(0, len(codes), n)]
    x[:len(codes)] = codes
    return x


def _z(cls, raw, n_out):
    """The 16 kHz stream the model sees for the whole signal ``raw`` of class ``cls``: decoded, resampled as a whole on the GPU, delayed."""
    import torch
    from vap_realtime_amd import engine, pcm, resample
    fmt, hz = cls
    x = raw if fmt == "f32" else pcm.decode(fmt, raw, np.float32)
    assert x.dtype == np.float32
    if hz == 16000:
        return x[:n_out]
    q = resample.geometry(hz)
    n_y = -(-q["new"] * x.size // q["orig"])
    xd, yd = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.zeros(n_y, device="cuda")
    assert engine.load_library().vapx_resample(hz, 1, x.size, xd.data_ptr(), yd.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return resample.delayed(yd.cpu().numpy(), hz, n_out)


def _schedule(n_streams, ticks, seed):
    """Per tick the stream ids of the batch: everybody first, then ragged, reordered subsets - slot offsets change from tick to tick and
    streams skip ticks.  Ticks 5 and 6 and the last hold every stream again, so that what tick 5 queues meets every stream at once."""
    rng = np.random.default_rng(seed)
    plan = []
    for t in range(ticks):
        k = n_streams if t in (0, 5, 6, ticks - 1) else int(rng.integers(n_streams // 3, n_streams + 1))
        plan.append([int(s) for s in rng.permutation(n_streams)[:k]])
    return plan


class _Plan:
    """Signals and the 16 kHz streams they define.  A stream's signal is per EPOCH: epoch 1 begins at tick EVT for the streams of the
    events (a new pair of classes, or a reset, is a new signal from its first sample) when ``events`` is set."""

    def __init__(self, events):
        self.events = events
        self.plan = _schedule(S, TICKS, seed=3 + events)
        self.raw, self.z = {}, {}
        for s in range(S):
            for ep in range(2 if events and s in (SWAP, RESET) else 1):
                pair = self.pair(s, ep)
                for ch in range(2):
                    fmt, hz = TABLE[pair[ch]]
                    self.raw[s, ep, ch] = _raw(fmt, TICKS * (hz // FRAME_HZ), seed=1000 * ep + 10 * s + ch)
                    self.z[s, ep, ch] = _z(TABLE[pair[ch]], self.raw[s, ep, ch], TICKS * HOP)

    @staticmethod
    def pair(s, ep):
        return PAIRS[s][::-1] if ep and s == SWAP else PAIRS[s]

    def walk(self):
        """Per tick: (t, ids, [(epoch, own frame index) per id])."""
        frame, epoch = [0] * S, [0] * S
        for t, ids in enumerate(self.plan):
            if self.events and t == EVT:
                for s in (SWAP, RESET):
                    frame[s], epoch[s] = 0, 1
            yield t, ids, [(epoch[s], frame[s]) for s in ids]
            for s in ids:
                frame[s] += 1

    def legs(self, s, ep, k):
        """The slot of stream s for its own frame k: its two rows, each in its own class."""
        pair, rows = self.pair(s, ep), []
        for ch in range(2):
            h = TABLE[pair[ch]][1] // FRAME_HZ
            rows.append(self.raw[s, ep, ch][k * h:(k + 1) * h])
        return tuple(rows)

    def hop16(self, s, ep, k):
        return np.stack([self.z[s, ep, ch][k * HOP:(k + 1) * HOP] for ch in range(2)])


def _plan(events):
    if ("plan", events) not in _CACHE:
        _CACHE["plan", events] = _Plan(events)
    return _CACHE["plan", events]


def _reference(events, split):
    """want[t] = the output rows of tick t of a plain 16 kHz engine fed the streams the classes define.  Recorded once, never changed."""
    key = ("ref", events, split)
    if key not in _CACHE:
        p = _plan(events)
        e = _engine(split_f16=split)
        want = []
        for t, ids, at in p.walk():
            if events and t == EVT:
                e.reset_carry(SWAP)                                         # the LSTM and the ring are carried over
                e.reset_stream(RESET)
            want.append(e.step(np.stack([p.hop16(s, ep, k) for s, (ep, k) in zip(ids, at)]), ids).copy())
        e.close()
        for w in want:
            w.setflags(write=False)
        _CACHE[key] = want
    return _CACHE[key]


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _mixed_engine(**kw):
    e = _engine(input_classes=TABLE, **kw)
    for s in range(S):
        e.set_stream_channel_classes(s, *PAIRS[s])                          # stream 5: one class, through the new call
    return e


def _run_mixed(e, p, mode, on_tick=None):
    import torch
    from vap_realtime_amd import engine
    rows = [e.input_row_bytes(c) for c in range(len(TABLE))]
    pin = engine.pinned_empty((S * 2 * max(rows),), np.uint8) if mode == "pinned" else None
    got, offsets = [], set()
    for t, ids, at in p.walk():
        if on_tick:
            on_tick(t)
        arrays = [p.legs(s, ep, k) for s, (ep, k) in zip(ids, at)]
        offsets.add(tuple(np.cumsum([0] + [a[0].nbytes + a[1].nbytes for a in arrays[:-1]])))
        if mode == "pageable":
            got.append(e.step(arrays, ids).copy())                          # a list of per-slot pairs of rows
        elif mode == "pinned":
            block = e.pack_input(ids, arrays, out=pin)
            assert block.ctypes.data == pin.ctypes.data
            got.append(e.step(block, ids).copy())                           # one packed uint8 block, page-locked
        else:
            dev = torch.from_numpy(e.pack_input(ids, arrays).copy()).cuda()
            out = torch.zeros((len(ids), engine.OUT_STRIDE), device="cuda")
            assert dev.data_ptr() % 16 == 0
            e.step_packed_device(ids, dev.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            got.append(out.cpu().numpy())
    assert len(offsets) >= TICKS - 3                                        # the slot offsets did move from tick to tick
    return got


# ---- 1. the whole output row, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split_f16"])
@pytest.mark.parametrize("mode", ["pageable", "pinned", "device"])
def test_mixed_legs_equal_a_16k_engine_fed_the_streams_the_classes_define(mode, split):
    from vap_realtime_amd import engine
    p, want = _plan(False), _reference(False, split)
    e = _mixed_engine(split_f16=split)
    assert [e.stream_channel_classes(s) for s in range(S)] == PAIRS and e.stream_class(5) == 1
    got = _run_mixed(e, p, mode)
    for t, ids in enumerate(p.plan):
        bad = [(k, ids[k], PAIRS[ids[k]]) for k in range(len(ids)) if not _same_bits(got[t][k], want[t][k])]
        assert not bad, f"tick {t}: (slot, stream, classes) {bad}: max {np.abs(got[t] - want[t]).max()}"
    last = got[-1]
    assert np.isfinite(last).all() and np.abs(last[:, :6]).max() > 0
    assert last[:, engine.OUT_NVALID].tolist() == [min(sum(s in ids for ids in p.plan), 8) for s in p.plan[-1]]
    e.close()


# ---- 2. each channel against the code of before ----------------------------------------------------------------------------------------
def test_each_channel_equals_a_stream_of_one_class_set_by_the_old_call():
    """Engine ``one[ch]`` has every stream in ONE class, the class of its channel ch in the mixed engine, set by vapx_set_stream_class, and
    hears that channel with the other one silent.  The encoder output (VAPX_OUT_E) of channel ch of the mixed run equals it, every tick."""
    from vap_realtime_amd import engine, pcm
    p = _plan(False)
    mixed = _mixed_engine()
    got = _run_mixed(mixed, p, "pageable")
    mixed.close()
    for ch in range(2):
        one = _engine(input_classes=TABLE)
        for s in range(S):
            one.set_stream_class(s, PAIRS[s][ch])
        for t, ids, at in p.walk():
            arrays = []
            for s, (ep, k) in zip(ids, at):
                c = PAIRS[s][ch]
                own = p.legs(s, ep, k)[ch]
                sil = np.full_like(own, pcm.SILENCE[TABLE[c][0]])
                arrays.append(np.stack([own, sil] if ch == 0 else [sil, own]))      # [2, hop_in] of one class: today's slot
            w = engine.split_outputs(one.step(arrays, ids))["e"][:, ch]
            g = engine.split_outputs(got[t])["e"][:, ch]
            bad = [(ids[k], PAIRS[ids[k]]) for k in range(len(ids)) if not _same_bits(np.ascontiguousarray(g[k]), np.ascontiguousarray(w[k]))]
            assert not bad, f"tick {t}, channel {ch + 1}: (stream, classes) {bad}"
        assert np.abs(w).max() > 0
        one.close()


# ---- 3. a class change in mid-run ------------------------------------------------------------------------------------------------------
def test_a_class_change_in_mid_run():
    """At tick 5 stream 2 goes (48 k, 8 k) -> (8 k, 48 k) and stream 4 is reset.  From that tick on they equal, in the reference, a fresh
    signal of the new pair on a stream whose LSTM and ring were carried over (reset_carry), and a stream reset in full."""
    from vap_realtime_amd import engine
    p, want = _plan(True), _reference(True, False)
    e = _mixed_engine()

    def on_tick(t):
        if t == EVT:
            e.set_stream_channel_classes(SWAP, *PAIRS[SWAP][::-1])
            e.reset_stream(RESET)
            assert e.stream_channel_classes(SWAP) == PAIRS[SWAP][::-1]
            with pytest.raises(engine.VapxError, match="vapx_get_stream_channel_classes"):
                e.stream_class(SWAP)

    got = _run_mixed(e, p, "pageable", on_tick)
    for t, ids in enumerate(p.plan):
        bad = [(k, ids[k]) for k in range(len(ids)) if not _same_bits(got[t][k], want[t][k])]
        assert not bad, f"tick {t}: (slot, stream) {bad}: max {np.abs(got[t] - want[t]).max()}"
    seen = sum(SWAP in ids for ids in p.plan)                               # stream 2 kept its window across the change ...
    since = sum(RESET in ids for ids in p.plan[EVT:])                       # ... stream 4 restarted its own at tick 5
    last, ids = got[-1], p.plan[-1]
    assert last[ids.index(SWAP), engine.OUT_NVALID] == min(seen, 8) and last[ids.index(RESET), engine.OUT_NVALID] == min(since, 8) and seen > since
    e.close()


# ---- 4. a trunk group with mixed legs on the leader --------------------------------------------------------------------------------------
def test_trunk_group_with_mixed_legs_on_the_leader():
    """vap leads at 20 Hz; bc follows with a window of its own, nod at 10 Hz.  The vapx_step_group wire rows equal those of a group whose
    leader is the plain 16 kHz engine fed the reference streams."""
    from vap_realtime_amd import engine as E, weights as W
    cpc = W.synthetic_weights(41, 20, "vap")[0]
    blobs = {"vap": W.pack_blob(cpc, W.synthetic_weights(42, 20, "vap")[1], "vap"),
             "bc": W.pack_blob(cpc, W.synthetic_weights(43, 20, "bc")[1], "bc"),
             "nod": W.pack_blob(cpc, W.synthetic_weights(44, 10, "nod")[1], "nod")}
    hz, ctx = {"vap": 20, "bc": 20, "nod": 10}, {"vap": 8.5 / 20, "bc": 12.5 / 20, "nod": 6.5 / 10}
    p = _plan(False)
    mixed = E.TrunkGroup(blobs, hz, ctx, max_streams=S, input_classes=TABLE)
    plain = E.TrunkGroup(blobs, hz, ctx, max_streams=S)
    assert mixed.order[0] == "vap" and mixed.R["nod"] == 2
    for s in range(S):
        mixed.leader.set_stream_channel_classes(s, *PAIRS[s])
    for t, ids, at in p.walk():
        if t == 10:
            break
        got = mixed.step_wire([p.legs(s, ep, k) for s, (ep, k) in zip(ids, at)], ids)
        want = plain.step_wire(np.stack([p.hop16(s, ep, k) for s, (ep, k) in zip(ids, at)]), ids)
        for m in ("vap", "bc", "nod"):
            assert _same_bits(np.ascontiguousarray(got[m]), np.ascontiguousarray(want[m])), (t, m)
    assert (got["nod"][:, E.OUT_STATUS] != E.STATUS_NO_FRAME).any() and np.abs(got["bc"][:, :10]).max() > 0
    mixed.close()
    plain.close()


# ---- 5. the new calls -------------------------------------------------------------------------------------------------------------
def test_the_new_calls_and_their_refusals():
    import ctypes as C
    from vap_realtime_amd import engine as E
    lib = E.load_library()
    assert lib.vapx_abi_version() == 2
    two = (C.c_int32 * 2)(7, 7)

    def refused(e, rc, code, *words):
        msg = lib.vapx_last_error(e._h).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    plain = _engine(max_streams=2)                                          # no table
    refused(plain, lib.vapx_set_stream_channel_classes(plain._h, 0, 0, 0), -1, "no input classes")
    refused(plain, lib.vapx_get_stream_channel_classes(plain._h, 0, two), -1, "no input classes")
    assert lib.vapx_input_row_bytes(plain._h, 0) == 0 and list(two) == [7, 7]
    plain.close()
    uni = _engine(max_streams=2, input_hz=8000, input_format="mulaw")       # a uniform engine has no table either
    refused(uni, lib.vapx_set_stream_channel_classes(uni._h, 0, 0, 0), -1, "no input classes")
    assert lib.vapx_input_row_bytes(uni._h, 0) == 0
    uni.close()

    a, b = _engine(max_streams=4, input_classes=TABLE), _engine(max_streams=4, input_classes=TABLE)
    assert [lib.vapx_input_row_bytes(a._h, c) for c in (0, 1, 2, 3, 4, -1)] == [800 * 4, 400, 2400 * 2, 1600, 0, 0]
    assert [lib.vapx_input_slot_bytes(a._h, c) for c in range(4)] == [2 * lib.vapx_input_row_bytes(a._h, c) for c in range(4)]
    assert lib.vapx_get_stream_channel_classes(a._h, 3, two) == 0 and list(two) == [0, 0]      # every channel starts in class 0
    for e in (a, b):
        e.set_stream_channel_classes(0, 2, 1)
        e.set_stream_class(1, 3)                                            # the old call means (c, c)
        e.set_stream_channel_classes(2, 1, 1)
    assert [a.stream_channel_classes(s) for s in range(4)] == [(2, 1), (3, 3), (1, 1), (0, 0)]
    assert a.stream_class(1) == 3 and a.stream_class(2) == 1
    refused(a, lib.vapx_get_stream_class(a._h, 0), -1, "stream 0", "(2, 1)", "vapx_get_stream_channel_classes")
    rng = np.random.default_rng(5)
    pairs = [(2, 1), (3, 3), (1, 1), (0, 0)]

    def arrays(ids):
        out = []
        for s in ids:
            out.append(tuple(_raw(TABLE[c][0], TABLE[c][1] // FRAME_HZ, seed=int(rng.integers(1 << 30))) for c in pairs[s]))
        return out

    ids = [2, 0, 3, 1]
    x = arrays(ids)
    # the slot of a stream is row(c1) + row(c2)
    assert a.pack_input(ids, x).size == sum(a.input_row_bytes(c) for s in ids for c in pairs[s]) == 800 + (4800 + 400) + 6400 + 3200
    assert _same_bits(a.step(x, ids).copy(), b.step(x, ids).copy())
    # refused calls: a bad id, a bad class in either channel, a null out - and nothing changes
    refused(a, lib.vapx_set_stream_channel_classes(a._h, 4, 0, 0), -4, "stream id 4")
    refused(a, lib.vapx_set_stream_channel_classes(a._h, -1, 0, 0), -4, "stream id -1")
    refused(a, lib.vapx_set_stream_channel_classes(a._h, 0, 4, 0), -4, "class 4", "channel 1")
    refused(a, lib.vapx_set_stream_channel_classes(a._h, 0, 1, -1), -4, "class -1", "channel 2")
    refused(a, lib.vapx_get_stream_channel_classes(a._h, 4, two), -4, "stream id 4")
    refused(a, lib.vapx_get_stream_channel_classes(a._h, 0, None), -1, "null out")
    assert [a.stream_channel_classes(s) for s in range(4)] == pairs
    for _ in range(3):                                                      # had a refused call queued a reset, the carry would differ now
        x = arrays(ids)
        assert _same_bits(a.step(x, ids).copy(), b.step(x, ids).copy())
    # the refusals of a table engine stand for a stream with mixed legs
    import torch
    block = E.aligned_bytes(a.pack_input(ids, x).size)
    block[:] = a.pack_input(ids, x)
    out = np.zeros((4, E.OUT_STRIDE), np.float32)
    idv = np.array(ids, np.int32)
    refused(a, lib.vapx_step(a._h, 4, idv.ctypes.data, block.ctypes.data, 800, out.ctypes.data, 0, None), -1, "samples_per_ch must be 0")
    rec = np.zeros((1, int(lib.vapx_state_floats(a._h, 0))), np.float32)
    refused(a, lib.vapx_export_streams(a._h, 1, None, rec.ctypes.data, 0, None), -1, "vapx_export_streams", "input classes")
    fr, emb = torch.zeros((1, 2, 1120), device="cuda"), torch.zeros((1, 2, 256), device="cuda")
    refused(a, lib.vapx_encode_audio(a._h, 1, None, fr.data_ptr(), emb.data_ptr(), None), -1, "input classes")
    x = arrays(ids)
    assert _same_bits(a.step(x, ids).copy(), b.step(x, ids).copy())
    a.close()
    b.close()


# ---- 6. the native front-end, end to end ---------------------------------------------------------------------------------------------
def _read_packet(sock):
    import struct
    sock.settimeout(20)
    buf = b""
    while len(buf) < 4:
        buf += sock.recv(4 - len(buf))
    ln = struct.unpack("<I", buf)[0]
    payload = b""
    while len(payload) < ln:
        payload += sock.recv(ln - len(payload))
    return payload


def test_front_end_end_to_end_with_a_pair_port():
    """Two dialogues on a pair port (mulaw@8000 + s16@48000) and one on the plain class port of s16@48000, 10 frames in 10 ms packets.
    Every frame is answered; the echo blocks have their own lengths (400 and 2400 samples) and are the decoded samples exactly; the heads
    agree with a direct run of a mixed engine within the project's 1e-4 (which rows share a tick is up to the receive threads' timing, and
    a row's last bit depends on the shape of its batch: no bit equality here, as in tests/test_input_classes_gpu.py)."""
    import socket
    import time
    from vap_realtime_amd import engine, ingest, pcm, wire
    classes = [("mulaw", 8000), ("s16", 48000)]
    frames, n = 10, 3
    of = [(0, 1), (0, 1), (1, 1)]
    hop_in = [400, 2400]
    sig = [[_raw(classes[c][0], frames * hop_in[c], seed=70 + 2 * s + ch) for ch, c in enumerate(of[s])] for s in range(n)]
    dec = [[pcm.decode(classes[c][0], sig[s][ch], np.float64) for ch, c in enumerate(of[s])] for s in range(n)]
    ref = _engine(max_streams=n, input_classes=classes)
    for s in range(n):
        ref.set_stream_channel_classes(s, *of[s])
    want = []
    for f in range(frames):
        arrays = [tuple(sig[s][ch][f * hop_in[c]:(f + 1) * hop_in[c]] for ch, c in enumerate(of[s])) for s in range(n)]
        want.append(engine.split_outputs(ref.step(arrays).copy()))
    ref.close()
    eng = _engine(max_streams=n, input_classes=classes)
    srv = ingest.NativeServer(eng, port_in=0, port_out=0, max_wait_s=0.5, pair_ports=[(0, 1, 0)])
    try:
        assert len(srv.class_ports) == 2 and len(srv.pair_ports) == 1 and srv.pair_ports[0] not in srv.class_ports
        ins = []
        for s, port in enumerate([srv.pair_ports[0], srv.pair_ports[0], srv.class_ports[1]]):      # one after another: the lowest free slot is s
            ins.append(socket.create_connection(("127.0.0.1", port)))
            while srv.stats()["in_connections"] < s + 1:
                time.sleep(0.005)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in range(n)]
        while srv.stats()["out_connections"] < n:
            time.sleep(0.01)
        data = [wire.encode_input_planar(sig[s][0], classes[0], sig[s][1], classes[1]) for s in range(2)]
        data.append(wire.encode_input(sig[2][0], sig[2][1], "s16"))
        pkt = [80 + 960, 80 + 960, 1920]
        worst = 0.0
        for f in range(frames):
            for s in range(n):
                for q in range(5):
                    ins[s].sendall(data[s][(f * 5 + q) * pkt[s]:(f * 5 + q + 1) * pkt[s]])
            for s in range(n):
                r = wire.decode_result(_read_packet(outs[s]))
                h = [hop_in[c] for c in of[s]]
                assert len(r["x1"]) == h[0] and len(r["x2"]) == h[1], (f, s)
                assert np.array_equal(r["x1"], dec[s][0][f * h[0]:(f + 1) * h[0]]) and np.array_equal(r["x2"], dec[s][1][f * h[1]:(f + 1) * h[1]]), (f, s)
                for k in ("p_now", "p_future", "vad"):
                    worst = max(worst, float(np.abs(np.asarray(r[k], np.float64) - want[f][k][s].astype(np.float64)).max()))
        print(f"pair port through TCP: max |front-end - direct mixed engine| = {worst:.2e}")
        assert worst <= 1e-4
        st = srv.stats()
        assert st["frames_done"] == n * frames and st["numeric_resets"] == 0 and st["rx_bytes"] == frames * 5 * sum(pkt)
        assert [eng.stream_channel_classes(s) for s in range(n)] == of
    finally:
        srv.close()
        eng.close()
    assert [eng._cls[s].tolist() for s in range(n)] == [list(c) for c in of]      # the mirror followed the front-end (refresh_stream_classes)
