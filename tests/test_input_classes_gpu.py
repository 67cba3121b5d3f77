"""Input classes on the GPU: streams of different sample formats and rates in one engine (vapx_set_input_classes; csrc/input_classes.hip).

Every comparison of outputs is BIT EQUALITY against the existing uniform path: an engine with vapx_set_input_rate + vapx_set_input_format
per class, which tests/test_pcm_gpu.py and tests/test_resample_gpu.py tie to pcm.py / resample.py and float64.  The mixed kernel and the
uniform kernels share one definition of each expansion and of the resampler's chain (csrc/input_decode.h), so no tolerance is needed.

A row's last bits may depend on the shape of its batch (which GEMM tile a row falls into), so a uniform engine never steps a smaller
batch than the mixed engine: class c's engine steps the SAME ids in the SAME order, with the real samples in the slots of its own streams
and silence in the others, and only its own streams' rows are compared.  Synthetic weights, ctx_frames = 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
FORMATS = ("f32", "s16", "mulaw", "alaw")
RATES = (16000, 8000, 32000, 48000)
ALL = [(f, r) for r in RATES for f in FORMATS]
# two cases of 8 classes, together all 16 combinations.  A (50 Hz) has the smallest slots: 8 kHz G.711 is 160 bytes per channel;
# B (5 Hz) the largest window: 48 kHz f32 is hop_in 9600 (K = 41 taps; the 8 kHz classes of A run the two-phase table, K = 15)
CASE_A = (50, [("mulaw", 8000), ("alaw", 8000), ("s16", 8000), ("f32", 16000), ("mulaw", 16000), ("alaw", 16000), ("s16", 32000), ("alaw", 32000)])
CASE_B = (5, [("f32", 48000), ("s16", 48000), ("mulaw", 48000), ("alaw", 48000), ("f32", 8000), ("f32", 32000), ("mulaw", 32000), ("s16", 16000)])
assert sorted(set(CASE_A[1]) | set(CASE_B[1])) == sorted(ALL) and len(CASE_A[1]) == len(CASE_B[1]) == 8
CASES = {"A_50hz": CASE_A, "B_5hz": CASE_B}


def _blob(frame_hz, mode="vap", seed=0):
    key = ("blob", frame_hz, mode, seed)
    if key not in _CACHE:
        from vap_realtime_amd import weights as W
        _CACHE[key] = W.pack_blob(*W.synthetic_weights(seed, frame_hz, mode), mode)
    return _CACHE[key]


def _engine(frame_hz, max_streams=6, mode="vap", ctx_frames=8, **kw):
    from vap_realtime_amd import engine
    return engine.Engine(_blob(frame_hz, mode), frame_hz, (ctx_frames + 0.5) / frame_hz, max_streams=max_streams, mode=mode, **kw)


def _raw(fmt, shape, seed):
    """Seeded samples of moderate level (|value| < 0.125) in the format's own dtype; zero and both signs occur."""
    from vap_realtime_amd import pcm
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        x = (rng.integers(-4096, 4096, shape) / 32768.0 + rng.standard_normal(shape) * 1e-3).astype(np.float32)      # not on the s16 grid
        x.reshape(-1)[:2] = [0.0, -0.0]
        return x
    if fmt == "s16":
        x = rng.integers(-4096, 4096, shape).astype(np.int16)
        x.reshape(-1)[:3] = [0, -1, 1]
        return x
    codes = np.nonzero(np.abs(pcm.TABLES[fmt].astype(np.int64)) < 4096)[0].astype(np.uint8)
    x = codes[rng.integers(0, len(codes), shape)]
    x.reshape(-1)[:len(codes)] = codes
    return x


def _silence(cls, frame_hz):
    from vap_realtime_amd import engine, pcm
    dt, shape = engine.input_slot_shape(cls, frame_hz)
    return np.full(shape, pcm.SILENCE[cls[0]], dt)


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
    """Signals, classes over time and the events of tick 5 for one case: two streams per class; stream X is reset, stream Y moves to a
    class of ITS OWN RATE in another format with its model state kept, stream Z is reset and moves to a class of ANOTHER rate."""

    def __init__(self, frame_hz, classes, ticks=12):
        self.frame_hz, self.classes, self.ticks = frame_hz, classes, ticks
        self.S = 2 * len(classes)
        self.plan = _schedule(self.S, ticks, seed=frame_hz)
        first = [s // 2 for s in range(self.S)]
        self.X = 3
        self.Y, y_to = next((s, c) for s in range(4, self.S) for c in range(len(classes))
                            if classes[c][1] == classes[first[s]][1] and c != first[s])
        self.Z, z_to = next((s, c) for s in range(self.S - 1, 0, -1) for c in range(len(classes))
                            if s != self.Y and classes[c][1] != classes[first[s]][1] and classes[c][1] != 16000)
        assert len({self.X, self.Y, self.Z}) == 3
        self.y_from, self.y_to, self.z_to = first[self.Y], y_to, z_to
        self.cls_at = [list(first) for _ in range(ticks)]                   # [tick][stream] -> class
        for t in range(5, ticks):
            self.cls_at[t][self.Y], self.cls_at[t][self.Z] = y_to, z_to
        self.sig = {}                                                       # (stream, class) -> [2, ticks * hop_in] samples of that class
        for s in range(self.S):
            for c in {self.cls_at[0][s], self.cls_at[ticks - 1][s]}:
                self.sig[s, c] = _raw(classes[c][0], (2, ticks * (classes[c][1] // frame_hz)), seed=100 * s + c + frame_hz)

    def slot(self, t, s, c=None):
        c = self.cls_at[t][s] if c is None else c
        hop_in = self.classes[c][1] // self.frame_hz
        return np.ascontiguousarray(self.sig[s, c][:, t * hop_in:(t + 1) * hop_in])


def _reference(name):
    """Recorded once per case: want[t][k] = the output row of batch slot k of tick t, taken from the uniform engine of that stream's class."""
    if ("ref", name) in _CACHE:
        return _CACHE["ref", name]
    frame_hz, classes = CASES[name]
    p = _Plan(frame_hz, classes)
    uni = [_engine(frame_hz, max_streams=p.S, input_hz=hz, input_format=f) for f, hz in classes]
    sil = [_silence(c, frame_hz) for c in classes]
    want = []
    for t, ids in enumerate(p.plan):
        if t == 5:
            for e in uni:
                e.reset_stream(p.X)
                e.reset_stream(p.Z)
            # Y keeps its LSTM and window: its whole state record moves to the engine of the new class (the same rate, so the record fits;
            # with the cache the continuation is bit-identical, tests/test_state_bulk_gpu.py), then the reconnect's reset_carry on both
            uni[p.y_to].import_streams([p.Y], uni[p.y_from].export_streams([p.Y], cache=True), cache=True)
            uni[p.y_to].reset_carry(p.Y)
        rows = np.zeros((len(ids), 784), np.float32)
        for c, e in enumerate(uni):
            mine = [k for k, s in enumerate(ids) if p.cls_at[t][s] == c]
            if not mine:
                continue
            block = np.stack([p.slot(t, s) if p.cls_at[t][s] == c else sil[c] for s in ids])
            rows[mine] = e.step(block, ids)[mine]
        want.append(rows)
    for e in uni:
        e.close()
    _CACHE["ref", name] = (p, want)
    return p, want


# ---- 1. a mixed batch equals the uniform engines -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pageable", "pinned", "device"])
@pytest.mark.parametrize("name", list(CASES))
def test_mixed_batch_equals_the_uniform_engines_bit_for_bit(name, mode):
    import torch
    from vap_realtime_amd import engine
    frame_hz, classes = CASES[name]
    p, want = _reference(name)
    e = _engine(frame_hz, max_streams=p.S, input_classes=classes)
    assert [e.stream_class(s) for s in range(p.S)] == [0] * p.S             # every stream starts in class 0
    for s in range(p.S):
        e.set_stream_class(s, p.cls_at[0][s])                               # 16+ queued requests: more than one launch of the reset kernel
    sizes = [e.input_slot_bytes(c) for c in range(len(classes))]
    assert sizes == [engine.input_slot_bytes(c, frame_hz) for c in classes] and all(b % 16 == 0 for b in sizes)
    assert (min(sizes) == 320 and frame_hz == 50) or (max(sizes) == 2 * 9600 * 4 and frame_hz == 5)
    pin = engine.pinned_empty((p.S * max(sizes),), np.uint8) if mode == "pinned" else None
    offsets_seen = set()
    for t, ids in enumerate(p.plan):
        if t == 5:
            e.reset_stream(p.X)
            e.set_stream_class(p.Y, p.y_to)
            e.reset_carry(p.Y)                                              # the reconnect's call, as on the uniform side: already queued
            e.reset_stream(p.Z)
            e.set_stream_class(p.Z, p.z_to)
            assert e.stream_class(p.Y) == p.y_to and e.stream_class(p.Z) == p.z_to
        arrays = [p.slot(t, s) for s in ids]
        offsets_seen.add(tuple(np.cumsum([0] + [a.nbytes for a in arrays[:-1]])))
        if mode == "pageable":
            got = e.step(arrays, ids).copy()                                # a list of per-slot arrays
        elif mode == "pinned":
            block = e.pack_input(ids, arrays, out=pin)
            assert block.ctypes.data == pin.ctypes.data
            got = e.step(block, ids).copy()                                 # one packed uint8 block, page-locked
        else:
            dev = torch.from_numpy(e.pack_input(ids, arrays).copy()).cuda()
            out = torch.zeros((len(ids), engine.OUT_STRIDE), device="cuda")
            assert dev.data_ptr() % 16 == 0
            e.step_packed_device(ids, dev.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            got = out.cpu().numpy()
        bad = [(k, ids[k], classes[p.cls_at[t][ids[k]]]) for k in range(len(ids)) if not np.array_equal(got[k], want[t][k])]
        assert not bad, f"tick {t}: (slot, stream, class) {bad}: max {np.abs(got - want[t]).max()}"
    assert len(offsets_seen) >= p.ticks - 3                                 # the slot offsets did change from tick to tick
    assert np.isfinite(got).all() and np.abs(got[:, :6]).max() > 0 and got[:, engine.OUT_NVALID].min() >= 1
    seen = {s: sum(s in ids for ids in p.plan) for s in (p.Y, 0)}           # Y kept its window across the class change ...
    since5 = {s: sum(s in ids for ids in p.plan[5:]) for s in (p.X, p.Z)}   # ... X and Z restarted theirs at tick 5
    for s, frames in {**seen, **since5}.items():
        assert got[p.plan[-1].index(s), engine.OUT_NVALID] == min(frames, 8), (s, frames)
    assert seen[p.Y] > since5[p.Z]
    e.close()


# ---- 2. a one-class table equals vapx_set_input_rate + vapx_set_input_format ---------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split_f16"])
@pytest.mark.parametrize("cls", [("mulaw", 8000), ("s16", 48000)], ids=["mulaw_8k", "s16_48k"])
def test_one_class_table_equals_rate_plus_format(cls, split):
    frame_hz, ticks, S = 20, 6, 3
    hop_in = cls[1] // frame_hz
    raw = _raw(cls[0], (S, 2, ticks * hop_in), seed=cls[1])
    a = _engine(frame_hz, max_streams=S, split_f16=split, input_classes=[cls])
    b = _engine(frame_hz, max_streams=S, split_f16=split, input_hz=cls[1], input_format=cls[0])
    for t in range(ticks):
        seg = np.ascontiguousarray(raw[:, :, t * hop_in:(t + 1) * hop_in])
        # a list of per-slot arrays (ids None: 0 .. n-1), or the uniform block itself: with one class it IS the packed block
        got = a.step(seg.reshape(-1).view(np.uint8), [0, 1, 2]) if t % 2 else a.step(list(seg))
        assert np.array_equal(got, b.step(seg)), t
    assert np.isfinite(got).all() and np.abs(got[:, :6]).max() > 0
    a.close()
    b.close()


# ---- 3. a trunk group with a table on the leader ----------------------------------------------------------------------------------
def test_trunk_group_with_a_table_on_the_leader():
    """vap leads at 20 Hz; bc follows with a window of its own, nod at 10 Hz.  vapx_step_group wire rows of the mixed leader equal those
    of a uniform-leader group per class (same ids, silence in the other classes' slots)."""
    from vap_realtime_amd import engine as E, weights as W
    classes = [("f32", 16000), ("mulaw", 8000), ("s16", 48000)]
    cpc = W.synthetic_weights(41, 20, "vap")[0]
    blobs = {"vap": W.pack_blob(cpc, W.synthetic_weights(42, 20, "vap")[1], "vap"),
             "bc": W.pack_blob(cpc, W.synthetic_weights(43, 20, "bc")[1], "bc"),
             "nod": W.pack_blob(cpc, W.synthetic_weights(44, 10, "nod")[1], "nod")}
    hz, ctx = {"vap": 20, "bc": 20, "nod": 10}, {"vap": 8.5 / 20, "bc": 12.5 / 20, "nod": 6.5 / 10}
    S, ticks = 6, 10
    mixed = E.TrunkGroup(blobs, hz, ctx, max_streams=S, input_classes=classes)
    assert mixed.order[0] == "vap" and mixed.R["nod"] == 2 and mixed.T_of["bc"] == 12 and mixed.input_classes == classes
    lib = mixed.leader.lib
    assert lib.vapx_get_input_classes(mixed.leader._h, None, 0) == 3 and lib.vapx_get_input_classes(mixed.engines["bc"]._h, None, 0) == 0
    uni = [E.TrunkGroup(blobs, hz, ctx, max_streams=S, input_hz=r, input_format=f) for f, r in classes]
    cls_of = [s % 3 for s in range(S)]
    for s in range(S):
        mixed.leader.set_stream_class(s, cls_of[s])
    sig = [_raw(classes[cls_of[s]][0], (2, ticks * (classes[cls_of[s]][1] // 20)), seed=7 + s) for s in range(S)]
    sil = [_silence(c, 20) for c in classes]
    plan = [[0, 1, 2, 3, 4, 5], [5, 3, 1, 0, 2, 4], [4, 0, 5], [1, 2, 3, 4, 5, 0], [2, 5, 1, 3], [0, 1, 2, 3, 4, 5]]
    frame = [0] * S                                                         # a stream's own next hop
    for t in range(ticks):
        ids = plan[t % len(plan)]
        def hop_of(s):
            h = classes[cls_of[s]][1] // 20
            return np.ascontiguousarray(sig[s][:, frame[s] * h:(frame[s] + 1) * h])
        got = mixed.step_wire([hop_of(s) for s in ids], ids)
        for c, g in enumerate(uni):
            want = g.step_wire(np.stack([hop_of(s) if cls_of[s] == c else sil[c] for s in ids]), ids)
            mine = [k for k, s in enumerate(ids) if cls_of[s] == c]
            for m in ("vap", "bc", "nod"):
                assert np.array_equal(got[m][mine], want[m][mine]), (t, c, m)
        for s in ids:
            frame[s] += 1
    assert (got["nod"][:, E.OUT_STATUS] != E.STATUS_NO_FRAME).any() and np.abs(got["bc"][:, :10]).max() > 0
    assert got["vap"][:, E.OUT_NVALID].min() >= 5
    for g in uni + [mixed]:
        g.close()


# ---- 4. refusals and queries -----------------------------------------------------------------------------------------------------
def test_refusals_and_queries():
    import ctypes as C
    import torch
    from vap_realtime_amd import engine as E
    lib = E.load_library()
    assert lib.vapx_abi_version() == 2

    def table(entries):
        return (E._InputClass * max(len(entries), 1))(*[E._InputClass(hz, f) for hz, f in entries])

    def refused(e, rc, code, *words):
        msg = lib.vapx_last_error(e._h).decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)

    three = [(16000, 0), (8000, 2), (48000, 1)]
    e = _engine(20, max_streams=4)
    assert lib.vapx_get_input_classes(e._h, None, 0) == 0 and lib.vapx_input_slot_bytes(e._h, 0) == 0       # no table
    refused(e, lib.vapx_set_stream_class(e._h, 0, 0), -1, "no input classes")
    # n = 0 and n = 17; a bad rate, a bad format, a duplicate entry
    refused(e, lib.vapx_set_input_classes(e._h, 0, table(three)), -1, "n = 0", "1 .. 16")
    refused(e, lib.vapx_set_input_classes(e._h, 17, table(three * 6)), -1, "n = 17", "1 .. 16")
    refused(e, lib.vapx_set_input_classes(e._h, 2, table([(16000, 0), (44100, 1)])), -1, "class 1", "44100")
    refused(e, lib.vapx_set_input_classes(e._h, 2, table([(16000, 4), (8000, 1)])), -1, "class 0", "format 4")
    refused(e, lib.vapx_set_input_classes(e._h, 3, table([(8000, 2), (16000, 0), (8000, 2)])), -1, "classes 0 and 2", "duplicate")
    assert lib.vapx_get_input_classes(e._h, None, 0) == 0                   # a refused call changes nothing
    # the table itself, and what the queries give back
    assert lib.vapx_set_input_classes(e._h, 3, table(three)) == 0
    e.input_classes = E.input_class_table([("f32", 16000), ("mulaw", 8000), ("s16", 48000)])      # what Engine(input_classes=...) keeps
    e._mirror_input_classes()
    back = table([(0, 0)] * 4)
    assert lib.vapx_get_input_classes(e._h, back, 4) == 3 and [(b.input_hz, b.format) for b in back[:3]] == three
    assert [lib.vapx_input_slot_bytes(e._h, c) for c in (0, 1, 2, 3, -1)] == [2 * 800 * 4, 2 * 400 * 1, 2 * 2400 * 2, 0, 0]
    assert [lib.vapx_get_stream_class(e._h, s) for s in range(4)] == [0] * 4
    refused(e, lib.vapx_set_input_classes(e._h, 3, table(three)), -1, "once")
    # a table before vapx_set_input_rate / _format
    refused(e, lib.vapx_set_input_rate(e._h, 8000), -1, "input classes")
    refused(e, lib.vapx_set_input_format(e._h, 1), -1, "input classes")
    # vapx_set_stream_class out of range
    refused(e, lib.vapx_set_stream_class(e._h, 4, 0), -4, "stream id 4")
    refused(e, lib.vapx_set_stream_class(e._h, -1, 0), -4, "stream id -1")
    refused(e, lib.vapx_set_stream_class(e._h, 0, 3), -4, "class 3")
    refused(e, lib.vapx_get_stream_class(e._h, 4), -4, "stream id 4")
    e.set_stream_class(1, 2)
    assert lib.vapx_get_stream_class(e._h, 1) == 2 and e.stream_class(1) == 2
    # the step: samples_per_ch != 0, a misaligned base, VAPX_IDS_DEVICE
    ids = np.array([1, 0], np.int32)
    block = E.aligned_bytes(9600 + 6400 + 16)
    block[:] = 0
    out = np.zeros((2, E.OUT_STRIDE), np.float32)
    refused(e, lib.vapx_step(e._h, 2, ids.ctypes.data, block.ctypes.data, 800, out.ctypes.data, 0, None), -1, "samples_per_ch must be 0")
    refused(e, lib.vapx_step(e._h, 2, ids.ctypes.data, block.ctypes.data + 4, 0, out.ctypes.data, 0, None), -1, "16-byte aligned")
    idt = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    dev, dout = torch.zeros(16000, dtype=torch.uint8, device="cuda"), torch.zeros((2, E.OUT_STRIDE), device="cuda")
    refused(e, lib.vapx_step(e._h, 2, idt.data_ptr(), dev.data_ptr(), 0, dout.data_ptr(), 1 | 2 | 4, None), -1, "VAPX_IDS_DEVICE", "host")
    assert lib.vapx_step(e._h, 2, ids.ctypes.data, block.ctypes.data, 0, out.ctypes.data, 0, None) == 0      # and the step they did not touch
    assert np.isfinite(out).all() and out[0, E.OUT_NVALID] == 1
    with pytest.raises(TypeError, match="int16 samples, not float32"):
        e.step([np.zeros((2, 2400), np.float32), np.zeros((2, 800), np.float32)], [1, 0])
    with pytest.raises(ValueError, match=r"takes \[2, 800\] samples"):
        e.step([np.zeros((2, 2400), np.int16), np.zeros((2, 400), np.float32)], [1, 0])
    # vapx_encode_audio, vapx_export_streams / vapx_import_streams
    fr, emb = torch.zeros((1, 2, 1120), device="cuda"), torch.zeros((1, 2, 256), device="cuda")
    refused(e, lib.vapx_encode_audio(e._h, 1, None, fr.data_ptr(), emb.data_ptr(), None), -1, "input classes")
    rec = np.zeros((1, int(lib.vapx_state_floats(e._h, 0))), np.float32)
    refused(e, lib.vapx_export_streams(e._h, 1, None, rec.ctypes.data, 0, None), -1, "vapx_export_streams", "input classes")
    refused(e, lib.vapx_import_streams(e._h, 1, None, rec.ctypes.data, 0, None), -1, "vapx_import_streams", "input classes")
    # vapx_get_state / vapx_set_state work, as with an input rate
    st = e.get_state(1)
    e.set_state(1, st)
    assert st["n_frames"] == 1
    e.close()
    # a table after a step
    e = _engine(20, max_streams=1)
    e.step(np.zeros((1, 2, 800), np.float32))
    refused(e, lib.vapx_set_input_classes(e._h, 3, table(three)), -1, "before its first step")
    e.close()
    # a table after vapx_set_input_rate / _format
    for kw in ({"input_hz": 8000}, {"input_format": "s16"}):
        e = _engine(20, max_streams=1, **kw)
        refused(e, lib.vapx_set_input_classes(e._h, 3, table(three)), -1, "of its own")
        e.close()
    with pytest.raises(ValueError, match="replaces input_hz / input_format"):
        _engine(20, input_hz=8000, input_classes=[("f32", 16000)])
    # a table on a follower; an engine with a table does not become one
    lead, fol, own = _engine(20, max_streams=1), _engine(20, max_streams=1, mode="bc"), _engine(20, max_streams=1, mode="bc", input_classes=[("s16", 16000)])
    with pytest.raises(E.VapxError, match="input classes of its own"):
        own.attach_trunk(lead)
    fol.attach_trunk(lead)
    refused(fol, lib.vapx_set_input_classes(fol._h, 3, table(three)), -1, "follower", "leader")
    for x in (fol, own, lead):
        x.close()


# ---- 5. the native front-end, end to end --------------------------------------------------------------------------------------------
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


def test_front_end_end_to_end_with_class_ports():
    """Three class ports, two dialogues on each, 10 frames in 10 ms packets of the class.  Every frame is answered, the echo blocks are the
    decoded samples exactly, and the heads agree with a direct mixed-engine run within the project's 1e-4 bar (which rows share a tick is up
    to the receive threads' timing, and a row's last bit depends on the shape of its batch: no bit equality here).  Then a dialogue closes
    and reconnects on another class's port and is served in the new class."""
    import socket
    import time
    from vap_realtime_amd import engine, ingest, pcm, wire
    classes = [("f32", 16000), ("mulaw", 8000), ("s16", 48000)]
    wire_of = {"f32": "f64", "mulaw": "mulaw", "s16": "s16"}
    frame_hz, frames, S = 20, 10, 6
    cls_of = [s // 2 for s in range(S)]                                     # connected in this order: slots 0, 1 class 0; 2, 3 class 1; 4, 5 class 2
    hop_in = [hz // frame_hz for _, hz in classes]
    # float64 samples for the f64 framing (not f32-representable: the host casts), raw samples otherwise
    sig = [np.random.default_rng(40 + s).standard_normal((2, frames * hop_in[0])) * 0.05 if cls_of[s] == 0
           else _raw(classes[cls_of[s]][0], (2, frames * hop_in[cls_of[s]]), seed=40 + s) for s in range(S)]
    dec = [sig[s] if cls_of[s] == 0 else pcm.decode(classes[cls_of[s]][0], sig[s], np.float64) for s in range(S)]      # what the packet echoes
    ref = _engine(frame_hz, max_streams=S, input_classes=classes)           # the same samples, stepped directly on a mixed engine
    for s in range(S):
        ref.set_stream_class(s, cls_of[s])
    want = []
    for f in range(frames):
        arrays = [sig[s][:, f * hop_in[cls_of[s]]:(f + 1) * hop_in[cls_of[s]]] for s in range(S)]
        want.append(engine.split_outputs(ref.step(arrays).copy()))
    ref.close()
    eng = _engine(frame_hz, max_streams=S, input_classes=classes)
    with pytest.raises(engine.VapxError, match="gain with a raw input class"):
        ingest.NativeServer(eng, port_in=0, port_out=0, gain=0.5)
    with pytest.raises(engine.VapxError, match="passive shard"):
        ingest.NativeServer(eng, port_in=-1, port_out=-1)
    srv = ingest.NativeServer(eng, port_in=0, port_out=0, max_wait_s=0.5)
    try:
        assert len(srv.class_ports) == 3 and len(set(srv.class_ports)) == 3
        ins = []
        for s in range(S):                                                  # one after another: the lowest free slot is s
            ins.append(socket.create_connection(("127.0.0.1", srv.class_ports[cls_of[s]])))
            while srv.stats()["in_connections"] < s + 1:
                time.sleep(0.005)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in range(S)]
        while srv.stats()["out_connections"] < S:
            time.sleep(0.01)
        data = [wire.encode_input(sig[s][0], sig[s][1], wire_of[classes[cls_of[s]][0]]) for s in range(S)]
        pkt = [wire.input_packet_bytes(wire_of[f], hz) for f, hz in classes]
        assert pkt == [2560, 160, 1920]
        worst = 0.0
        for f in range(frames):
            for s in range(S):
                pb = pkt[cls_of[s]]
                for p in range(5):
                    ins[s].sendall(data[s][(f * 5 + p) * pb:(f * 5 + p + 1) * pb])
            for s in range(S):
                r = wire.decode_result(_read_packet(outs[s]))
                h = hop_in[cls_of[s]]
                seg = dec[s][:, f * h:(f + 1) * h]
                assert len(r["x1"]) == h and np.array_equal(r["x1"], seg[0]) and np.array_equal(r["x2"], seg[1]), (f, s)
                for k in ("p_now", "p_future", "vad"):
                    worst = max(worst, float(np.abs(np.asarray(r[k], np.float64) - want[f][k][s].astype(np.float64)).max()))
        print(f"class ports through TCP: max |front-end - direct mixed engine| = {worst:.2e}")
        assert worst <= 1e-4
        st = srv.stats()
        assert st["frames_done"] == S * frames and st["numeric_resets"] == 0
        assert st["rx_bytes"] == frames * 5 * 2 * sum(pkt)
        assert [eng.stream_class(s) for s in range(S)] == cls_of
        # stream 0 (f64 at 16 kHz) closes and comes back as a mu-law telephone: served in the new class, from a fresh state
        ins[0].close()
        while srv.stats()["in_connections"] > S - 1:
            time.sleep(0.005)
        ins[0] = socket.create_connection(("127.0.0.1", srv.class_ports[1]))
        while srv.stats()["in_connections"] < S:
            time.sleep(0.005)
        fresh = _engine(frame_hz, max_streams=1, input_hz=8000, input_format="mulaw")      # and the uniform engine of that class agrees
        for f in range(2):
            seg = np.ascontiguousarray(sig[2][:, f * 400:(f + 1) * 400])
            ins[0].sendall(wire.encode_input(seg[0], seg[1], "mulaw"))
            r = wire.decode_result(_read_packet(outs[0]))
            w = engine.split_outputs(fresh.step(seg[None]))
            assert len(r["x1"]) == 400 and np.array_equal(r["x1"], pcm.decode("mulaw", seg[0], np.float64))
            for k in ("p_now", "p_future", "vad"):
                assert np.abs(np.asarray(r[k], np.float64) - w[k][0]).max() <= 1e-4, (f, k)
        fresh.close()
        assert eng.stream_class(0) == 1
    finally:
        srv.close()
        eng.close()
