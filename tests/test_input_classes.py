"""Input classes without a GPU: the packed-block layout (engine.pack_input_classes), the native front-end's class ports over a step
function (vapx_ingest_open_fn with a class table: every class its own input port, the step function sees the packed block an engine
would), the config struct of before the classes, and the refusals of the group / passive front-ends and of ``serve``'s arguments."""
import ctypes as C
import socket
import struct
import time

import numpy as np
import pytest

from vap_realtime_amd import engine, ingest, pcm, wire

CLASSES = [("f64", 16000), ("mulaw", 8000), ("s16", 48000)]       # as a front-end names them; the engine's name of "f64" is "f32"
FRAME_HZ = 20
WIRE_OF = {"f32": "f64", "s16": "s16", "mulaw": "mulaw", "alaw": "alaw"}


def _wait(cond, timeout=5.0):
    t0 = time.time()
    while not cond() and time.time() - t0 < timeout:
        time.sleep(0.005)
    assert cond()


def _recv_exact(sock, n):
    b = b""
    while len(b) < n:
        chunk = sock.recv(n - len(b))
        assert chunk, "socket closed"
        b += chunk
    return b


def _read_result(sock):
    sock.settimeout(10)
    ln = struct.unpack("<I", _recv_exact(sock, 4))[0]
    return wire.decode_result(_recv_exact(sock, ln))


def _signal(cls, frames, seed):
    """[2, frames * hop_in] samples as a client of class ``cls`` holds them: float64 for the f64 framing, raw samples otherwise."""
    fmt, hz = cls
    rng = np.random.default_rng(seed)
    n = frames * (hz // FRAME_HZ)
    if fmt == "f32":
        return rng.standard_normal((2, n)) * 0.1
    if fmt == "s16":
        return rng.integers(-4096, 4096, (2, n)).astype(np.int16)
    return rng.integers(0, 256, (2, n)).astype(np.uint8)


def _as_staged(cls, x):
    """What the front-end stages for a frame of class ``cls``: the f32 cast of the f64 pairs, or the raw samples as they are."""
    return x.astype(np.float32) if cls[0] == "f32" else x


class Recorder:
    """A step function that keeps every tick's ids, classes and packed block, and answers with the slot's byte count in p_now[0]."""

    def __init__(self):
        self.srv, self.ticks, self.resets = None, [], []

    def step(self, ids, audio, out):
        cls = [self.srv.stream_class(int(s)) for s in ids]
        self.ticks.append((ids.tolist(), cls, audio.copy()))
        out[:, 0] = [engine.input_slot_bytes(self.tab[c], FRAME_HZ) for c in cls]
        out[:, 1] = cls
        return 0

    def reset(self, sid):
        self.resets.append(sid)


def test_pack_input_agrees_with_the_layout_rule():
    tab = engine.input_class_table([("f32", 16000), ("mulaw", 8000), ("s16", 48000), ("alaw", 32000)])
    for frame_hz in (50, 5):
        sizes = [engine.input_slot_bytes(c, frame_hz) for c in tab]
        hop_in = [hz // frame_hz for _, hz in tab]
        assert sizes == [2 * hop_in[0] * 4, 2 * hop_in[1], 2 * hop_in[2] * 2, 2 * hop_in[3]] and all(b % 16 == 0 for b in sizes)
        slot_classes = [2, 1, 1, 0, 3, 2, 0]                                # a ragged batch: classes repeat and alternate
        rng = np.random.default_rng(frame_hz)
        arrays = []
        for c in slot_classes:
            dt, shape = engine.input_slot_shape(tab[c], frame_hz)
            assert shape == (2, hop_in[c])
            arrays.append(rng.standard_normal(shape).astype(np.float32) if tab[c][0] == "f32" else rng.integers(0, 200, shape).astype(dt))
        block = engine.pack_input_classes(tab, frame_hz, slot_classes, arrays)
        assert block.dtype == np.uint8 and block.ndim == 1 and block.ctypes.data % 16 == 0 and block.size == sum(sizes[c] for c in slot_classes)
        at = 0
        for c, a in zip(slot_classes, arrays):                              # slot k at the byte offset the earlier slots add up to
            assert at % 16 == 0 and block[at:at + sizes[c]].tobytes() == a.tobytes()      # [2][hop_in]: channel 1's row, then channel 2's
            at += sizes[c]
        out = engine.aligned_bytes(block.size + 64)
        assert engine.pack_input_classes(tab, frame_hz, slot_classes, arrays, out=out).ctypes.data == out.ctypes.data
        # float64 is cast for an f32 class, as Engine.step casts; a raw class takes its own dtype and shape only
        f64 = [a.astype(np.float64) if a.dtype == np.float32 else a for a in arrays]
        assert np.array_equal(engine.pack_input_classes(tab, frame_hz, slot_classes, f64), block)
        with pytest.raises(TypeError, match="batch slot 1: class 1 .mulaw at 8000 Hz. takes uint8 samples, not int16"):
            engine.pack_input_classes(tab, frame_hz, slot_classes, [arrays[0], arrays[0]] + arrays[2:])
        with pytest.raises(ValueError, match="batch slot 0: class 2"):
            engine.pack_input_classes(tab, frame_hz, slot_classes, [arrays[0][:, :-16]] + arrays[1:])
        with pytest.raises(ValueError, match="6 arrays for 7 batch slots"):
            engine.pack_input_classes(tab, frame_hz, slot_classes, arrays[:-1])
    for bad, why in (([("f32", 44100)], "44100"), ([("g722", 16000)], "g722"), ([("s16", 8000)] * 2, "two equal"), ([], "1 .. 16"),
                     ([(f, r) for f in ("f32", "s16", "mulaw", "alaw") for r in (8000, 16000, 32000, 48000)] + [("f32", 8000)], "1 .. 16")):
        with pytest.raises(ValueError, match=why):
            engine.input_class_table(bad)
    assert len(engine.input_class_table([(f, r) for f in (0, 1, 2, 3) for r in (8000, 16000, 32000, 48000)])) == 16       # every combination fits
    assert ingest.parse_input_class("f64@16000:50007") == (("f32", 16000), 50007) and ingest.parse_input_class("mulaw@8000") == (("mulaw", 8000), 0)
    with pytest.raises(ValueError, match="FORMAT@RATE"):
        ingest.parse_input_class("mulaw:8000")


def test_front_end_over_a_step_function_with_class_ports():
    tab = ingest.class_table(CLASSES)
    rec = Recorder()
    rec.tab = tab
    srv = ingest.NativeServer.over_function(rec.step, 6, FRAME_HZ, reset=rec.reset, max_wait_s=0.5, input_classes=CLASSES)
    rec.srv = srv
    frames = 3
    try:
        assert len(srv.class_ports) == 3 and len(set(srv.class_ports)) == 3 and all(p > 0 for p in srv.class_ports) and srv.port_in == srv.class_ports[0]
        # one dialogue per class, connected in the order class 1, 2, 0: slots 0, 1, 2 are of classes 1, 2, 0
        order = [1, 2, 0]
        ins = []
        for k, c in enumerate(order):
            ins.append(socket.create_connection(("127.0.0.1", srv.class_ports[c])))
            _wait(lambda: srv.stats()["in_connections"] == k + 1)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in order]
        _wait(lambda: srv.stats()["out_connections"] == 3)
        sig = [_signal(tab[c], frames, seed=c) for c in order]
        for f in range(frames):
            for k, c in enumerate(order):
                fmt, hz = tab[c]
                hop_in, pkt = hz // FRAME_HZ, wire.input_packet_bytes(WIRE_OF[fmt], hz)
                data = wire.encode_input(sig[k][0, f * hop_in:(f + 1) * hop_in], sig[k][1, f * hop_in:(f + 1) * hop_in], WIRE_OF[fmt])
                assert len(data) == 5 * pkt                                 # 10 ms packets, 5 per 20 Hz frame
                for p in range(5):
                    ins[k].sendall(data[p * pkt:(p + 1) * pkt])
            for k, c in enumerate(order):
                r = _read_result(outs[k])                                   # the k-th output connection hears the k-th stream
                fmt, hz = tab[c]
                hop_in = hz // FRAME_HZ
                seg = sig[k][:, f * hop_in:(f + 1) * hop_in]
                echo = seg if fmt == "f32" else pcm.decode(fmt, seg, np.float64)
                assert len(r["x1"]) == hop_in and np.array_equal(r["x1"], echo[0]) and np.array_equal(r["x2"], echo[1])
                assert r["p_now"][0] == engine.input_slot_bytes(tab[c], FRAME_HZ) and r["p_now"][1] == c
        assert len(rec.ticks) == frames and sorted(rec.resets) == [0, 1, 2]
        for f, (ids, cls, block) in enumerate(rec.ticks):
            assert sorted(ids) == [0, 1, 2] and cls == [order[s] for s in ids]      # vapx_ingest_stream_class: the class of the slot's port
            assert block.dtype == np.uint8 and block.size == sum(engine.input_slot_bytes(tab[c], FRAME_HZ) for c in cls)
            at = 0
            for s, c in zip(ids, cls):                                      # the bytes that were sent, de-interleaved, at the offsets the classes imply
                hop_in = tab[c][1] // FRAME_HZ
                want = _as_staged(tab[c], sig[s][:, f * hop_in:(f + 1) * hop_in])
                nb = engine.input_slot_bytes(tab[c], FRAME_HZ)
                assert block[at:at + nb].tobytes() == np.ascontiguousarray(want).tobytes(), (f, s, c)
                at += nb
        # a connection that closes and reconnects on another class's port is served in the new class: slot 0 (class 1) -> class 2
        ins[0].close()
        _wait(lambda: srv.stats()["in_connections"] == 2)
        ins[0] = socket.create_connection(("127.0.0.1", srv.class_ports[2]))
        _wait(lambda: srv.stats()["in_connections"] == 3)
        x = _signal(tab[2], 1, seed=9)
        ins[0].sendall(wire.encode_input(x[0], x[1], WIRE_OF[tab[2][0]]))
        r = _read_result(outs[0])
        assert len(r["x1"]) == 2400 and np.array_equal(r["x1"], pcm.decode("s16", x[0], np.float64)) and r["p_now"][1] == 2
        ids, cls, block = rec.ticks[-1]
        assert ids == [0] and cls == [2] and block.tobytes() == x.tobytes() and rec.resets.count(0) == 2
        st = srv.stats()
        assert st["frames_done"] == 3 * frames + 1 and st["numeric_resets"] == 0
    finally:
        srv.close()


def test_the_config_struct_of_before_the_classes_opens_a_front_end_as_ever():
    lib = engine.load_library()
    assert C.sizeof(ingest._IngestConfigNoClasses) == 72 and C.sizeof(ingest._IngestConfig) == 72 + 128 + 64
    assert ingest._IngestConfig.n_input_classes.offset == 68             # where the shorter struct has its tail padding
    raw = (C.c_ubyte * 72)(*([0xFF] * 72))                                 # ... which a caller never initialised
    cfg = ingest._IngestConfigNoClasses.from_buffer(raw)
    for name, v in (("struct_size", 72), ("port_in", 0), ("port_out", 0), ("rx_threads", 1), ("tx_threads", 1), ("max_wait_us", 500000), ("min_batch", 0),
                    ("reset_on_connect", 1), ("broadcast", -1), ("bind_any", 0), ("gain", 1.0), ("target_util_pct", 100), ("flags", 0), ("cpu_first", 0),
                    ("cpu_count", 0), ("input_format", 0)):
        setattr(cfg, name, v)
    assert bytes(raw[68:72]) == b"\xff" * 4
    seen = []

    def step(_user, n, ids, audio, out):
        seen.append(np.ctypeslib.as_array(audio, shape=(n, 2, 800)).copy())
        np.ctypeslib.as_array(out, shape=(n, engine.OUT_STRIDE))[:, :engine.OUT_STATUS + 1] = 0.0
        return 0

    fn = ingest._STEP_FN(step)
    h = C.c_void_p()
    assert lib.vapx_ingest_open_fn(C.cast(fn, C.c_void_p), None, None, 1, 1, 20, 0, C.byref(cfg), C.byref(h)) == 0
    try:
        arr = (C.c_int32 * 4)()
        assert lib.vapx_ingest_class_ports(h, arr, 4) == 0 and lib.vapx_ingest_stream_class(h, 0) == -1      # no table
        pin, pout = C.c_int32(0), C.c_int32(0)
        lib.vapx_ingest_ports(h, C.byref(pin), C.byref(pout))
        assert pin.value > 0 and pout.value > 0
        i, o = socket.create_connection(("127.0.0.1", pin.value)), socket.create_connection(("127.0.0.1", pout.value))
        x = np.random.default_rng(1).standard_normal((2, 800))
        i.sendall(wire.encode_input(x[0], x[1]))
        r = _read_result(o)
        assert np.array_equal(r["x1"], x[0]) and np.array_equal(r["x2"], x[1]) and np.array_equal(seen[0][0], x.astype(np.float32))
    finally:
        lib.vapx_ingest_close(h)
    cfg.struct_size = 76                                                    # a size no version of the struct ever had
    assert lib.vapx_ingest_open_fn(C.cast(fn, C.c_void_p), None, None, 1, 1, 20, 0, C.byref(cfg), C.byref(h)) == -1


def test_group_and_passive_front_ends_refuse_a_table():
    def step(ids, audio, out):
        return 0

    with pytest.raises(engine.VapxError, match="passive shard"):           # a shard behind a front door
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, port_in=-1, port_out=-1, input_classes=CLASSES)
    lib = engine.load_library()
    cfg = ingest.NativeServer._cfg(0, 0, 1.0, 0.002, 0, True, None, 0, 0, False, input_classes=CLASSES)
    fn = ingest._STEP_FN(lambda *a: 0)
    modes, h = (C.c_int32 * 2)(0, 1), C.c_void_p()
    rc = lib.vapx_ingest_open_group_fn(C.cast(fn, C.c_void_p), None, None, 2, 2, 20, 50, modes, 2, C.byref(cfg), None, C.byref(h))
    assert rc == -1 and b"trunk group's front-end takes no input classes" in lib.vapx_ingest_last_open_error()
    # what a table may not come with
    with pytest.raises(engine.VapxError, match="gain with a raw input class"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, gain=0.5, input_classes=CLASSES)
    with pytest.raises(engine.VapxError, match="input_format together with input classes"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, input_format="s16", input_classes=CLASSES)
    with pytest.raises(ValueError, match="3 input classes need 3 input ports"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, input_classes=CLASSES, class_ports=[0, 0])
    srv = ingest.NativeServer.over_function(step, 2, FRAME_HZ, gain=0.5, input_classes=[("f64", 16000), ("f64", 8000)])      # no raw class: the gain is fine
    assert len(srv.class_ports) == 2
    srv.close()


@pytest.mark.parametrize("extra,why", [
    (["--input_rate", "8000"], "every class names its own rate"),
    (["--input_format", "s16"], "every class names its own format"),
    (["--mode", "vap+bc"], "the group front-end has one input port"),
    (["--gpus", "2"], "the front door has one input port"),
    (["--save_state", "state.bin"], "state records of an engine with input classes do not exist yet"),
    (["--load_state", "state.bin"], "state records of an engine with input classes do not exist yet"),
    (["--input_class", "mulaw@8000:50018"], "two equal"),
    (["--input_class", "g722@16000"], "g722"),
])
def test_serve_refuses_what_input_classes_do_not_go_with(extra, why, capsys):
    from vap_realtime_amd import serve
    with pytest.raises(SystemExit) as e:
        serve.main(["--input_class", "f64@16000:50007", "--input_class", "mulaw@8000:50017", "--synthetic-weights", "0"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert why in err and len([ln for ln in err.splitlines() if "error:" in ln]) == 1      # its own one-line reason


def test_class_ports_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/native/input_classes_san.cpp: the front-end compiled into ONE stand-alone program with stubs of the engine, opened over a step
    function with a class table and driven by loopback clients on three class ports (steady traffic, reconnects on another class's port in
    the middle of a frame, a close under load).  Any sanitizer report fails the test; no GPU, nothing loaded into Python."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.fail("g++ not on PATH: the front-end's host code cannot be checked")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "input_classes_san.cpp")
    exe = tmp_path / "input_classes_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wno-subobject-linkage", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-o", str(exe), src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    for m in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert m not in log, log[-6000:]
    assert r.returncode == 0 and "ok: 12 dialogues on 3 class ports" in log and "bad blocks 0" in log, log[-3000:]
