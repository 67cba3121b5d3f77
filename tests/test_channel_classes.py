"""Input classes per channel without a GPU: the packed block with a class per channel (engine.pack_input_classes with pairs), the
``A+B[:PORT]`` syntax of ``serve --input_class`` and the table it derives, the native front-end's PAIR ports over a step function
(vapx_ingest_open_fn: planar packets arrive in the step function as the packed block an engine would take), a reconnect on another
port in the middle of a frame, and the config structs of before the pair ports."""
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


def _leg(cls, frames, seed):
    """[frames * hop_in] samples of one channel as a client of class ``cls`` holds them: float64 for the f64 framing, raw otherwise."""
    fmt, hz = cls
    rng = np.random.default_rng(seed)
    n = frames * (hz // FRAME_HZ)
    if fmt == "f32":
        return rng.standard_normal(n) * 0.1
    if fmt == "s16":
        return rng.integers(-4096, 4096, n).astype(np.int16)
    return rng.integers(0, 256, n).astype(np.uint8)


def _staged(cls, x):
    """The bytes the front-end stages for a channel's row: the f32 cast of the f64 samples, or the raw samples as they are."""
    return (x.astype(np.float32) if cls[0] == "f32" else x).tobytes()


def _echo(cls, x):
    return x if cls[0] == "f32" else pcm.decode(cls[0], x, np.float64)


# ---- 1. the packed block ----------------------------------------------------------------------------------------------------------
def test_pack_input_with_a_class_per_channel():
    tab = engine.input_class_table([("f32", 16000), ("mulaw", 8000), ("s16", 48000), ("alaw", 32000)])
    for frame_hz in (50, 20, 5):
        row = [engine.input_row_bytes(c, frame_hz) for c in tab]
        assert row == [16000 // frame_hz * 4, 8000 // frame_hz, 48000 // frame_hz * 2, 32000 // frame_hz] and all(b % 16 == 0 for b in row)
        assert [2 * b for b in row] == [engine.input_slot_bytes(c, frame_hz) for c in tab]
        # a mixed slot is never larger than the largest same-class slot: staging, LDS and the 4 GiB rule of the table stand
        assert max(row[a] + row[b] for a in range(4) for b in range(4)) == 2 * max(row)
        rng = np.random.default_rng(frame_hz)

        def leg(c):
            dt, (_, hop_in) = engine.input_slot_shape(tab[c], frame_hz)
            return rng.standard_normal(hop_in).astype(np.float32) if dt == np.float32 else rng.integers(0, 100, hop_in).astype(dt)

        slots = [(0, 1), (1, 0), (2, 1), (1, 2), (3, 2), 1, (2, 2), (0, 3)]
        arrays = [np.stack([leg(c), leg(c)]) if isinstance(c, int) else (leg(c[0]), leg(c[1])) for c in slots]
        block = engine.pack_input_classes(tab, frame_hz, slots, arrays)
        assert block.dtype == np.uint8 and block.ndim == 1 and block.ctypes.data % 16 == 0
        at = 0
        for c, a in zip(slots, arrays):                                     # channel 1's row, then channel 2's, slots back to back
            for ch, k in enumerate((c, c) if isinstance(c, int) else c):
                assert at % 16 == 0
                want = np.ascontiguousarray(a[ch]).tobytes()
                assert len(want) == row[k] and block[at:at + row[k]].tobytes() == want, (c, ch)
                at += row[k]
        assert at == block.size
        # c1 == c2: a pair of 1-D arrays, a pair (c, c) and today's [2, hop_in] array under a class index give the same bytes
        same = [1, 2, 0, 3]
        two_d = [np.stack([leg(c), leg(c)]) for c in same]
        today = engine.pack_input_classes(tab, frame_hz, same, two_d)
        assert today.tobytes() == b"".join(a.tobytes() for a in two_d)     # which is the layout of before: [2][hop_in] per slot
        assert np.array_equal(engine.pack_input_classes(tab, frame_hz, [(c, c) for c in same], [(a[0], a[1]) for a in two_d]), today)
        assert np.array_equal(engine.pack_input_classes(tab, frame_hz, [(c, c) for c in same], two_d), today)
        assert np.array_equal(engine.pack_input_classes(tab, frame_hz, same, [(a[0], a[1]) for a in two_d]), today)
        out = engine.aligned_bytes(block.size + 64)
        assert engine.pack_input_classes(tab, frame_hz, slots, arrays, out=out).ctypes.data == out.ctypes.data
        f64 = [tuple(x.astype(np.float64) if x.dtype == np.float32 else x for x in a) if isinstance(a, tuple) else a for a in arrays]
        assert np.array_equal(engine.pack_input_classes(tab, frame_hz, slots, f64), block)      # float64 is cast for an f32 class
        with pytest.raises(TypeError, match="batch slot 0: channel classes .0, 1. take a pair of 1-D arrays"):
            engine.pack_input_classes(tab, frame_hz, slots, [np.zeros((2, 16), np.float32)] + arrays[1:])
        with pytest.raises(TypeError, match="batch slot 0: class 1 .mulaw at 8000 Hz. takes uint8 samples, not float32"):
            engine.pack_input_classes(tab, frame_hz, slots, [(arrays[0][0], arrays[0][0])] + arrays[1:])
        with pytest.raises(ValueError, match="batch slot 2: class 1 .mulaw at 8000 Hz. takes"):
            engine.pack_input_classes(tab, frame_hz, slots, arrays[:2] + [(arrays[2][0], arrays[2][1][:-16])] + arrays[3:])
        with pytest.raises(ValueError, match="one index or a pair"):
            engine.pack_input_classes(tab, frame_hz, [(0, 1, 2)], arrays[:1])
        with pytest.raises(ValueError, match="two entries"):
            engine.pack_input_classes(tab, frame_hz, [(0, 1)], [(arrays[0][0],)])


# ---- 2. A+B[:PORT] -----------------------------------------------------------------------------------------------------------------
def test_parsing_pair_ports_and_the_derived_table():
    assert ingest.parse_input_port("mulaw@8000:50017") == ([("mulaw", 8000)], 50017)
    assert ingest.parse_input_port("s16@48000+mulaw@8000:50037") == ([("s16", 48000), ("mulaw", 8000)], 50037)
    assert ingest.parse_input_port("f64@16000+f64@16000") == ([("f32", 16000), ("f32", 16000)], 0)
    for bad in ("s16@48000+mulaw:50037", "s16@48000+mulaw@8000+alaw@8000", "s16@48000+mulaw@8000:x", "s16@48000+", "+"):
        with pytest.raises(ValueError, match="FORMAT@RATE"):
            ingest.parse_input_port(bad)
    with pytest.raises(ValueError, match="g722"):
        ingest.parse_input_port("s16@48000+g722@8000")
    with pytest.raises(ValueError, match="44100"):
        ingest.parse_input_port("s16@44100+mulaw@8000")
    # the table: the distinct classes named anywhere, in order of first appearance; a class only pair ports name gets an ephemeral port
    tab, cports, pports = ingest.input_ports(["f64@16000:50007", "s16@48000+mulaw@8000:50037", "mulaw@8000:50017", "mulaw@8000+s16@48000",
                                              "alaw@32000+alaw@32000:50047"])
    assert tab == [("f32", 16000), ("s16", 48000), ("mulaw", 8000), ("alaw", 32000)]
    assert cports == [50007, 0, 50017, 0] and pports == [(1, 2, 50037), (2, 1, 0), (3, 3, 50047)]
    assert ingest.input_ports(["f64@16000:50007", "mulaw@8000"]) == ([("f32", 16000), ("mulaw", 8000)], [50007, 0], [])      # as before
    with pytest.raises(ValueError, match="two equal"):
        ingest.input_ports(["mulaw@8000:1", "mulaw@8000:2"])
    with pytest.raises(ValueError, match="two equal"):
        ingest.input_ports(["s16@48000+mulaw@8000:1", "s16@48000+mulaw@8000:2"])
    with pytest.raises(ValueError, match="at most 16"):
        ingest.input_ports([f"{a}@8000+{b}@{r}" for a in ("s16", "mulaw", "alaw") for b in ("s16", "mulaw", "alaw") for r in (8000, 16000)])
    # planar packets
    x1, x2 = np.arange(160, dtype=np.uint8), (np.arange(960) - 480).astype(np.int16)
    data = wire.encode_input_planar(x1, ("mulaw", 8000), x2, ("s16", 48000))
    assert len(data) == 2 * (80 + 960) and data[:80] == x1[:80].tobytes() and data[80:1040] == x2[:480].tobytes() and data[1040:1120] == x1[80:].tobytes()
    f = np.linspace(-1, 1, 320)
    data = wire.encode_input_planar(f, ("f64", 16000), x1, ("alaw", 8000))
    assert len(data) == 2 * (1280 + 80) and data[:1280] == f[:160].astype("<f8").tobytes() and data[1280:1360] == x1[:80].tobytes()
    with pytest.raises(ValueError, match="10 ms"):
        wire.encode_input_planar(x1[:100], ("mulaw", 8000), x2, ("s16", 48000))
    with pytest.raises(ValueError, match="packets"):
        wire.encode_input_planar(x1[:80], ("mulaw", 8000), x2, ("s16", 48000))


@pytest.mark.parametrize("extra,why", [
    (["--input_rate", "8000"], "every class names its own rate"),
    (["--input_format", "s16"], "every class names its own format"),
    (["--mode", "vap+bc"], "the group front-end has one input port"),
    (["--gpus", "2"], "the front door has one input port"),
    (["--save_state", "state.bin"], "state records of an engine with input classes do not exist yet"),
    (["--load_state", "state.bin"], "state records of an engine with input classes do not exist yet"),
    (["--input_class", "s16@48000+mulaw@8000:50038"], "two equal"),
    (["--input_class", "s16@48000+g722@16000"], "g722"),
    (["--input_class", "s16@48000+mulaw@8000+alaw@8000"], "FORMAT@RATE+FORMAT@RATE[:PORT]"),
])
def test_serve_refuses_with_a_pair_port_what_it_refuses_with_a_class_port(extra, why, capsys):
    from vap_realtime_amd import serve
    with pytest.raises(SystemExit) as e:
        serve.main(["--input_class", "f64@16000:50007", "--input_class", "s16@48000+mulaw@8000:50037", "--synthetic-weights", "0"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert why in err and len([ln for ln in err.splitlines() if "error:" in ln]) == 1      # its own one-line reason


# ---- 3. pair ports over a step function ------------------------------------------------------------------------------------------------
class Recorder:
    """A step function that keeps every tick's ids, channel classes and packed block, and answers with the slot's bytes and classes."""

    def __init__(self, tab):
        self.srv, self.tab, self.ticks, self.resets = None, tab, [], []

    def step(self, ids, audio, out):
        cls = [self.srv.stream_channel_classes(int(s)) for s in ids]
        self.ticks.append((ids.tolist(), cls, audio.copy()))
        out[:, 0] = [sum(engine.input_row_bytes(self.tab[c], FRAME_HZ) for c in pair) for pair in cls]
        out[:, 1] = [10 * a + b for a, b in cls]
        return 0

    def reset(self, sid):
        self.resets.append(sid)


def test_pair_ports_over_a_step_function():
    """Slots 0 and 1 connect on the pair ports (mulaw@8000, s16@48000) and (f64@16000, mulaw@8000), slot 2 on a pair port of one class twice
    (planar all the same), slot 3 on the plain class port of s16@48000 (interleaved, as ever)."""
    tab = ingest.class_table(CLASSES)
    rec = Recorder(tab)
    pairs = [(1, 2, 0), (0, 1, 0), (1, 1, 0)]
    srv = ingest.NativeServer.over_function(rec.step, 6, FRAME_HZ, reset=rec.reset, max_wait_s=0.5, input_classes=CLASSES, pair_ports=pairs)
    rec.srv = srv
    frames = 3
    try:
        assert len(srv.pair_ports) == 3 and len(set(srv.pair_ports + srv.class_ports)) == 6 and all(p > 0 for p in srv.pair_ports)
        of = [(1, 2), (0, 1), (1, 1), (2, 2)]                                # the channel classes of slots 0 .. 3
        ports = srv.pair_ports + [srv.class_ports[2]]
        ins = []
        for k, port in enumerate(ports):
            ins.append(socket.create_connection(("127.0.0.1", port)))
            _wait(lambda: srv.stats()["in_connections"] == k + 1)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in ports]
        _wait(lambda: srv.stats()["out_connections"] == 4)
        sig = [[_leg(tab[c], frames, seed=10 * k + ch) for ch, c in enumerate(of[k])] for k in range(4)]
        data = [wire.encode_input_planar(sig[k][0], tab[of[k][0]], sig[k][1], tab[of[k][1]]) for k in range(3)]
        data.append(wire.encode_input(sig[3][0], sig[3][1], "s16"))
        pkt = [80 + 960, 1280 + 80, 80 + 80, 1920]
        assert [len(d) for d in data] == [frames * 5 * b for b in pkt]
        for f in range(frames):
            for k in range(4):
                if k == 1:                                                  # in pieces that split packets, channels and f64 samples
                    chunk = data[k][f * 5 * pkt[k]:(f + 1) * 5 * pkt[k]]
                    for a in range(0, len(chunk), 333):
                        ins[k].sendall(chunk[a:a + 333])
                else:
                    for p in range(5):                                      # 10 ms packets, 5 per 20 Hz frame
                        ins[k].sendall(data[k][(f * 5 + p) * pkt[k]:(f * 5 + p + 1) * pkt[k]])
            for k in range(4):
                r = _read_result(outs[k])                                   # the k-th output connection hears the k-th stream
                hops = [tab[c][1] // FRAME_HZ for c in of[k]]
                legs = [sig[k][ch][f * hops[ch]:(f + 1) * hops[ch]] for ch in range(2)]
                assert len(r["x1"]) == hops[0] and len(r["x2"]) == hops[1]  # each echo block with its own count
                assert np.array_equal(r["x1"], _echo(tab[of[k][0]], legs[0])) and np.array_equal(r["x2"], _echo(tab[of[k][1]], legs[1])), (f, k)
                assert r["p_now"][0] == sum(engine.input_row_bytes(tab[c], FRAME_HZ) for c in of[k]) and r["p_now"][1] == 10 * of[k][0] + of[k][1]
        assert len(rec.ticks) == frames and sorted(rec.resets) == [0, 1, 2, 3]
        for f, (ids, cls, block) in enumerate(rec.ticks):
            assert sorted(ids) == [0, 1, 2, 3] and cls == [of[s] for s in ids]
            at = 0
            for s in ids:                                                   # the documented packed block: channel 1's row, then channel 2's
                for ch, c in enumerate(of[s]):
                    hop_in = tab[c][1] // FRAME_HZ
                    want = _staged(tab[c], sig[s][ch][f * hop_in:(f + 1) * hop_in])
                    assert len(want) == engine.input_row_bytes(tab[c], FRAME_HZ) and block[at:at + len(want)].tobytes() == want, (f, s, ch)
                    at += len(want)
            assert at == block.size
        assert srv.stream_class(2) == 1 and srv.stream_class(3) == 2
        with pytest.raises(engine.VapxError, match="channels differ"):
            srv.stream_class(0)
        # slot 0 sends two packets and a half of a frame, closes, and comes back on the OTHER pair port: the half frame is dropped, the new
        # connection's first frame is served in the new classes from its first byte
        ins[0].sendall(data[0][:2 * pkt[0] + 500])
        ins[0].close()
        _wait(lambda: srv.stats()["in_connections"] == 3)
        assert srv.stats()["rx_bytes"] == frames * 5 * sum(pkt) + 2 * pkt[0] + 500      # read, staged as a part of a frame, and dropped
        ins[0] = socket.create_connection(("127.0.0.1", srv.pair_ports[1]))
        _wait(lambda: srv.stats()["in_connections"] == 4)
        x = [_leg(tab[0], 1, seed=90), _leg(tab[1], 1, seed=91)]
        ins[0].sendall(wire.encode_input_planar(x[0], tab[0], x[1], tab[1]))
        r = _read_result(outs[0])
        assert len(r["x1"]) == 800 and len(r["x2"]) == 400 and np.array_equal(r["x1"], x[0]) and np.array_equal(r["x2"], _echo(tab[1], x[1]))
        ids, cls, block = rec.ticks[-1]
        assert ids == [0] and cls == [(0, 1)] and block.tobytes() == _staged(tab[0], x[0]) + _staged(tab[1], x[1]) and rec.resets.count(0) == 2
        st = srv.stats()
        assert st["frames_done"] == 4 * frames + 1 and st["numeric_resets"] == 0
    finally:
        srv.close()


# ---- 4. what a table refuses, a pair port refuses; the structs of before ------------------------------------------------------------------
def test_refusals_and_the_config_structs_of_before_the_pair_ports():
    def step(ids, audio, out):
        return 0

    assert C.sizeof(ingest._IngestConfigNoClasses) == 72 and C.sizeof(ingest._IngestConfig) == 72 + 128 + 64
    assert C.sizeof(ingest._IngestConfigPairs) == 72 + 128 + 64 + 8 + 16 * 12 and ingest._IngestConfigPairs.n_pair_ports.offset == 264
    with pytest.raises(engine.VapxError, match="pair_ports without input classes"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, pair_ports=[(0, 0, 0)])
    with pytest.raises(engine.VapxError, match="not an index into the table"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, input_classes=CLASSES, pair_ports=[(0, 3, 0)])
    with pytest.raises(engine.VapxError, match="must be >= 0"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, input_classes=CLASSES, pair_ports=[(0, 1, -1)])
    with pytest.raises(ValueError, match="at most 16"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, input_classes=CLASSES, pair_ports=[(0, 1, 0)] * 17)
    with pytest.raises(engine.VapxError, match="passive shard"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, port_in=-1, port_out=-1, input_classes=CLASSES, pair_ports=[(0, 1, 0)])
    with pytest.raises(engine.VapxError, match="gain with a raw input class"):
        ingest.NativeServer.over_function(step, 2, FRAME_HZ, gain=0.5, input_classes=CLASSES, pair_ports=[(0, 1, 0)])
    lib = engine.load_library()
    cfg = ingest.NativeServer._cfg(0, 0, 1.0, 0.002, 0, True, None, 0, 0, False, input_classes=CLASSES, pair_ports=[(0, 1, 0)])
    assert cfg.struct_size == C.sizeof(ingest._IngestConfigPairs)
    fn = ingest._STEP_FN(lambda *a: 0)
    modes, h = (C.c_int32 * 2)(0, 1), C.c_void_p()
    rc = lib.vapx_ingest_open_group_fn(C.cast(fn, C.c_void_p), None, None, 2, 2, 20, 50, modes, 2, C.byref(cfg), None, C.byref(h))
    assert rc == -1 and b"trunk group's front-end takes no input classes" in lib.vapx_ingest_last_open_error()
    # every struct size of before still opens and means "no pair ports": the bytes behind it are never read
    for size, table in ((72, 0), (72 + 128 + 64, 3)):
        raw = (C.c_ubyte * C.sizeof(ingest._IngestConfigPairs))(*([0xFF] * C.sizeof(ingest._IngestConfigPairs)))
        cfg = ingest._IngestConfigPairs.from_buffer(raw)
        for name, v in (("struct_size", size), ("port_in", 0), ("port_out", 0), ("rx_threads", 1), ("tx_threads", 1), ("max_wait_us", 500000),
                        ("min_batch", 0), ("reset_on_connect", 1), ("broadcast", -1), ("bind_any", 0), ("gain", 1.0), ("target_util_pct", 100),
                        ("flags", 0), ("cpu_first", 0), ("cpu_count", 0), ("input_format", 0)):
            setattr(cfg, name, v)
        if table:
            cfg.n_input_classes = table
            for i, (f, hz) in enumerate(ingest.class_table(CLASSES)):
                cfg.input_classes[i] = engine._InputClass(hz, pcm.FORMATS[f])
                cfg.class_ports_in[i] = 0
        assert cfg.n_pair_ports == -1                                       # what a caller of the shorter struct never initialised
        h = C.c_void_p()
        assert lib.vapx_ingest_open_fn(C.cast(fn, C.c_void_p), None, None, 2, 2, 20, 0, C.byref(cfg), C.byref(h)) == 0, size
        arr, two = (C.c_int32 * 16)(), (C.c_int32 * 2)(7, 7)
        assert lib.vapx_ingest_pair_ports(h, arr, 16) == 0 and lib.vapx_ingest_class_ports(h, arr, 16) == table
        assert lib.vapx_ingest_stream_channel_classes(h, 0, two) == (0 if table else -1) and list(two) == ([0, 0] if table else [7, 7])
        assert lib.vapx_ingest_stream_channel_classes(h, 2, two) == (-4 if table else -1)
        lib.vapx_ingest_close(h)
    cfg.struct_size = 72 + 128 + 64 + 8                                     # a size no version of the struct ever had
    assert lib.vapx_ingest_open_fn(C.cast(fn, C.c_void_p), None, None, 2, 2, 20, 0, C.byref(cfg), C.byref(h)) == -1


# ---- 5. the host code of the pair ports under sanitizers, in a program of its own ------------------------------------------------------
def test_pair_ports_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/native/channel_classes_san.cpp: the front-end compiled into ONE stand-alone program with stubs of the engine, opened over a step
    function with a class table and three pair ports, and driven by loopback clients whose planar packets arrive in odd-sized pieces
    (steady traffic, reconnects on another port in the middle of a frame and of a sample, a close under load).  Any sanitizer report fails
    the test; no GPU, nothing loaded into Python."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.fail("g++ not on PATH: the front-end's host code cannot be checked")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "channel_classes_san.cpp")
    exe = tmp_path / "channel_classes_san"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wno-subobject-linkage", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-o", str(exe), src], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    for m in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert m not in log, log[-6000:]
    assert r.returncode == 0 and "ok: 12 dialogues on 3 pair ports and a class port" in log and "bad blocks 0" in log, log[-3000:]
