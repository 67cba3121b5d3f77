"""Input as 16-bit PCM and G.711 mu-law / A-law, the host side (no GPU): the definition (vap-realtime_amd/pcm.py) against the closed forms
and the standard library, the generated csrc/pcm_tables.h, the client-side codec of wire.py, and the native front-end over a stub step
function with ``input_format`` s16 and mulaw — the step must receive exactly the raw samples the clients sent, de-interleaved, and the result
packets must echo their decoded values.  tests/test_pcm_gpu.py holds the kernel and the engine."""
import os
import shutil
import socket
import struct
import subprocess
import time

import numpy as np
import pytest

from vap_realtime_amd import engine, ingest, pcm, wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = np.arange(256, dtype=np.uint8)
ALL16 = np.arange(-32768, 32768).astype(np.int16)


# ---- 1. the definition ---------------------------------------------------------------------------------------------------------------
def _mulaw_closed(c):
    c = ~c & 0xFF
    e, m = (c >> 4) & 7, c & 15
    t = (((m << 3) + 0x84) << e) - 0x84
    return -t if c & 0x80 else t


def _alaw_closed(c):
    c = c ^ 0x55
    e, m = (c >> 4) & 7, c & 15
    t = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return t if c & 0x80 else -t


def test_tables_equal_the_closed_forms_and_the_anchors():
    assert pcm.FORMATS == {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}
    assert pcm.BYTES_PER_SAMPLE == {"f32": 4, "s16": 2, "mulaw": 1, "alaw": 1}
    assert pcm.MULAW.dtype == pcm.ALAW.dtype == np.int16 and pcm.MULAW.shape == pcm.ALAW.shape == (256,)
    assert pcm.MULAW.tolist() == [_mulaw_closed(c) for c in range(256)]
    assert pcm.ALAW.tolist() == [_alaw_closed(c) for c in range(256)]
    U, A = pcm.MULAW, pcm.ALAW
    assert (U[0x00], U[0x80], U[0x7F], U[0xFF]) == (-32124, 32124, 0, 0) and len(set(U.tolist())) == 255
    assert (A[0xD5], A[0x55], A[0xAA], A[0x2A]) == (8, -8, 32256, -32256) and len(set(A.tolist())) == 256


def test_tables_equal_audioop():
    audioop = pytest.importorskip("audioop")
    raw = CODES.tobytes()
    assert np.frombuffer(audioop.ulaw2lin(raw, 2), dtype="<i2").tolist() == pcm.MULAW.tolist()
    assert np.frombuffer(audioop.alaw2lin(raw, 2), dtype="<i2").tolist() == pcm.ALAW.tolist()


def test_every_value_is_exact_and_zero_is_positive():
    for fmt, raw in (("s16", ALL16), ("mulaw", CODES), ("alaw", CODES)):
        f32, f64 = pcm.decode(fmt, raw), pcm.decode(fmt, raw, np.float64)
        assert f32.dtype == np.float32 and f64.dtype == np.float64
        lin = pcm.linear(fmt, raw).astype(np.int64)
        assert np.array_equal(f32.astype(np.float64), f64) and np.array_equal(f64 * 32768.0, lin.astype(np.float64))     # no rounding anywhere
        assert not np.signbit(f32[lin == 0]).any() and not np.signbit(f64[lin == 0]).any()
    assert (pcm.linear("mulaw", CODES) == 0).sum() == 2 and (pcm.linear("s16", ALL16) == 0).sum() == 1
    with pytest.raises(TypeError, match="int16"):
        pcm.decode("s16", CODES)
    with pytest.raises(ValueError, match="g722"):
        pcm.format_id("g722")


def test_generated_header_is_what_pcm_py_writes():
    path = os.path.join(ROOT, "vap-realtime_amd", "csrc", "pcm_tables.h")
    text = open(path).read()
    assert text == pcm.tables_header_text()
    for name, table in (("MULAW", pcm.MULAW), ("ALAW", pcm.ALAW)):          # and the text holds the 256 values, in code order
        body = text[text.index(f"#define VAPX_PCM_{name}_TABLE"):].split("\n#define")[0].split("TABLE", 1)[1]
        assert [int(v) for v in body.replace("\\", " ").replace(",", " ").split()] == table.tolist()


# ---- 2. the client-side codec --------------------------------------------------------------------------------------------------------
def test_wire_round_trip_every_code_and_every_int16():
    for fmt, raw in (("s16", ALL16), ("mulaw", CODES), ("alaw", CODES)):
        values = pcm.decode(fmt, raw, np.float64)
        # a client that holds floats: encode -> decode gives the floats back, for every value the format can hold
        data = wire.encode_input(values, values[::-1], fmt)
        assert len(data) == 2 * raw.size * pcm.BYTES_PER_SAMPLE[fmt]
        x1, x2 = wire.decode_input(data, fmt)
        assert x1.dtype == np.float64 and np.array_equal(x1, values) and np.array_equal(x2, values[::-1])
        # a client that holds raw samples: they travel as they are (mu-law's second zero code 0x7F included)
        data = wire.encode_input(raw, raw[::-1].copy(), fmt)
        got = np.frombuffer(data, dtype=pcm.DTYPES[fmt]).reshape(-1, 2)
        assert np.array_equal(got[:, 0], raw) and np.array_equal(got[:, 1], raw[::-1])
        x1, x2 = wire.decode_input(data, fmt)
        assert np.array_equal(x1, values) and np.array_equal(x2, values[::-1])
    # the encoder picks the codes themselves, except mu-law's negative zero
    assert np.array_equal(pcm.encode("alaw", pcm.decode("alaw", CODES, np.float64)), CODES)
    back = pcm.encode("mulaw", pcm.decode("mulaw", CODES, np.float64))
    assert back[0x7F] == 0xFF and np.array_equal(np.delete(back, 0x7F), np.delete(CODES, 0x7F))
    # f64 is what it was
    x = np.linspace(-1, 1, 160)
    assert wire.encode_input(x, -x, "f64") == wire.encode_input(x, -x) and len(wire.encode_input(x, -x)) == 2560
    with pytest.raises(ValueError, match="multiple of 4"):
        wire.decode_input(b"\0" * 6, "s16")
    with pytest.raises(ValueError, match="opus"):
        wire.encode_input(x, x, "opus")
    # integers that are not the format's samples are refused by name, not scaled as if they were floats
    for fmt, bad in (("mulaw", ALL16[:4]), ("alaw", ALL16[:4]), ("s16", CODES[:4]), ("s16", np.arange(4))):
        with pytest.raises(TypeError, match=f"{fmt} input: raw samples are {pcm.DTYPES[fmt].name}.*{bad.dtype.name} is neither"):
            wire.encode_input(bad, bad, fmt)


def test_g711_encoder_nearest_value_ties_to_the_smaller_magnitude():
    for fmt in ("mulaw", "alaw"):
        table = pcm.TABLES[fmt].astype(np.int64)
        v = np.arange(-32768, 32768)
        got = table[pcm.encode(fmt, v / 32768.0)]
        dist = np.abs(table[None, :] - v[:, None])                         # [65536, 256]
        best = dist.min(axis=1)
        assert np.array_equal(np.abs(got - v), best)                        # a nearest value ...
        tied = dist == best[:, None]
        smallest = np.where(tied, np.abs(table)[None, :], 1 << 20).min(axis=1)
        assert np.array_equal(np.abs(got), smallest)                        # ... and among equally near ones the smaller magnitude
        assert (tied.sum(axis=1) > 1).any()


def test_packet_sizes():
    want = {("f64", 16000): 2560, ("s16", 8000): 320, ("s16", 16000): 640, ("s16", 48000): 1920,
            ("mulaw", 8000): 160, ("mulaw", 16000): 320, ("mulaw", 48000): 960, ("alaw", 8000): 160, ("alaw", 16000): 320, ("alaw", 48000): 960}
    for (fmt, hz), n in want.items():
        assert wire.input_packet_bytes(fmt, hz) == n
        x = np.zeros(hz // 100)
        assert len(wire.encode_input(x, x, fmt)) == n                       # 10 ms of (ch1, ch2) pairs


# ---- 3. the native front-end over a stub step function ------------------------------------------------------------------------------
class RawModel:
    """Keeps every block the step receives; p_now = the mean of each channel's 16-bit linear values."""

    def __init__(self, fmt):
        self.fmt, self.blocks = fmt, []

    def step(self, ids, audio, out):
        self.blocks.append((ids.tolist(), audio.copy()))
        out[:, 0:2] = pcm.linear(self.fmt, audio).astype(np.float64).mean(axis=2)
        return 0


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
    return ln, wire.decode_result(_recv_exact(sock, ln))


def _wait(cond, timeout=5.0):
    t0 = time.time()
    while not cond() and time.time() - t0 < timeout:
        time.sleep(0.005)
    assert cond()


def _raw_signal(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        x = rng.integers(-32768, 32768, (2, 2, n)).astype(np.int16)
        x[0, 0, :4] = [-32768, 32767, 0, -1]
    else:
        x = rng.integers(0, 256, (2, 2, n)).astype(np.uint8)
        x[0, 0, :256], x[1, 1, :256] = CODES, CODES[::-1]                   # every code, both zero codes among them
    return x


@pytest.mark.parametrize("fmt", ["s16", "mulaw"])
def test_front_end_hands_the_raw_samples_to_the_step_and_echoes_their_values(fmt):
    hop, frames = 800, 3
    pkt = wire.input_packet_bytes(fmt)                                      # 640 / 320 bytes per 10 ms
    pair = wire.PAIR_BYTES[fmt]
    m = RawModel(fmt)
    srv = ingest.NativeServer.over_function(m.step, 4, 20, max_wait_s=0.5, input_format=fmt)
    try:
        ins = [socket.create_connection(("127.0.0.1", srv.port_in)) for _ in range(2)]
        _wait(lambda: srv.stats()["in_connections"] == 2)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in range(2)]
        _wait(lambda: srv.stats()["out_connections"] == 2)
        x = _raw_signal(fmt, frames * hop, 11)
        for f in range(frames):
            for s in range(2):
                data = wire.encode_input(x[s, 0, f * hop:(f + 1) * hop], x[s, 1, f * hop:(f + 1) * hop], fmt)
                assert len(data) == 5 * pkt == hop * pair
                if f == 0:                                                  # 10 ms packets
                    for p in range(5):
                        ins[s].sendall(data[p * pkt:(p + 1) * pkt])
                elif f == 1:
                    # packets of other lengths, as a short f64 packet is handled: the bytes are a stream, a sample pair split across two
                    # packets is put together, and a frame is complete when its last byte is there — not before
                    cuts = (0, 1, pair + 1, 3 * pkt - 1, 3 * pkt + pair // 2, len(data) - 1)
                    for a, b in zip(cuts[:-1], cuts[1:]):
                        ins[s].sendall(data[a:b])
                        time.sleep(0.002)
                    if s == 1:                                              # both dialogues are a byte short: the byte completes the frame
                        for k in range(2):                                  # (a tick on less would show as an extra block below)
                            last = wire.encode_input(x[k, 0, 2 * hop - 1:2 * hop], x[k, 1, 2 * hop - 1:2 * hop], fmt)[-1:]
                            ins[k].sendall(last)
                else:
                    ins[s].sendall(data)                                    # the whole frame at once
            for s in range(2):
                ln, r = _read_result(outs[s])
                assert ln == 12876                                          # the result packet is unchanged: hop f64 samples per channel
                seg = x[s, :, f * hop:(f + 1) * hop]
                want = pcm.decode(fmt, seg, np.float64)
                for k, name in enumerate(("x1", "x2")):
                    got = np.asarray(r[name])
                    assert np.array_equal(got, want[k]) and not np.signbit(got[want[k] == 0]).any()
                np.testing.assert_allclose(r["p_now"], pcm.linear(fmt, seg).astype(np.float64).mean(axis=1), rtol=1e-6)
        assert len(m.blocks) == frames
        for f, (ids, block) in enumerate(m.blocks):                         # exactly the raw samples, de-interleaved, in batch order
            assert sorted(ids) == [0, 1] and block.dtype == pcm.DTYPES[fmt] and block.shape == (2, 2, hop)
            for k, sid in enumerate(ids):
                assert np.array_equal(block[k], x[sid, :, f * hop:(f + 1) * hop]), (f, sid)
        st = srv.stats()
        assert st["frames_done"] == 2 * frames and st["rx_bytes"] == 2 * frames * hop * pair
    finally:
        srv.close()


def test_group_front_end_echoes_a_slower_models_hops_from_raw_input():
    """A model at half the leader's rate answers every second hop with ONE packet that echoes both hops: the first comes from the
    front-end's f64 history, which is filled from the expanded raw staging."""
    hop = 800
    seen = []

    def step(ids, audio, wire_blocks):
        seen.append(audio.copy())
        wire_blocks["nod"][:, engine.OUT_STATUS] = 0.0 if len(seen) % 2 == 0 else engine.STATUS_NO_FRAME
        return 0

    srv = ingest.NativeServer.over_group_function(step, ["vap", "nod"], 1, frame_hz=[20, 10], ctx_frames=[8, 8], max_wait_s=0.2,
                                                  input_format="alaw")
    try:
        i = socket.create_connection(("127.0.0.1", srv.port_in))
        _wait(lambda: srv.stats()["in_connections"] == 1)
        o = socket.create_connection(("127.0.0.1", srv.ports_out["nod"]))
        _wait(lambda: srv.stats()["out_connections"] == 1)
        x = np.random.default_rng(3).integers(0, 256, (2, 2 * hop)).astype(np.uint8)
        for f in range(2):
            i.sendall(wire.encode_input(x[0, f * hop:(f + 1) * hop], x[1, f * hop:(f + 1) * hop], "alaw"))
            _wait(lambda: len(seen) == f + 1)
        o.settimeout(10)
        ln = struct.unpack("<I", _recv_exact(o, 4))[0]
        r = wire.decode_result(_recv_exact(o, ln), "nod")
        assert np.array_equal(r["x1"], pcm.decode("alaw", x[0], np.float64)) and np.array_equal(r["x2"], pcm.decode("alaw", x[1], np.float64))
        assert seen[0].dtype == np.uint8 and np.array_equal(seen[1][0], x[:, hop:])
    finally:
        srv.close()


def test_refusals_of_the_function_front_end():
    m = RawModel("s16")
    with pytest.raises(engine.VapxError, match="gain with a raw input format"):
        ingest.NativeServer.over_function(m.step, 1, 20, input_format="s16", gain=2.0)
    with pytest.raises(engine.VapxError, match="input_format: known are"):
        ingest.NativeServer.over_function(m.step, 1, 20, input_format=7)
    with pytest.raises(ValueError, match="g722"):
        ingest.NativeServer.over_function(m.step, 1, 20, input_format="g722")
    srv = ingest.NativeServer.over_function(m.step, 1, 20, input_format="f64", gain=2.0)      # gain and the f64 framing: as ever
    srv.close()
    # the Python twin refuses a raw format loudly

    class Vap:
        hop, n_streams, mode = 800, 1, "vap"

        def process(self, new, ids=None):
            raise AssertionError
    from vap_realtime_amd.server import ManyStreamServer
    with pytest.raises(ValueError, match="mulaw"):
        ManyStreamServer(Vap(), port_in=0, port_out=0, input_format="mulaw")
    Vap.input_format = "s16"
    with pytest.raises(ValueError, match="s16"):
        ManyStreamServer(Vap(), port_in=0, port_out=0)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
def test_open_against_an_engine_with_a_format(tmp_path):
    """A config format that disagrees with the engine's is refused with a message; the engine's format is taken otherwise (an engine
    needs a GPU, so the front-end is compiled next to a stub engine: tests/native/pcm_open_check.cpp).  The program also sends two frames
    per raw format through the front-end in chunks that split sample pairs; it is built with the address and undefined-behaviour
    sanitizers (a stand-alone program, as tests/test_ingest_sanitizers.py builds its own), so a step off the raw staging fails the test."""
    exe = tmp_path / "pcm_open_check"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wno-subobject-linkage", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "native", "pcm_open_check.cpp")],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    log = r.stdout + r.stderr
    for marker in ("ERROR: AddressSanitizer", "runtime error:", "LeakSanitizer"):
        assert marker not in log, log[-6000:]
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), log[-3000:]


def test_exports_and_serve_flag():
    for name in ("vapx_set_input_format", "vapx_get_input_format", "vapx_pcm_decode"):
        assert name in engine.EXPORTS and hasattr(engine.load_library(), name)
    import argparse
    from vap_realtime_amd import serve
    assert serve.rate_kw(argparse.Namespace(input_rate=16000, input_format="f64")) == {}
    assert serve.rate_kw(argparse.Namespace(input_rate=8000, input_format="mulaw")) == {"input_hz": 8000, "input_format": "mulaw"}
    assert serve.rate_kw(argparse.Namespace(input_rate=16000)) == {}
