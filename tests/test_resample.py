"""The input-rate filter without a GPU (vap-realtime_amd/resample.py): the tap tables against the formula's shape, the streaming form
against the whole-signal form in float64, the committed fp32 tables of the HIP kernel, and what state records and snapshot files of an
engine with an input rate look like next to today's."""
import os

import numpy as np
import pytest

from vap_realtime_amd import engine, resample, snapshot
from vap_realtime_amd.engine import VapxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRY = {8000: (1, 2, 7, 15, 14), 32000: (2, 1, 13, 28, 27), 48000: (3, 1, 19, 41, 40)}     # orig, new, width, K, H


def test_taps_shape_gain_and_symmetry():
    for hz, (orig, new, width, K, H) in GEOMETRY.items():
        q = resample.geometry(hz)
        assert (q["orig"], q["new"], q["width"], q["K"], q["H"], q["d"]) == (orig, new, width, K, H, 7)
        h = resample.taps(hz)
        assert h.shape == (new, K) and h.dtype == np.float64
        np.testing.assert_array_equal(h, h.astype(np.float32).astype(np.float64))         # the values ARE fp32 numbers
        assert np.all(np.abs(h.sum(axis=1) - 1.0) < 1e-3), h.sum(axis=1)                  # DC gain of every phase
        # phase 0 samples the kernel at (k - width) / orig: even around k = width
        np.testing.assert_array_equal(h[0, :2 * width + 1], h[0, :2 * width + 1][::-1])
        assert h[0, width] == np.float32(q["base"] / orig)                                # sinc(0) = 1, window(0) = 1
    for hz in (16000, 44100, 22050, 11025, 0):
        with pytest.raises(ValueError):
            resample.geometry(hz)
    assert [resample.history_floats(hz) for hz in (8000, 16000, 32000, 48000)] == [28, 0, 56, 80]
    assert resample.hop_in(8000, 20) == 400 and resample.hop_in(48000, 50) == 960 and resample.hop_in(32000, 10) == 3200


def test_taps_match_torchaudio_when_it_is_installed():
    ta = pytest.importorskip("torchaudio")
    import torch
    for hz, (orig, new, width, K, H) in GEOMETRY.items():
        kern, w = ta.functional.functional._get_sinc_resample_kernel(hz, 16000, np.gcd(hz, 16000), dtype=torch.float32)
        assert w == width
        np.testing.assert_array_equal(kern.reshape(new, K).double().numpy(), resample.taps(hz))


def test_committed_tap_tables_are_the_formula():
    path = os.path.join(ROOT, "vap-realtime_amd", "csrc", "resample_taps.h")
    assert open(path).read() == resample.taps_header_text()
    text = open(path).read()
    for hz in GEOMETRY:                                    # nine significant digits give back the fp32 value
        line = next(l for l in text.splitlines() if l.startswith(f"#define VAPX_RESAMPLE_TAPS_{hz} "))
        vals = np.array([np.float32(v.strip().rstrip("f")) for v in line.split(" ", 2)[2].split(",")], np.float32)
        np.testing.assert_array_equal(vals.astype(np.float64), resample.taps(hz).reshape(-1))


@pytest.mark.parametrize("hz,frame_hz", [(8000, 20), (48000, 50), (32000, 10)])
def test_streaming_equals_the_whole_signal_shifted(hz, frame_hz):
    q = resample.geometry(hz)
    rng = np.random.default_rng(hz)
    x = rng.uniform(-1, 1, (2, hz))                        # 1 s, two channels
    hop_in, hop = hz // frame_hz, 16000 // frame_hz
    st = resample.stream_state(hz, (2,))
    z = np.concatenate([resample.stream_ref(x[:, t * hop_in:(t + 1) * hop_in], st, hz) for t in range(frame_hz)], axis=-1)
    assert z.shape == (2, 16000) and st["hist"].shape == (2, q["H"])
    y = resample.whole_ref(x, hz)
    assert y.shape == (2, 16000)
    want = resample.delayed(y, hz, 16000)
    assert not want[:, :q["new"] * q["d"]].any() and want[:, q["new"] * q["d"]:].any()
    np.testing.assert_array_equal(z, want)                 # same taps, same order of summation: exact
    np.testing.assert_array_equal(st["hist"], x[:, -q["H"]:])
    # a signal whose length is no multiple of orig: ceil(new * n / orig) outputs
    assert resample.whole_ref(x[0, :1001], hz).shape == (-(-q["new"] * 1001 // q["orig"]),)


def test_state_record_floats_with_and_without_a_rate():
    for T in (1, 50, 200):
        base = engine.state_record_floats(T)
        assert engine.state_record_floats(T, input_hz=16000) == base == 8 + 1664 + 2 * T * 256
        for hz, extra in ((8000, 28), (32000, 56), (48000, 80)):
            assert engine.state_record_floats(T, input_hz=hz) == base + extra
            assert engine.state_record_floats(T, True, input_hz=hz) == engine.state_record_floats(T, True) + extra
            assert engine.state_record_floats(T, follower=True, input_hz=hz) == engine.state_record_floats(T, follower=True)   # the leader owns the audio
            assert engine.state_record_floats(T, input_hz=hz) % 4 == 0
    rec = np.zeros((2, engine.state_record_floats(5, input_hz=32000)), np.float32)
    rec[:, :8].view(np.int32)[:] = [engine.STATE_MAGIC, 5, 20, engine.STATE_HAS_LSTM | engine.STATE_HAS_RESAMPLE, 3, 0, 32000, 3]
    rec[:, 8 + 1664:8 + 1664 + 54] = np.arange(54)
    s = engine.split_state(rec, 5, input_hz=32000)
    assert s["input_hz"].tolist() == [32000, 32000] and s["resample_started"].tolist() == [3, 3]
    assert s["resample_hist"].shape == (2, 2, 27) and s["resample_hist"][1, 1, 0] == 27 and s["ring"].shape == (2, 2, 5, 256)
    assert engine.split_state(np.zeros((1, engine.state_record_floats(5)), np.float32), 5)["resample_hist"] is None
    with pytest.raises(VapxError, match="fits no layout"):
        engine.split_state(rec, 5)                         # read as a 16 kHz engine's record


class StubEngine:
    """What snapshot touches of an Engine."""

    def __init__(self, input_hz=None, T=6, hz=20, max_streams=3):
        self.T, self.frame_hz, self.mode, self.max_streams, self.split_f16 = T, hz, "vap", max_streams, False
        if input_hz is not None:
            self.input_hz = input_hz
        self.imported = []

    def _in_hz(self):
        return getattr(self, "input_hz", 16000)

    def export_streams(self, ids=None, cache=False):
        ids = list(range(self.max_streams)) if ids is None else list(ids)
        in_hz = self._in_hz()
        rec = np.random.default_rng(1).standard_normal((len(ids), engine.state_record_floats(self.T, cache, input_hz=in_hz))).astype(np.float32)
        bits = (engine.STATE_HAS_LSTM | (engine.STATE_HAS_CACHE if cache else 0) | (engine.STATE_HAS_RESAMPLE if in_hz != 16000 else 0))
        rec[:, :8].view(np.int32)[:] = [engine.STATE_MAGIC, self.T, self.frame_hz, bits, 2, 0, 0 if in_hz == 16000 else in_hz, 0]
        return rec

    def import_streams(self, ids, records, cache=None):
        self.imported.append((list(ids), np.array(records), cache))


def test_snapshot_header_carries_the_rate_only_when_it_is_not_16000(tmp_path):
    today = {"version": 1, "frame_hz": 20, "ctx_frames": 6, "modes": ["vap"], "split_f16": False, "cache": True, "ids": [0, 1, 2],
             "record_floats": [engine.state_record_floats(6, True)]}
    p16, p16b, p8 = (str(tmp_path / n) for n in ("s16", "s16b", "s8"))
    assert snapshot.save(p16, StubEngine()) == today                       # an engine that knows no rate
    assert snapshot.save(p16b, StubEngine(input_hz=16000)) == today        # ... and one at 16000: the header of today, key for key
    assert open(p16, "rb").read() == open(p16b, "rb").read()
    assert "input_hz" not in snapshot.describe(StubEngine(input_hz=16000))
    h8 = snapshot.save(p8, StubEngine(input_hz=8000))
    assert h8 == dict(today, input_hz=8000, record_floats=[engine.state_record_floats(6, True, input_hz=8000)])
    got, off = snapshot.read_header(p8)
    assert got == h8 and os.path.getsize(p8) == off + 4 * 3 * h8["record_floats"][0]
    # round trip into an 8000 engine
    b = StubEngine(input_hz=8000)
    assert snapshot.load(p8, b) == [0, 1, 2]
    np.testing.assert_array_equal(b.imported[0][1], StubEngine(input_hz=8000).export_streams(None, True))
    # an 8000 file is refused by a 16000 description, and the reverse; the field is named and nothing is imported
    for path, target in ((p8, StubEngine()), (p8, StubEngine(input_hz=16000)), (p16, StubEngine(input_hz=8000)), (p8, StubEngine(input_hz=48000))):
        with pytest.raises(VapxError, match="input_hz"):
            snapshot.load(path, target)
        assert target.imported == []
    # the per-record check names it too: a 16 kHz record inside a block described as 8000
    desc8 = snapshot.describe(StubEngine(input_hz=8000))
    with pytest.raises(VapxError, match=r"record 0: input_hz 0 differs from the engine's 8000"):
        snapshot.check_records(np.pad(StubEngine().export_streams(None, True), ((0, 0), (0, 28))), desc8, True, False)
    snapshot.check_records(StubEngine(input_hz=8000).export_streams(None, True), desc8, True, False)
    snapshot.check_records(StubEngine().export_streams(None, True), snapshot.describe(StubEngine()), True, False)


def test_offline_reads_the_new_rates_and_frames_them_in_hops(tmp_path):
    import wave
    from vap_realtime_amd import offline

    def wav(name, rate, n=2000):
        p = str(tmp_path / name)
        with wave.open(p, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate); w.writeframes((np.arange(n) % 100).astype("<i2").tobytes())
        return p
    assert isinstance(offline.read_wav_mono(wav("a16.wav", 16000)), np.ndarray)            # 16 kHz: the samples, as before
    for rate in (8000, 32000, 48000):
        x, got = offline.read_wav_mono(wav(f"a{rate}.wav", rate))
        assert got == rate and x.shape == (2000,) and x.dtype == np.float32
    for rate in (44100, 22050, 11025):
        with pytest.raises(ValueError, match="expected 16000 Hz"):
            offline.read_wav_mono(wav(f"b{rate}.wav", rate))

    class FakeVap:
        hop, hop_in, calls = 800, 400, []

        def process(self, batch, ids):
            self.calls.append((batch.shape, ids.tolist()))
            return {"p_now": np.zeros((len(ids), 2)), "p_future": np.ones((len(ids), 2))}
    vap = FakeVap()
    a, b = np.arange(1300, dtype=np.float32), np.arange(450, dtype=np.float32)
    res = offline.run_offline_hops(vap, [(a, a), (b, b)])
    assert [len(r) for r in res] == [3, 1] and vap.calls == [((2, 2, 400), [0, 1]), ((1, 2, 400), [0]), ((1, 2, 400), [0])]
    assert [r["t"] for r in res[0]] == [0.05, 0.1, 0.15]                                   # the server's framing: (f + 1) * hop / 16000


def test_serve_applies_the_rate_to_the_engines_it_builds():
    import argparse
    from vap_realtime_amd import serve
    assert serve.rate_kw(argparse.Namespace(input_rate=16000)) == {} and serve.rate_kw(argparse.Namespace()) == {}      # engines built as before
    assert serve.rate_kw(argparse.Namespace(input_rate=8000)) == {"input_hz": 8000}
    steps = []

    class Lead:
        max_batch, hop, hop_in = 2, 800, 400

        def step(self, audio):
            steps.append(audio.shape)

        def reset_stream(self, i):
            steps.append(i)
    serve._warm_up(Lead())                                 # the warm-up tick before a snapshot import takes hop_in samples
    assert steps == [(2, 2, 400), 0, 1]
    with pytest.raises(SystemExit):
        serve.main(["--input_rate", "44100"])
