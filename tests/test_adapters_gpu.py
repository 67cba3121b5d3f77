"""Drop-in surfaces on the GPU: VAPRealTime (level 2), the model-attribute surface (level 1) driven
by an orchestration that reads like the reference's process_vap, and the TCP front-end end to end."""
import socket
import struct
import time

import numpy as np
import pytest

from golden_util import Case

pytestmark = pytest.mark.gpu
TOL = 1e-4


def test_vaprealtime_dropin_matches_golden():
    """Same constructor / process_vap / result attributes as rvap/vap_main/vap_main.py:185-335, fed
    the way proc_serv_in feeds it (float64 carry + new samples)."""
    import torch
    from vap_realtime_amd.realtime import VAPRealTime
    c = Case("vap20")
    rt = VAPRealTime(c.vap_sd, {"weights": c.cpc_sd}, torch.device("cuda", 0), c.frame_hz, c.ctx_sec)
    assert rt.audio_frame_size == 1120 and rt.frame_contxt_padding == 320 and rt.audio_context_len == 50
    cur1, cur2 = np.zeros(320), np.zeros(320)
    for f in range(c.n_frames):
        new = c.new_samples(f)[0].astype(np.float64)
        cur1, cur2 = np.concatenate([cur1, new[0]]), np.concatenate([cur2, new[1]])
        assert len(cur1) == rt.audio_frame_size
        before = rt.process_time_abs
        rt.process_vap(cur1 if f % 2 else cur1.tolist(), cur2 if f % 2 else cur2.tolist())   # list and ndarray inputs
        assert rt.process_time_abs != before
        np.testing.assert_allclose(rt.result_p_now, c.z["p_now"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(rt.result_p_future, c.z["p_future"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(rt.result_vad, c.z["vad"][f][0], rtol=0, atol=TOL)
        assert len(rt.current_x1_audio) == 800
        cur1, cur2 = cur1[-320:], cur2[-320:]
    r = rt.get_result()
    assert set(r) == {"t", "x1", "x2", "p_now", "p_future", "vad"}
    with pytest.raises(ValueError):
        rt.process_vap(np.zeros(100), np.zeros(100))


def test_level1_model_surface_under_reference_style_orchestration():
    """The calls process_vap makes on self.vap (vap_main.py:272-307), against the HIP-backed VapGPT."""
    import torch
    from vap_realtime_amd.realtime import VapGPT
    c = Case("vap20")
    vap = VapGPT.from_state_dicts(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec).to("cuda").eval()
    e1_context, e2_context = [], []
    carry = np.zeros((2, 320), np.float32)
    for f in range(c.n_frames):
        buf = np.concatenate([carry, c.new_samples(f)[0]], axis=1)
        carry = buf[:, -320:]
        x1_ = torch.from_numpy(buf[0]).cuda().unsqueeze(0).unsqueeze(0)
        x2_ = torch.from_numpy(buf[1]).cuda().unsqueeze(0).unsqueeze(0)
        e1, e2 = vap.encode_audio(x1_, x2_)
        e1_context.append(e1); e2_context.append(e2)
        e1_context, e2_context = e1_context[-c.T:], e2_context[-c.T:]
        x1c, x2c = torch.cat(e1_context, dim=1), torch.cat(e2_context, dim=1)
        o1 = vap.ar_channel(x1c, attention=False)
        o2 = vap.ar_channel(x2c, attention=False)
        out = vap.ar(o1["x"], o2["x"], attention=False)
        logits = vap.vap_head(out["x"])
        vad1 = vap.va_classifier(o1["x"]).sigmoid()[:, -1]
        vad2 = vap.va_classifier(o2["x"]).sigmoid()[:, -1]
        probs = logits.softmax(dim=-1)
        p_now = vap.objective.probs_next_speaker_aggregate(probs, from_bin=0, to_bin=1)
        p_future = vap.objective.probs_next_speaker_aggregate(probs, from_bin=2, to_bin=3)
        np.testing.assert_allclose(logits[0, -1].cpu().numpy(), c.z["logits"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(p_now[0, -1].cpu().numpy(), c.z["p_now"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(p_future[0, -1].cpu().numpy(), c.z["p_future"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose([float(vad1), float(vad2)], c.z["vad"][f][0], rtol=0, atol=TOL)
        if f"inter.f{f}.rows" in c.z.files:
            rows = c.z[f"inter.f{f}.rows"]
            np.testing.assert_allclose(out["x"][0].cpu().numpy()[rows], c.z[f"inter.f{f}.comb"], rtol=0, atol=TOL)
            np.testing.assert_allclose(out["x1"][0].cpu().numpy()[rows], c.z[f"inter.f{f}.stereo2"][0], rtol=3e-5, atol=1e-3)


class _ReferenceShapedRealTime:
    """``VAPRealTime`` with the reference's construction statements (vap_main.py:194-215; vap_bc_main.py:188-209, vap_nod_main.py:187-208 and
    the library twin vap_realtime/model.py:25-49 are the same lines) and its per-frame orchestration (vap_main.py:249-320 /
    vap_realtime/model.py:126-240).  Only the two class names are rebound to vap_realtime_amd.realtime; tests/test_level1_construction.py
    runs the same statements on the CPU."""

    BINS_P_NOW = [0, 1]
    BINS_PFUTURE = [2, 3]

    def __init__(self, VapConfig, VapGPT, mode, vap_model, cpc_model, device, frame_rate, context_len_sec):
        import torch
        from torch import nn
        conf = VapConfig()
        self.vap = VapGPT(conf)

        self.device = device

        sd = torch.load(vap_model, map_location=torch.device('cpu'))
        self.vap.load_encoder(cpc_model=cpc_model)
        self.vap.load_state_dict(sd, strict=False)

        self.vap.encoder1.downsample[1].weight = nn.Parameter(sd['encoder.downsample.1.weight'])
        self.vap.encoder1.downsample[1].bias = nn.Parameter(sd['encoder.downsample.1.bias'])
        self.vap.encoder1.downsample[2].ln.weight = nn.Parameter(sd['encoder.downsample.2.ln.weight'])
        self.vap.encoder1.downsample[2].ln.bias = nn.Parameter(sd['encoder.downsample.2.ln.bias'])

        self.vap.encoder2.downsample[1].weight = nn.Parameter(sd['encoder.downsample.1.weight'])
        self.vap.encoder2.downsample[1].bias = nn.Parameter(sd['encoder.downsample.1.bias'])
        self.vap.encoder2.downsample[2].ln.weight = nn.Parameter(sd['encoder.downsample.2.ln.weight'])
        self.vap.encoder2.downsample[2].ln.bias = nn.Parameter(sd['encoder.downsample.2.ln.bias'])

        self.vap.to(self.device)
        self.vap = self.vap.eval()

        self.mode = mode
        self.audio_context_len = int(context_len_sec * frame_rate)
        self.e1_context = []
        self.e2_context = []

    def process_vap(self, x1, x2):
        import torch
        with torch.no_grad():
            x1_ = torch.tensor([[x1]], dtype=torch.float32, device=self.device)
            x2_ = torch.tensor([[x2]], dtype=torch.float32, device=self.device)
            e1, e2 = self.vap.encode_audio(x1_, x2_)
            self.e1_context.append(e1)
            self.e2_context.append(e2)
            if len(self.e1_context) > self.audio_context_len:
                self.e1_context = self.e1_context[-self.audio_context_len:]
            if len(self.e2_context) > self.audio_context_len:
                self.e2_context = self.e2_context[-self.audio_context_len:]
            x1_ = torch.cat(self.e1_context, dim=1).to(self.device)
            x2_ = torch.cat(self.e2_context, dim=1).to(self.device)
            o1 = self.vap.ar_channel(x1_, attention=False)
            o2 = self.vap.ar_channel(x2_, attention=False)
            out = self.vap.ar(o1["x"], o2["x"], attention=False)
            r = {}
            if self.mode == "vap":
                logits = self.vap.vap_head(out["x"])
                vad1 = self.vap.va_classifier(o1["x"])
                vad2 = self.vap.va_classifier(o2["x"])
                probs = logits.softmax(dim=-1)
                p_now = self.vap.objective.probs_next_speaker_aggregate(probs, from_bin=self.BINS_P_NOW[0], to_bin=self.BINS_P_NOW[-1])
                p_future = self.vap.objective.probs_next_speaker_aggregate(probs, from_bin=self.BINS_PFUTURE[0], to_bin=self.BINS_PFUTURE[1])
                r["p_now"] = p_now.to('cpu').tolist()[0][-1]
                r["p_future"] = p_future.to('cpu').tolist()[0][-1]
                r["vad"] = [float(vad1.sigmoid().to('cpu')[::, -1]), float(vad2.sigmoid().to('cpu')[::, -1])]
                r["logits"] = logits.to('cpu')[0, -1].numpy()
            elif self.mode == "bc":
                bc = self.vap.bc_head(out["x"])
                r["p_bc_react"] = float(bc.softmax(dim=-1)[:, -1, 1].to('cpu'))
                r["p_bc_emo"] = float(bc.softmax(dim=-1)[:, -1, 2].to('cpu'))
            else:
                p_bc = self.vap.bc_head(out["x"])
                nod = self.vap.nod_head(out["x"])
                r["p_bc"] = p_bc.sigmoid()[-1].to('cpu').numpy().reshape(-1)            # every row of the window (vap_nod_main.py:276)
                r["p_nod_short"] = float(nod.softmax(dim=-1)[:, -1, 1].to('cpu'))
                r["p_nod_long"] = float(nod.softmax(dim=-1)[:, -1, 2].to('cpu'))
                r["p_nod_long_p"] = float(nod.softmax(dim=-1)[:, -1, 3].to('cpu'))
            return r


@pytest.mark.parametrize("name", ["vap20", "bc20", "nod20", "vap50", "nod20_10s"])
def test_reference_constructor_lines_then_level1_orchestration(name, tmp_path):
    """``VapGPT(VapConfig())`` -> ``load_encoder`` -> ``load_state_dict(strict=False)`` -> eight downsample assignments ->
    ``.to(device)`` -> ``.eval()`` against a lazily built libvapx engine, then the reference's per-frame calls; checkpoint FILES in the
    reference's format.  ``vap50`` (T = 250) and ``nod20_10s`` (T = 200) outgrow the engine's first window capacity (64 rows) during warm-up:
    the rebuild must carry the LSTM state over (any loss shows as a jump at frame 65)."""
    import argparse
    import torch
    from vap_realtime_amd import realtime as R
    c = Case(name)
    vap_t = {k: torch.from_numpy(np.asarray(v)) for k, v in c.vap_sd.items()}
    vap_t["encoder.encoder.gEncoder.conv0.weight"] = torch.zeros(256, 1, 10)
    vap_p, cpc_p = str(tmp_path / "vap_state_dict.pt"), str(tmp_path / "60k_epoch4-d0f474de.pt")
    torch.save(vap_t, vap_p)
    torch.save({"weights": {k: torch.from_numpy(np.asarray(v)) for k, v in c.cpc_sd.items()},
                "config": argparse.Namespace(hiddenGar=256, hiddenEncoder=256)}, cpc_p)
    klass = {"vap": R.VapGPT, "bc": R.VapGPT_bc, "nod": R.VapGPT_nod}[c.mode]
    rt = _ReferenceShapedRealTime(R.VapConfig, klass, c.mode, vap_p, cpc_p, torch.device("cuda", 0), c.frame_hz, c.ctx_sec)
    assert rt.vap._engine is None                                # lazily built
    cur = np.zeros((2, 320))
    capacities = set()
    for f in range(c.n_frames):
        cur = np.concatenate([cur, c.new_samples(f)[0].astype(np.float64)], axis=1)
        r = rt.process_vap(cur[0].tolist(), cur[1].tolist())
        cur = cur[:, -320:]
        capacities.add(rt.vap._engine.T)
        if c.mode == "vap":
            np.testing.assert_allclose(r["logits"], c.z["logits"][f][0], rtol=0, atol=TOL, err_msg=f"frame {f}")
            np.testing.assert_allclose(r["p_now"], c.z["p_now"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_future"], c.z["p_future"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["vad"], c.z["vad"][f][0], rtol=0, atol=TOL)
        elif c.mode == "bc":
            np.testing.assert_allclose(r["p_bc_react"], c.z["p_bc_react"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_bc_emo"], c.z["p_bc_emo"][f][0], rtol=0, atol=TOL)
        else:
            n = min(f + 1, c.T)
            np.testing.assert_allclose(r["p_bc"], c.z["p_bc"][f][0, :n], rtol=0, atol=TOL, err_msg=f"frame {f}")
            np.testing.assert_allclose(r["p_nod_short"], c.z["p_nod_short"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_nod_long"], c.z["p_nod_long"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_nod_long_p"], c.z["p_nod_long_p"][f][0], rtol=0, atol=TOL)
    assert capacities == ({64} if c.T <= 64 else {64, 256})
    assert rt.vap.frame_hz == c.frame_hz                          # read off the downsample kernel, not off VapConfig (50)
    # a weight assigned after the engine exists takes effect on the next call (the stale engine is rebuilt)
    if c.mode == "vap":
        x = torch.randn(1, 3, 256, device="cuda")
        before = rt.vap.va_classifier(x)
        sd = torch.load(vap_p, map_location="cpu")
        sd["va_classifier.bias"] = sd["va_classifier.bias"] + 1.0
        rt.vap.load_state_dict(sd, strict=False)
        np.testing.assert_allclose((rt.vap.va_classifier(x) - before).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    with pytest.raises(NotImplementedError):
        rt.vap.ar_channel(torch.zeros(1, 4, 256, device="cuda"), attention=True)


def test_tcp_front_end_end_to_end_on_gpu():
    """2560-byte packets in, length-prefixed result packets out, three dialogues on one engine."""
    from vap_realtime_amd import wire
    from vap_realtime_amd.realtime import ManyStreamVAP
    from vap_realtime_amd.server import ManyStreamServer
    c = Case("multi3")
    vap = ManyStreamVAP(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, n_streams=3)
    srv = ManyStreamServer(vap, port_in=0, port_out=0, max_wait_s=1.0).start()
    try:
        ins = []
        for _ in range(3):
            ins.append(socket.create_connection(("127.0.0.1", srv.port_in)))
            time.sleep(0.05)
        outs = []
        for _ in range(3):
            outs.append(socket.create_connection(("127.0.0.1", srv.port_out)))
            time.sleep(0.05)
        for f in range(6):
            new = c.new_samples(f).astype(np.float64)
            for p in range(5):
                for s in range(3):
                    ins[s].sendall(wire.encode_input(new[s, 0, p * 160:(p + 1) * 160], new[s, 1, p * 160:(p + 1) * 160]))
            for s in range(3):
                outs[s].settimeout(20)
                hdr = b""
                while len(hdr) < 4:
                    hdr += outs[s].recv(4 - len(hdr))
                ln = struct.unpack("<I", hdr)[0]
                assert ln == 12876
                payload = b""
                while len(payload) < ln:
                    payload += outs[s].recv(ln - len(payload))
                r = wire.decode_result(payload)
                np.testing.assert_allclose(r["p_now"], c.z["p_now"][f][s], rtol=0, atol=TOL)
                np.testing.assert_allclose(r["p_future"], c.z["p_future"][f][s], rtol=0, atol=TOL)
                np.testing.assert_allclose(r["vad"], c.z["vad"][f][s], rtol=0, atol=TOL)
                np.testing.assert_array_equal(r["x1"], new[s, 0])
    finally:
        srv.stop()


def test_level3_functional_step_matches_the_reference_static_module():
    """VAPRealTimeStatic.forward (tools/vap_static.py:235-304, the module the reference exports to ONNX): caller-held
    embedding context, first call with a zero row — against a golden produced by the reference class itself."""
    import os
    import torch
    from golden_util import GOLDEN
    from vap_realtime_amd import realtime, synth, weights as W
    z = np.load(os.path.join(GOLDEN, "static20.npz"))
    hz, ctx, F_ = int(z["meta.frame_hz"]), float(z["meta.ctx_sec"]), int(z["meta.n_frames"])
    cpc, vap = W.synthetic_weights(int(z["meta.seed"]), hz, "vap")
    assert np.array_equal(W.weights_fingerprint(cpc, vap), z["meta.weights_fp"])
    hop, T = 16000 // hz, int(ctx * hz)
    audio = synth.dialogue_batch([int(z["meta.stream"])], hop * F_ + 320)
    m = realtime.VAPRealTimeStatic(vap, cpc, torch.device("cuda", 0), hz, ctx)
    e1c = torch.zeros(1, 1, 256)
    e2c = torch.zeros(1, 1, 256)
    worst = 0.0
    for f in range(F_):
        win = torch.from_numpy(audio[:, :, f * hop:f * hop + hop + 320].copy())
        p_now, p_future, v1, v2, e1, e2 = m(win[:, 0:1], win[:, 1:2], e1c, e2c)
        assert p_now.shape == (1, 2) and v1.shape == (1, 1) and e1.shape == (1, 1, 256)
        got = {"p_now": p_now[0].cpu().numpy(), "p_future": p_future[0].cpu().numpy(),
               "vad": np.array([float(v1), float(v2)], np.float32), "e": torch.stack([e1[0, 0], e2[0, 0]]).cpu().numpy()}
        for k, v in got.items():
            worst = max(worst, float(np.abs(v - z[k][f]).max()))
        e1c = e1 if f == 0 else torch.cat([e1c.to(e1.device), e1], dim=1)[:, -(T - 1):]
        e2c = e2 if f == 0 else torch.cat([e2c.to(e2.device), e2], dim=1)[:, -(T - 1):]
    print("static forward worst |diff| =", worst)
    assert worst <= TOL
    with pytest.raises(Exception, match="exceeds"):
        m(win[:, 0:1], win[:, 1:2], torch.zeros(1, T, 256), torch.zeros(1, T, 256))


def test_vapgpt_forward_signature_with_realtime_semantics():
    """VapGPT.forward(waveform[B,2,N]) -> {"logits": [B,n,256], "vad": [B,n,2]} (train/model.py:292-319 signature) run
    with the realtime framing: must reproduce the per-frame logits / VAD of the reference's process_vap goldens, for a
    batch of independent dialogues in one call, and be repeatable (state is reset per call)."""
    import torch
    from vap_realtime_amd import realtime
    c = Case("multi3")
    m = realtime.VapGPT.from_state_dicts(c.cpc_sd, c.vap_sd, c.frame_hz, c.ctx_sec, max_batch=3)
    wav = torch.from_numpy(c.audio[:, :, :c.hop * c.n_frames].copy())
    for _ in range(2):
        ret = m(wav)
        assert set(ret) == {"logits", "vad"}
        assert ret["logits"].shape == (3, c.n_frames, 256) and ret["vad"].shape == (3, c.n_frames, 2)
        got_l = ret["logits"].cpu().numpy().transpose(1, 0, 2)           # [F,S,256] like the golden
        got_v = torch.sigmoid(ret["vad"]).cpu().numpy().transpose(1, 0, 2)
        assert np.abs(got_l - c.z["logits"]).max() <= TOL
        assert np.abs(got_v - c.z["vad"]).max() <= TOL
    with pytest.raises(NotImplementedError):
        m(wav, attention=True)


@pytest.mark.parametrize("name", ["vap20", "bc20", "nod20"])
def test_vaprealtime_from_reference_format_checkpoint_files(name, tmp_path):
    """``VAPRealTime(vap_model_path, cpc_model_path, device, rate, ctx)`` exactly as vap_main.py:500 calls it,
    on files in the reference's on-disk format (torch state dict incl. the ignored ``encoder.encoder.*`` keys; CPC file =
    {"weights": ..., "config": argparse.Namespace}); outputs must equal the golden of the imported reference, and
    ``get_result()`` must carry the mode's keys (vap_realtime/model.py:189-240)."""
    import argparse
    import torch
    from vap_realtime_amd.realtime import VAPRealTime
    c = Case(name)
    vap_t = {k: torch.from_numpy(np.asarray(v)) for k, v in c.vap_sd.items()}
    vap_t["encoder.encoder.gEncoder.conv0.weight"] = torch.zeros(256, 1, 10)     # skipped like vap_main.py:199-201
    vap_p, cpc_p = tmp_path / "vap_state_dict.pt", tmp_path / "60k_epoch4-d0f474de.pt"
    torch.save(vap_t, vap_p)
    torch.save({"weights": {k: torch.from_numpy(np.asarray(v)) for k, v in c.cpc_sd.items()},
                "config": argparse.Namespace(hiddenGar=256, hiddenEncoder=256)}, cpc_p)
    rt = VAPRealTime(str(vap_p), str(cpc_p), torch.device("cuda", 0), c.frame_hz, c.ctx_sec, mode=c.mode)
    cur = np.zeros((2, 320))
    for f in range(c.n_frames):
        cur = np.concatenate([cur, c.new_samples(f)[0].astype(np.float64)], axis=1)
        rt.process_vap(cur[0], cur[1])
        cur = cur[:, -320:]
        r = rt.get_result()
        if c.mode == "vap":
            assert set(r) == {"t", "x1", "x2", "p_now", "p_future", "vad"}
            np.testing.assert_allclose(r["p_now"], c.z["p_now"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_future"], c.z["p_future"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["vad"], c.z["vad"][f][0], rtol=0, atol=TOL)
        elif c.mode == "bc":
            assert set(r) == {"t", "x1", "x2", "p_bc_react", "p_bc_emo"}
            np.testing.assert_allclose(r["p_bc_react"], c.z["p_bc_react"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_bc_emo"], c.z["p_bc_emo"][f][0], rtol=0, atol=TOL)
        else:
            assert set(r) == {"t", "x1", "x2", "p_bc", "p_nod_short", "p_nod_long", "p_nod_long_p"}
            n = min(f + 1, c.T)
            np.testing.assert_allclose(np.asarray(r["p_bc"]).reshape(-1), c.z["p_bc"][f][0, :n], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_nod_short"], c.z["p_nod_short"][f][0], rtol=0, atol=TOL)
            np.testing.assert_allclose(r["p_nod_long_p"], c.z["p_nod_long_p"][f][0], rtol=0, atol=TOL)


@pytest.mark.parametrize("name", ["multi3", "bc20", "nod20"])
def test_native_tcp_front_end_end_to_end_on_gpu(name):
    """libvapx's own front-end (vapx_ingest_*): reference-format input packets in, reference-format result packets out,
    numbers == the golden of the imported reference program (vap_main / vap_bc_main / vap_nod_main), echo bit-exact."""
    from vap_realtime_amd import engine, ingest, weights as W, wire
    c = Case(name)
    S = len(c.streams)
    eng = engine.Engine(W.pack_blob(c.cpc_sd, c.vap_sd, c.mode), c.frame_hz, c.ctx_sec, max_streams=S + 2, mode=c.mode)
    srv = ingest.NativeServer(eng, port_in=0, port_out=0, max_wait_s=0.5)
    try:
        ins = [socket.create_connection(("127.0.0.1", srv.port_in)) for _ in range(S)]
        while srv.stats()["in_connections"] < S:
            time.sleep(0.01)
        outs = [socket.create_connection(("127.0.0.1", srv.port_out)) for _ in range(S)]
        while srv.stats()["out_connections"] < S:
            time.sleep(0.01)
        for f in range(c.n_frames):
            new = c.new_samples(f).astype(np.float64)
            for p in range(c.hop // 160):
                for s in range(S):
                    ins[s].sendall(wire.encode_input(new[s, 0, p * 160:(p + 1) * 160], new[s, 1, p * 160:(p + 1) * 160]))
            for s in range(S):
                outs[s].settimeout(20)
                hdr = b""
                while len(hdr) < 4:
                    hdr += outs[s].recv(4 - len(hdr))
                ln = struct.unpack("<I", hdr)[0]
                payload = b""
                while len(payload) < ln:
                    payload += outs[s].recv(ln - len(payload))
                r = wire.decode_result(payload, c.mode)
                np.testing.assert_array_equal(r["x1"], new[s, 0])
                np.testing.assert_array_equal(r["x2"], new[s, 1])
                if c.mode == "vap":
                    assert ln == 12876
                    for k in ("p_now", "p_future", "vad"):
                        np.testing.assert_allclose(r[k], c.z[k][f][s], rtol=0, atol=TOL)
                elif c.mode == "bc":
                    np.testing.assert_allclose(r["p_bc_react"], c.z["p_bc_react"][f][s], rtol=0, atol=TOL)
                    np.testing.assert_allclose(r["p_bc_emo"], c.z["p_bc_emo"][f][s], rtol=0, atol=TOL)
                else:
                    n = min(f + 1, c.T)
                    assert len(r["p_bc"]) == n                                  # every window row (vap_nod_main.py:276 quirk)
                    np.testing.assert_allclose(r["p_bc"], c.z["p_bc"][f][s][:n], rtol=0, atol=TOL)
                    for k in ("p_nod_short", "p_nod_long", "p_nod_long_p"):
                        np.testing.assert_allclose(r[k], c.z[k][f][s], rtol=0, atol=TOL)
        st = srv.stats()
        assert st["frames_done"] == c.n_frames * S and st["numeric_resets"] == 0 and st["dropped_listeners"] == 0
    finally:
        srv.close()
        eng.close()


def test_library_twin_vap_class_with_microphone_sources(tmp_path):
    """``Vap(mode, frame_rate, context_len_sec, language, mic1, mic2, ..., cpc_model=..., device=...)`` as in
    vap_realtime/model.py:15-257: checkpoint found by the reference's file name in a local directory, ``start_process()`` runs the
    worker that pulls 160-sample chunks from two microphone-like objects, ``get_result()`` blocks for one dict per frame."""
    import queue
    import torch
    from vap_realtime_amd import checkpoints as ck
    from vap_realtime_amd.realtime import Vap
    c = Case("vap20")
    _, fname = ck.checkpoint_name("vap", c.frame_hz, c.ctx_sec, "jp")
    (tmp_path / "asset" / "vap").mkdir(parents=True)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in c.vap_sd.items()}, tmp_path / "asset" / "vap" / fname)
    cpc_p = tmp_path / "cpc.pt"
    torch.save({"weights": {k: torch.from_numpy(np.asarray(v)) for k, v in c.cpc_sd.items()}}, cpc_p)

    class Mic:                                   # stands in for vap_realtime.input.Mic / Wav (out of scope): 160 samples per call
        def __init__(self, x):
            self.q = queue.Queue()
            for k in range(0, len(x), 160):
                self.q.put(x[k:k + 160].astype(np.float64))
            self.started = False

        def start_process(self):
            self.started = True

        def get_audio_data(self):
            try:
                return self.q.get(timeout=5)
            except queue.Empty:
                return None

    n = 12
    audio = c.audio[0, :, :c.hop * n]
    vap = Vap("vap", c.frame_hz, c.ctx_sec, "jp", Mic(audio[0]), Mic(audio[1]), cpc_model=str(cpc_p), device="cuda",
              search_dirs=[str(tmp_path)])
    with pytest.raises(Exception, match="never downloads"):
        Vap("vap", c.frame_hz, c.ctx_sec, "jp", cpc_model=str(cpc_p), search_dirs=[str(tmp_path)], force_download=True)
    vap.start_process()
    assert vap.mic1.started and vap.mic2.started
    for f in range(n):
        r = vap.get_result()                     # blocks until the worker has processed frame f
        assert set(r) == {"t", "x1", "x2", "p_now", "p_future", "vad"} and len(r["x1"]) == c.hop
        np.testing.assert_allclose(r["p_now"], c.z["p_now"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(r["p_future"], c.z["p_future"][f][0], rtol=0, atol=TOL)
        np.testing.assert_allclose(r["vad"], c.z["vad"][f][0], rtol=0, atol=TOL)
    vap._stop_worker = True


@pytest.mark.parametrize("gpus,precision", [(1, "fp32"), (2, "fp32"), (1, "split"), (1, "auto"), (2, "procs")], ids=["1", "2", "1-split", "1-auto", "2-procs"])
def test_serve_program_end_to_end(gpus, precision):
    """``python -m vap_realtime_amd.serve`` — the twin of ``python vap_main.py --vap_model ... --port_num_in ... --gpu`` (vap_main.py:461-530)
    for many dialogues: started as a subprocess with the reference's argument names, fed the golden audio over TCP, answers compared
    with the golden of the imported reference; SIGTERM stops it.  gpus = 2: two engines (both on this box's one GPU, ``--share-gpu``)
    behind ONE port pair — the front door sends dialogue k to engine k mod 2, every dialogue still gets its own golden numbers.
    ``--precision split``: the served engine runs the opt-in split-precision path (dedicated GPU), same golden, same tolerance.
    ``--precision auto`` (the default): 4 dialogues of the 20 Hz model are far below the fp32 path's capacity — it must pick fp32 and say so.
    ``2-procs``: ``--worker-procs on`` — the front door is a process of its own, each "GPU" a worker process that receives its connections over
    a unix-socket link (vapx_frontdoor_open_links); same ports, same placement, same golden numbers."""
    worker_procs = precision == "procs"
    if worker_procs:
        precision = "fp32"
    import os
    import re
    import signal
    import subprocess
    import sys
    from vap_realtime_amd import wire
    c = Case("multi3")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.Popen([sys.executable, "-u", "-m", "vap_realtime_amd.serve", "--synthetic-weights", str(c.seed), "--streams", "4",
                             "--port_num_in", "0", "--port_num_out", "0", "--vap_process_rate", str(c.frame_hz),
                             "--context_len_sec", str(c.ctx_sec), "--gpu", "--stats_sec", "0"]
                            + (["--gpus", str(gpus), "--share-gpu"] if gpus > 1 else []) + ["--precision", precision]
                            + (["--worker-procs", "on"] if worker_procs else ["--worker-procs", "off"]),
                            cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        line, seen = "", []
        t0 = time.time()
        while "input :" not in line and time.time() - t0 < 180:
            line = proc.stdout.readline()
            seen.append(line)
            assert line or proc.poll() is None, "serve exited early"
        if precision == "auto":
            assert any("--precision auto -> fp32" in l for l in seen), seen
            assert "fp32 arithmetic" in line
        assert ("worker processes" in line) == worker_procs
        pin, pout = (int(x) for x in re.search(r"input :(\d+), output :(\d+)", line).groups())
        S = len(c.streams)
        ins, outs = [], []
        for _ in range(S):                       # one by one: arrival order = dialogue index (the wire carries no stream id)
            ins.append(socket.create_connection(("127.0.0.1", pin)))
            time.sleep(0.1)
        for _ in range(S):
            outs.append(socket.create_connection(("127.0.0.1", pout)))
            time.sleep(0.1)
        for f in range(8):
            new = c.new_samples(f).astype(np.float64)
            for s in range(S):
                ins[s].sendall(wire.encode_input(new[s, 0], new[s, 1]))
            for s in range(S):
                outs[s].settimeout(30)
                hdr = b""
                while len(hdr) < 4:
                    hdr += outs[s].recv(4 - len(hdr))
                ln = struct.unpack("<I", hdr)[0]
                payload = b""
                while len(payload) < ln:
                    payload += outs[s].recv(ln - len(payload))
                r = wire.decode_result(payload)
                np.testing.assert_allclose(r["p_now"], c.z["p_now"][f][s], rtol=0, atol=TOL)
                np.testing.assert_allclose(r["vad"], c.z["vad"][f][s], rtol=0, atol=TOL)
        for s in ins + outs:
            s.close()
    finally:
        proc.send_signal(signal.SIGTERM)
        try:
            proc.wait(timeout=30)
        except subprocess.TimeoutExpired:
            proc.kill()
    assert proc.returncode == 0
