"""Mixed trunk groups without a device: the oracle against the mix_* goldens (three reference programs on one cpc_model file at
their own rates and windows), the group front-end's host logic for a model at half the leader's rate
(vapx_ingest_open_group_fn2 over a scripted step function), and the argument handling of TrunkGroup and serve."""
import socket
import struct
import time

import numpy as np
import pytest

from golden_util import Case
from oracle.vap_oracle import ServerFramer, VapOracle
from vap_realtime_amd import capacity, engine, ingest, serve, wire

TOL = 2e-5          # logits / embeddings: fp32 summation-order noise between two CPU formulations (tests/test_oracle_golden.py)
TOL_P = 2e-6        # probabilities


def _run_oracle(case):
    o = VapOracle(case.cpc_sd, case.vap_sd, case.frame_hz, case.ctx_sec, case.mode)
    S = len(case.streams)
    st, fr = o.new_state(S), ServerFramer(S, case.hop)
    return [o.step(fr.frame(case.new_samples(f)), st, None) for f in range(case.n_frames)]


def test_oracle_matches_the_three_programs_at_their_own_rates_and_windows():
    cv, cb, cn = Case("mix_vap20"), Case("mix_bc20_3s"), Case("mix_nod10_3s")
    assert (cv.frame_hz, cv.T, cb.frame_hz, cb.T, cn.frame_hz, cn.T) == (20, 50, 20, 60, 10, 30)
    assert cv.audio.shape == cb.audio.shape == cn.audio.shape == (2, 2, 64320) and np.array_equal(cv.audio, cn.audio)
    for k in cv.cpc_sd:                                        # one cpc_model file, whatever the rate
        assert np.array_equal(cv.cpc_sd[k], cb.cpc_sd[k]) and np.array_equal(cv.cpc_sd[k], cn.cpc_sd[k])
    es = int(cv.z["meta.e_stride"])
    for f, out in enumerate(_run_oracle(cv)):
        for k in ("p_now", "p_future", "vad"):
            np.testing.assert_allclose(out[k], cv.z[k][f], rtol=0, atol=TOL_P)
        np.testing.assert_allclose(out["logits"], cv.z["logits"][f], rtol=0, atol=TOL)
        if f % es == 0:
            np.testing.assert_allclose(out["e"], cv.z["e"][f // es], rtol=0, atol=TOL)
    for f, out in enumerate(_run_oracle(cb)):
        np.testing.assert_allclose(out["p_bc_react"], cb.z["p_bc_react"][f].reshape(-1), rtol=0, atol=TOL_P)
        np.testing.assert_allclose(out["p_bc_emo"], cb.z["p_bc_emo"][f].reshape(-1), rtol=0, atol=TOL_P)
    for f, out in enumerate(_run_oracle(cn)):
        for k in ("p_nod_short", "p_nod_long", "p_nod_long_p"):
            np.testing.assert_allclose(out[k], cn.z[k][f].reshape(-1), rtol=0, atol=TOL_P)
        n = min(f + 1, cn.T)
        np.testing.assert_allclose(out["p_bc"][:, :n], cn.z["p_bc"][f][:, :n], rtol=0, atol=TOL_P)


# ---- the group front-end with a model at half the leader's rate ---------------------------------------------------------------------
MODES = ("vap", "bc", "nod")
HZS, CTXS, HOP, S = (20, 20, 10), (50, 60, 30), 800, 3
A = engine.OUT_AUX


class MixedModel:
    """A scripted engine: stream slot s at its leader frame f.  vap and bc answer every frame; nod (R = 2) every second frame of a
    stream counted from its reset, with VAPX_STATUS_NO_FRAME in between.
    vap  p_now = [s, f]   bc  p_bc_react = 100 s + f   nod  short = s, long = its frame index, p_bc[r] = 1000 s + k + r / 64"""

    def __init__(self, poison=()):
        self.frames, self.phase, self.resets, self.calls = {}, {}, [], []
        self.poison = set(poison)                # (slot, leader frame since the stream's reset, mode): that row carries status 1

    def step(self, ids, audio, rows):
        self.calls.append(ids.tolist())
        for k, s in enumerate(int(i) for i in ids):
            f = self.frames.get(s, 0)
            self.frames[s] = f + 1
            rows["vap"][k, 0:2] = [s, f]
            rows["bc"][k, A + 1] = 100 * s + f
            ph = self.phase.get(s, 0) + 1
            if ph < 2:
                self.phase[s] = ph
                rows["nod"][k, :] = 0.0
                rows["nod"][k, engine.OUT_STATUS] = engine.STATUS_NO_FRAME
            else:
                self.phase[s] = 0
                kf = f // 2
                n = min(kf + 1, CTXS[2])
                rows["nod"][k, engine.OUT_NVALID] = n
                rows["nod"][k, A + 1], rows["nod"][k, A + 2] = s, kf
                rows["nod"][k, engine.OUT_LOGITS:engine.OUT_LOGITS + n] = [1000 * s + kf + r / 64 for r in range(n)]
            for m in MODES:
                if (s, f, m) in self.poison:
                    rows[m][k, engine.OUT_STATUS] = 1.0
        return 0

    def reset(self, sid):
        self.resets.append(sid)
        if sid >= 0:                             # a full reset restarts the stream's frame as well (vapx_reset_stream); carry-only does not
            self.frames[sid], self.phase[sid] = 0, 0


def _recv_exact(sock, n):
    b = b""
    while len(b) < n:
        chunk = sock.recv(n - len(b))
        assert chunk, "socket closed"
        b += chunk
    return b


def _read(sock, mode):
    sock.settimeout(10)
    ln = struct.unpack("<I", _recv_exact(sock, 4))[0]
    return ln, wire.decode_result(_recv_exact(sock, ln), mode)


def _wait(cond, timeout=5.0):
    t0 = time.time()
    while not cond() and time.time() - t0 < timeout:
        time.sleep(0.002)
    assert cond()


def _silent(sock):
    sock.setblocking(False)
    try:
        return sock.recv(1) == b"" and False
    except BlockingIOError:
        return True
    finally:
        sock.setblocking(True)


class _Rig:
    def __init__(self, model, **kw):
        kw.setdefault("max_wait_s", 0.5)
        self.srv = ingest.NativeServer.over_group_function(model.step, MODES, S, HZS, CTXS, reset=model.reset, **kw)
        self.ins, self.outs, self.n_out = [], {m: [] for m in MODES}, 0

    def connect(self):
        self.ins.append(socket.create_connection(("127.0.0.1", self.srv.port_in)))
        _wait(lambda: self.srv.stats()["in_connections"] == len(self.ins))
        for m in MODES:                                        # the k-th connection on a port hears the k-th dialogue
            self.outs[m].append(socket.create_connection(("127.0.0.1", self.srv.ports_out[m])))
            self.n_out += 1
            _wait(lambda: self.srv.stats()["out_connections"] == self.n_out)

    def close(self):
        self.srv.close()
        for s in self.ins + [c for l in self.outs.values() for c in l]:
            s.close()


def _nod_packet(sock, s, kf, x_hops):
    """One nod packet of dialogue s, its frame kf: the echo is exactly the two hops' samples, in order; the reference's layout."""
    ln, r = _read(sock, "nod")
    x1, x2 = np.concatenate([h[0] for h in x_hops]), np.concatenate([h[1] for h in x_hops])
    assert x1.size == 1600
    n = min(kf + 1, CTXS[2])
    want = {"t": r["t"], "x1": x1, "x2": x2, "p_bc": [1000 * s + kf + q / 64 for q in range(n)], "p_nod_short": [s],
            "p_nod_long": [kf], "p_nod_long_p": [0]}
    assert ln == len(wire.encode_result(want, "nod")) == 8 + 2 * (4 + 8 * 1600) + 4 + 8 * n + 3 * 12
    np.testing.assert_array_equal(r["x1"], x1)                 # float64 echo, bit-exact
    np.testing.assert_array_equal(r["x2"], x2)
    np.testing.assert_array_equal(r["p_bc"], np.asarray(want["p_bc"], np.float32).astype(np.float64))
    assert r["p_nod_short"][0] == s and r["p_nod_long"][0] == kf
    return 4 + ln


def test_slower_model_sends_one_packet_per_two_leader_frames_echoing_both_hops():
    """Two dialogues one leader frame apart: their nod frames fall on alternating ticks."""
    m = MixedModel()
    rig = _Rig(m)
    try:
        x = np.random.default_rng(5).standard_normal((2, 9, 2, HOP))
        rig.connect()
        rig.ins[0].sendall(wire.encode_input(x[0, 0, 0], x[0, 0, 1]))      # dialogue 0 is one frame ahead
        _, r = _read(rig.outs["vap"][0], "vap")
        assert list(r["p_now"]) == [0, 0]
        _, r = _read(rig.outs["bc"][0], "bc")
        assert r["p_bc_react"][0] == 0
        rig.connect()
        sent = {0: 1, 1: 0}
        nod_bytes = 0
        for t in range(8):
            for s in (0, 1):
                f = sent[s]
                rig.ins[s].sendall(wire.encode_input(x[s, f, 0], x[s, f, 1]))
                sent[s] += 1
            for s in (0, 1):
                f = sent[s] - 1
                ln, r = _read(rig.outs["vap"][s], "vap")                   # vap and bc: every frame, one hop echoed
                assert list(r["p_now"]) == [s, f] and len(r["x1"]) == HOP and np.array_equal(r["x1"], x[s, f, 0])
                ln, r = _read(rig.outs["bc"][s], "bc")
                assert r["p_bc_react"][0] == 100 * s + f and np.array_equal(r["x2"], x[s, f, 1])
                if f % 2:                                                  # exactly one of the two dialogues per tick
                    nod_bytes += _nod_packet(rig.outs["nod"][s], s, f // 2, [x[s, f - 1], x[s, f]])
        _wait(lambda: rig.srv.stats()["answered"] == 17)
        st = rig.srv.stats()
        assert st["frames_done"] == 17 and st["numeric_resets"] == 0 and m.resets == [0, 1]      # the two connections, nothing else
        assert all(_silent(c) for l in rig.outs.values() for c in l)                               # status 2 sent nothing, anywhere
        per_vap = 4 + len(wire.encode_result({"t": 0.0, "x1": x[0, 0, 0], "x2": x[0, 0, 1], "p_now": [0, 0], "p_future": [0, 0], "vad": [0, 0]}, "vap"))
        per_bc = 4 + len(wire.encode_result({"t": 0.0, "x1": x[0, 0, 0], "x2": x[0, 0, 1], "p_bc_react": [0], "p_bc_emo": [0]}, "bc"))
        assert st["tx_bytes"] == 17 * (per_vap + per_bc) + nod_bytes
    finally:
        rig.close()


def test_status_1_still_resets_and_restarts_the_slower_models_frame():
    m = MixedModel(poison=[(0, 5, "bc")])
    rig = _Rig(m)
    try:
        x = np.random.default_rng(6).standard_normal((10, 2, HOP))
        rig.connect()
        for f in range(10):
            rig.ins[0].sendall(wire.encode_input(x[f, 0], x[f, 1]))
            _wait(lambda: len(m.calls) == f + 1)
        # frames 0..4 answered; frame 5 (bc not finite) resets the dialogue and answers on no port — the hop nod had collected
        # (frame 4) is dropped with it; frames 6..9 are the reset stream's frames 0..3
        for f in list(range(5)) + [6, 7, 8, 9]:
            _, r = _read(rig.outs["vap"][0], "vap")
            assert list(r["p_now"]) == [0, f if f < 5 else f - 6] and np.array_equal(r["x1"], x[f, 0])
        _nod_packet(rig.outs["nod"][0], 0, 0, [x[0], x[1]])
        _nod_packet(rig.outs["nod"][0], 0, 1, [x[2], x[3]])
        _nod_packet(rig.outs["nod"][0], 0, 0, [x[6], x[7]])
        _nod_packet(rig.outs["nod"][0], 0, 1, [x[8], x[9]])
        _wait(lambda: rig.srv.stats()["answered"] == 9)
        assert rig.srv.stats()["numeric_resets"] == 1 and m.resets == [0, 0]                       # the connection, then the poisoned frame
        assert _silent(rig.outs["nod"][0]) and _silent(rig.outs["vap"][0])
    finally:
        rig.close()


def test_open_group_fn2_refusals():
    m = MixedModel()
    with pytest.raises(engine.VapxError, match="integer multiple"):
        ingest.NativeServer.over_group_function(m.step, ("vap", "bc"), S, (50, 20), (50, 50))
    with pytest.raises(engine.VapxError, match="fastest model"):
        ingest.NativeServer.over_group_function(m.step, ("vap", "bc"), S, (10, 20), (50, 50))


# ---- TrunkGroup / serve arguments ----------------------------------------------------------------------------------------------------
def test_trunk_plan_picks_the_fastest_leader_and_each_models_geometry():
    p = engine.trunk_plan(["nod", "vap", "bc"], {"vap": 20, "bc": 20, "nod": 10}, [10.0, 2.5, 5.0])
    assert p["leader"] == "vap" and p["order"] == ["vap", "nod", "bc"]                              # ties: blobs order
    assert p["R"] == {"nod": 2, "vap": 1, "bc": 1} and p["T"] == {"nod": 100, "vap": 50, "bc": 100}
    assert p["hop"] == {"nod": 1600, "vap": 800, "bc": 800} and p["L"]["nod"] == 1920
    q = engine.trunk_plan(["bc", "nod"], 20, 2.5)                                                   # scalars mean what they meant
    assert q["leader"] == "bc" and q["R"] == {"bc": 1, "nod": 1} and q["T"] == {"bc": 50, "nod": 50}
    for hz_l, hz_f in ((50, 10), (50, 5), (20, 10), (20, 5), (10, 5)):
        assert engine.trunk_plan(["vap", "nod"], [hz_l, hz_f], 1.0)["R"]["nod"] == hz_l // hz_f
    assert engine.trunk_plan(["vap", "nod"], [10, 20], 1.0)["leader"] == "nod"
    with pytest.raises(engine.VapxError, match="integer multiple"):
        engine.trunk_plan(["vap", "nod"], [50, 20], 1.0)
    with pytest.raises(engine.VapxError, match="one per model"):
        engine.trunk_plan(["vap", "nod"], [20, 20, 10], 1.0)
    with pytest.raises(engine.VapxError, match="names"):
        engine.trunk_plan(["vap", "nod"], {"vap": 20}, 1.0)
    with pytest.raises(engine.VapxError, match="5, 10, 20 or 50"):
        engine.trunk_plan(["vap", "nod"], [20, 4], 1.0)


def _args(**kw):
    import argparse
    a = argparse.Namespace(vap_process_rate="20", context_len_sec="2.5", save_state=None, load_state=None)
    a.__dict__.update(kw)
    return a


def test_serve_takes_one_rate_and_window_per_model_and_refuses_what_the_trunk_cannot_serve():
    names = ["vap", "bc", "nod"]
    p = serve.group_plan(_args(vap_process_rate="20,20,10", context_len_sec="2.5,5,10"), names)
    assert p["order"][0] == "vap" and p["R"]["nod"] == 2 and p["T"] == {"vap": 50, "bc": 100, "nod": 100}
    p = serve.group_plan(_args(), names)                                                           # a single value applies to all
    assert p["hz"] == {m: 20 for m in names} and p["T"] == {m: 50 for m in names}
    assert serve.group_plan(_args(save_state="s.bin"), names)["R"]["nod"] == 1                    # equal group: snapshots as before
    with pytest.raises(ValueError, match="2 value"):
        serve.group_plan(_args(vap_process_rate="20,10"), names)
    with pytest.raises(ValueError, match="integer multiple"):
        serve.group_plan(_args(vap_process_rate="50,20,10"), names)
    with pytest.raises(ValueError, match="half-collected frame"):
        serve.group_plan(_args(vap_process_rate="20,20,10", save_state="s.bin"), names)
    with pytest.raises(ValueError, match="half-collected frame"):
        serve.group_plan(_args(vap_process_rate="20,20,10", load_state="s.bin"), names)
    with pytest.raises(ValueError, match="different windows"):
        serve.group_plan(_args(context_len_sec="2.5,5,5", save_state="s.bin"), names)
    with pytest.raises(SystemExit):                                                                # argparse's error exit, before any device work
        serve.main(["--mode", "vap+nod", "--vap_process_rate", "50,20", "--synthetic-weights", "1"])
    with pytest.raises(SystemExit):
        serve.main(["--mode", "vap+nod", "--vap_process_rate", "20,10", "--save_state", "s.bin", "--synthetic-weights", "1"])
    with pytest.raises(SystemExit):
        serve.main(["--vap_process_rate", "20,10", "--synthetic-weights", "1"])                    # one model, two rates


def test_capacity_prices_every_model_at_its_own_rate_and_window():
    same = capacity.plan(1024, 20, 2.5, "vap+bc+nod")
    mixed_same = capacity.plan_mixed(1024, [("vap", 20, 2.5), ("bc", 20, 2.5), ("nod", 20, 2.5)])
    for p in ("fp32", "split"):
        assert mixed_same[p]["busy"] == pytest.approx(same[p]["busy"], rel=1e-12)
    pub = capacity.plan_mixed(1024, [("vap", 20, 2.5), ("bc", 20, 5.0), ("nod", 10, 10.0)])
    assert [r["ctx_frames"] for r in pub["models"]] == [50, 100, 100]
    assert pub["fp32"]["busy"] == pytest.approx(sum(r["fp32"]["busy"] for r in pub["models"]))
    assert pub["fp32"]["busy"] > same["fp32"]["busy"]                                              # the leader's window alone under-counts
    nod20 = capacity.plan_mixed(1024, [("vap", 20, 2.5), ("bc", 20, 5.0), ("nod", 20, 5.0)])
    assert pub["models"][2]["fp32"]["busy"] == pytest.approx(nod20["models"][2]["fp32"]["busy"] / 2, rel=0.02)   # same T = 100, half the frames
