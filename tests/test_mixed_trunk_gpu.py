"""Mixed trunk groups: models with different windows and frame rates on one CPC CNN + LSTM pass per leader tick.

The mix_* goldens are the reference's three programs run side by side on one cpc_model file and the same 64 320 samples:
vap at 20 Hz / 2.5 s (T = 50, leads), bc at 20 Hz / 3 s (T = 60) and nod at 10 Hz / 3 s (T = 30, one frame per two leader ticks).
Every comparison is at the project's parity bar of 1e-4."""
import functools

import numpy as np
import pytest

from golden_util import Case

pytestmark = pytest.mark.gpu

TOL = 1e-4
NAMES = {"vap": "mix_vap20", "bc": "mix_bc20_3s", "nod": "mix_nod10_3s"}


@functools.lru_cache(maxsize=None)
def _cases():
    return {m: Case(n) for m, n in NAMES.items()}


def _group(max_streams=2, **kw):
    from vap_realtime_amd import engine, weights as W
    cases = _cases()
    blobs = {m: W.pack_blob(cases[m].cpc_sd, cases[m].vap_sd, m) for m in ("vap", "bc", "nod")}
    hz = {m: cases[m].frame_hz for m in blobs}
    ctx = {m: cases[m].ctx_sec for m in blobs}
    return cases, engine.TrunkGroup(blobs, hz, ctx, max_streams=max_streams, **kw)


def _check_rows(mode, rows, f, gs, what=""):
    """rows [k, >= 16] of `mode` (output or wire rows) against frame f (the model's own frame index) of golden streams gs."""
    from vap_realtime_amd import engine as E
    z = _cases()[mode].z
    msg = f"{mode} frame {f} {what}"
    assert (rows[:, E.OUT_STATUS] == 0).all(), msg
    full = rows.shape[1] == E.OUT_STRIDE
    if mode == "vap":
        for k, at in (("p_now", E.OUT_P_NOW), ("p_future", E.OUT_P_FUTURE), ("vad", E.OUT_VAD)):
            np.testing.assert_allclose(rows[:, at:at + 2], z[k][f][gs], rtol=0, atol=TOL, err_msg=msg + k)
        if full:
            np.testing.assert_allclose(rows[:, E.OUT_LOGITS:E.OUT_LOGITS + 256], z["logits"][f][gs], rtol=0, atol=TOL, err_msg=msg + "logits")
            es = int(z["meta.e_stride"])
            if f % es == 0:
                np.testing.assert_allclose(rows[:, E.OUT_E:E.OUT_E + 512].reshape(-1, 2, 256), z["e"][f // es][gs], rtol=0, atol=TOL,
                                           err_msg=msg + "e")
    elif mode == "bc":
        np.testing.assert_allclose(rows[:, E.OUT_AUX + 1], z["p_bc_react"][f].reshape(-1)[gs], rtol=0, atol=TOL, err_msg=msg)
        np.testing.assert_allclose(rows[:, E.OUT_AUX + 2], z["p_bc_emo"][f].reshape(-1)[gs], rtol=0, atol=TOL, err_msg=msg)
    else:
        for i, k in enumerate(("p_nod_short", "p_nod_long", "p_nod_long_p")):
            np.testing.assert_allclose(rows[:, E.OUT_AUX + 1 + i], z[k][f].reshape(-1)[gs], rtol=0, atol=TOL, err_msg=msg + k)
        n = min(f + 1, _cases()["nod"].T)
        assert (rows[:, E.OUT_NVALID] == n).all(), msg
        np.testing.assert_allclose(rows[:, E.OUT_LOGITS:E.OUT_LOGITS + n], z["p_bc"][f][gs][:, :n], rtol=0, atol=TOL, err_msg=msg + "p_bc")


def _check_no_frame(rows, what=""):
    from vap_realtime_amd import engine as E
    assert (rows[:, E.OUT_STATUS] == E.STATUS_NO_FRAME).all(), what
    rest = np.delete(rows, E.OUT_STATUS, axis=1)
    assert not rest.any(), what


@pytest.mark.parametrize("split_f16", [False, True], ids=["fp32", "split_f16"])
@pytest.mark.parametrize("api", ["step", "step_wire"])
def test_three_models_one_trunk_three_reference_programs(api, split_f16):
    cases, grp = _group(split_f16=split_f16)
    c = cases["vap"]
    assert grp.order[0] == "vap" and grp.R == {"vap": 1, "bc": 1, "nod": 2} and grp.T_of == {"vap": 50, "bc": 60, "nod": 30}
    both = [0, 1]
    for f in range(c.n_frames):
        res = getattr(grp, api)(c.new_samples(f))
        _check_rows("vap", res["vap"], f, both)
        _check_rows("bc", res["bc"], f, both)
        due = grp.due("nod", res["nod"])
        assert due.all() if f % 2 else not due.any()
        if f % 2:
            _check_rows("nod", res["nod"], f // 2, both)
        else:
            _check_no_frame(res["nod"], f"tick {f}")
        if api == "step_wire":
            assert res["nod"].shape == (2, grp.wire_floats("nod")) and grp.wire_floats("nod") == 16 + 32 and grp.leader.group_bad() == []
    grp.close()


def test_phases_are_per_stream_under_ragged_reordered_batches():
    """Stream 81 joins one leader frame after stream 80, so exactly one of them has a nod frame due on every tick; the batch order
    swaps on every third tick; host ids that are not identity."""
    cases, grp = _group(max_streams=8)
    c = cases["vap"]
    sid = {0: 5, 1: 2}                                           # golden stream index -> stream slot
    for t in range(c.n_frames):
        members = [(0, t)] + ([(1, t - 1)] if t >= 1 else [])    # (golden stream, its own leader frame)
        if t % 3 == 2:
            members.reverse()
        audio = np.stack([c.audio[g, :, f * c.hop:(f + 1) * c.hop] for g, f in members])
        res = grp.step(audio, [sid[g] for g, _ in members])
        n_due = 0
        for i, (g, f) in enumerate(members):
            _check_rows("vap", res["vap"][i:i + 1], f, [g], f"tick {t}")
            _check_rows("bc", res["bc"][i:i + 1], f, [g], f"tick {t}")
            if f % 2:
                n_due += 1
                _check_rows("nod", res["nod"][i:i + 1], f // 2, [g], f"tick {t}")
            else:
                _check_no_frame(res["nod"][i:i + 1], f"tick {t} slot {i}")
        assert n_due == (1 if t >= 1 else 0)
        for m in grp.modes:
            assert grp.engines[m].bad_slots() == []
    grp.close()


def test_reset_in_mid_accumulation_restarts_the_frame():
    cases, grp = _group()
    c = cases["vap"]
    for f in range(7):                                           # an odd number of leader frames: stream 0 holds half a nod frame
        grp.step(c.new_samples(f))
    grp.reset_stream(0)
    for j in range(24):
        audio = np.stack([c.audio[0, :, j * c.hop:(j + 1) * c.hop], c.audio[1, :, (7 + j) * c.hop:(8 + j) * c.hop]])
        res = grp.step(audio)
        for i, f in ((0, j), (1, 7 + j)):
            _check_rows("vap", res["vap"][i:i + 1], f, [i])
            _check_rows("bc", res["bc"][i:i + 1], f, [i])
            if f % 2:
                _check_rows("nod", res["nod"][i:i + 1], f // 2, [i], f"after reset, j={j}")
            else:
                _check_no_frame(res["nod"][i:i + 1])
    grp.close()


@pytest.mark.parametrize("mode,hz_f,hz_l", [("nod", 10, 50), ("vap", 5, 20), ("bc", 5, 10)], ids=["50to10", "20to5", "10to5"])
def test_other_ratios_follower_equals_standalone_engine(mode, hz_f, hz_l):
    """No golden for these pairs: the follower against a stand-alone engine of the same weights fed the same audio (that engine is
    golden- and oracle-pinned by test_engine_gpu).  Three streams, 4·R leader frames past the follower's window of 4 frames.
    Measured on MI355X over the whole output row: 6.4e-6 (50 -> 10), 6.9e-6 (20 -> 5), 8.5e-6 (10 -> 5)."""
    from vap_realtime_amd import engine as E, synth, weights as W
    R, Tf = hz_l // hz_f, 4
    lmode = "bc" if mode == "vap" else "vap"
    cpc = W.synthetic_weights(41, hz_l, "vap")[0]
    blob_f = W.pack_blob(cpc, W.synthetic_weights(42, hz_f, mode)[1], mode)
    blob_l = W.pack_blob(cpc, W.synthetic_weights(43, hz_l, lmode)[1], lmode)
    grp = E.TrunkGroup({mode: blob_f, lmode: blob_l}, {mode: hz_f, lmode: hz_l}, {mode: Tf / hz_f, lmode: 1.0}, max_streams=3)
    assert grp.order[0] == lmode and grp.R[mode] == R and grp.T_of[mode] == Tf
    solo = E.Engine(blob_f, hz_f, Tf / hz_f, max_streams=3, mode=mode)
    hop_l, ticks = 16000 // hz_l, R * (Tf + 4)
    audio = synth.dialogue_batch([90, 91, 92], hop_l * ticks)
    worst = 0.0
    for t in range(ticks):
        got = grp.step(audio[:, :, t * hop_l:(t + 1) * hop_l])[mode]
        if (t + 1) % R:
            _check_no_frame(got, f"tick {t}")
            continue
        k = (t + 1) // R - 1
        want = solo.step(audio[:, :, k * R * hop_l:(k + 1) * R * hop_l])
        assert (got[:, E.OUT_STATUS] == 0).all() and np.array_equal(got[:, E.OUT_NVALID], want[:, E.OUT_NVALID])
        worst = max(worst, float(np.abs(got - want).max()))
        np.testing.assert_allclose(got, want, rtol=0, atol=TOL, err_msg=f"follower frame {k}")
    print(f"ratio {hz_l}->{hz_f} ({mode}): max |follower - stand-alone| = {worst:.3e}")
    solo.close()
    grp.close()


def test_overlap_groups_split_the_due_streams():
    """64 streams on two overlap groups, R = 2, the golden audio tiled: due sets of 0, 64 (two groups of 32), 0 (of 40), 40 and 24."""
    from vap_realtime_amd import engine as E, weights as W
    cases = _cases()
    c = cases["vap"]
    blobs = {m: W.pack_blob(cases[m].cpc_sd, cases[m].vap_sd, m) for m in ("vap", "nod")}
    grp = E.TrunkGroup(blobs, {"vap": 20, "nod": 10}, {"vap": 2.5, "nod": 3.0}, max_streams=64, groups=2)
    frame = [0] * 64                                             # each stream's own next leader frame
    plan = [range(64), range(64), range(40), range(64), range(64), range(64)]
    want_due = [0, 64, 0, 40, 24, 40]
    for t, members in enumerate(plan):
        members = list(members)
        audio = np.stack([c.audio[s % 2, :, frame[s] * c.hop:(frame[s] + 1) * c.hop] for s in members])
        res = grp.step(audio, members)
        assert int(grp.due("nod", res["nod"]).sum()) == want_due[t], f"tick {t}"
        for i, s in enumerate(members):
            f = frame[s]
            _check_rows("vap", res["vap"][i:i + 1], f, [s % 2], f"tick {t} stream {s}")
            if f % 2:
                _check_rows("nod", res["nod"][i:i + 1], f // 2, [s % 2], f"tick {t} stream {s}")
            else:
                _check_no_frame(res["nod"][i:i + 1], f"tick {t} stream {s}")
            frame[s] += 1
    grp.close()


def test_refusals_say_why_and_touch_no_stream():
    import torch
    from vap_realtime_amd import engine as E, weights as W
    from vap_realtime_amd.engine import VapxError
    cases = _cases()
    c = cases["vap"]
    cpc = c.cpc_sd

    def eng(mode, hz, seed=44, ctx=1.0):
        return E.Engine(W.pack_blob(cpc, W.synthetic_weights(seed, hz, mode)[1], mode), hz, ctx, max_streams=2, mode=mode)
    e50, e20, e10 = eng("vap", 50), eng("bc", 20), eng("nod", 10)
    with pytest.raises(VapxError, match="not an integer multiple"):
        e20.attach_trunk(e50)                                   # 50 -> 20
    with pytest.raises(VapxError, match="slower than this follower"):
        e20.attach_trunk(e10)                                   # the leader must be the fastest model
    with pytest.raises(VapxError, match="integer multiple"):
        E.trunk_plan(["vap", "bc"], [50, 20], 1.0)
    # both refused engines are still stand-alone engines
    a = np.zeros((2, 2, 800), np.float32)
    assert e20.step(a).shape == (2, E.OUT_STRIDE)
    for e in (e50, e20, e10):
        e.close()

    cases, grp = _group()
    nod = grp.engines["nod"]
    for f in range(3):
        grp.step(c.new_samples(f))                              # nod: one frame done, half of the next collected
    assert nod.get_state(0)["n_frames"] == 1
    # device ids on the leader's step: the host cannot know who is due
    dev = torch.device("cuda")
    ad = torch.from_numpy(np.ascontiguousarray(c.new_samples(3), dtype=np.float32)).to(dev)
    ids = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    outs = {m: torch.zeros((2, E.OUT_STRIDE), dtype=torch.float32, device=dev) for m in grp.modes}
    grp.leader.step_device(2, ad.data_ptr(), c.hop, outs["vap"].data_ptr(), ids_ptr=ids.data_ptr())
    grp.engines["bc"].step_follow_device(2, outs["bc"].data_ptr())       # a same-rate follower takes device ids
    with pytest.raises(VapxError, match="device stream ids"):
        nod.step_follow_device(2, outs["nod"].data_ptr())
    torch.cuda.synchronize()
    assert nod.get_state(0)["n_frames"] == 1 and nod.get_state(1)["n_frames"] == 1
    # bulk state records of a slower follower
    with pytest.raises(VapxError, match="refused on a trunk follower at 1/2"):
        nod.export_streams([0, 1])
    with pytest.raises(VapxError, match="refused on a trunk follower at 1/2"):
        grp.export_streams()
    rec = np.zeros((2, E.state_record_floats(30, follower=True)), np.float32)
    with pytest.raises(VapxError, match="refused on a trunk follower at 1/2"):
        nod.import_streams([0, 1], rec)
    assert nod.get_state(0)["n_frames"] == 1 and nod.get_state(1)["n_frames"] == 1
    # a same-rate follower with a window of its own exports and imports as before
    bc = grp.engines["bc"]
    recs = bc.export_streams([0, 1])
    assert E.split_state(recs, 60, follower=True)["ctx_frames"].tolist() == [60, 60]
    bc.import_streams([0, 1], recs)
    grp.close()


def _read_packet(sock, mode, timeout=20):
    import struct
    from vap_realtime_amd import wire
    sock.settimeout(timeout)
    hdr = b""
    while len(hdr) < 4:
        hdr += sock.recv(4 - len(hdr))
    ln = struct.unpack("<I", hdr)[0]
    payload = b""
    while len(payload) < ln:
        payload += sock.recv(ln - len(payload))
    return ln, payload, wire.decode_result(payload, mode)


def test_mixed_group_tcp_front_end_end_to_end():
    """The three programs behind ONE input port at the leader's framing: vap and bc answer every 800-sample frame, nod every second
    one with a packet that echoes 1600 samples per channel — byte for byte the reference's nod codec with n = 1600."""
    import socket
    import time
    from vap_realtime_amd import ingest, wire
    cases, grp = _group(max_streams=4)
    c, cn = cases["vap"], cases["nod"]
    S = 2
    srv = ingest.NativeServer.for_group(grp, port_in=0, ports_out=[0, 0, 0], max_wait_s=0.5)
    try:
        ins = [socket.create_connection(("127.0.0.1", srv.port_in)) for _ in range(S)]
        while srv.stats()["in_connections"] < S:
            time.sleep(0.01)
        outs = {}
        for k, m in enumerate(grp.modes):
            outs[m] = [socket.create_connection(("127.0.0.1", srv.ports_out[m])) for _ in range(S)]
            while srv.stats()["out_connections"] < (k + 1) * S:
                time.sleep(0.01)
        for f in range(c.n_frames):
            new = c.new_samples(f).astype(np.float64)
            for p in range(c.hop // 160):
                for s in range(S):
                    ins[s].sendall(wire.encode_input(new[s, 0, p * 160:(p + 1) * 160], new[s, 1, p * 160:(p + 1) * 160]))
            for s in range(S):
                ln, _, r = _read_packet(outs["vap"][s], "vap")
                assert ln == 12876
                np.testing.assert_array_equal(r["x1"], new[s, 0])
                for k in ("p_now", "p_future", "vad"):
                    np.testing.assert_allclose(r[k], c.z[k][f][s], rtol=0, atol=TOL)
                _, _, r = _read_packet(outs["bc"][s], "bc")
                np.testing.assert_array_equal(r["x2"], new[s, 1])
                np.testing.assert_allclose(r["p_bc_react"], cases["bc"].z["p_bc_react"][f][s], rtol=0, atol=TOL)
                np.testing.assert_allclose(r["p_bc_emo"], cases["bc"].z["p_bc_emo"][f][s], rtol=0, atol=TOL)
                if f % 2:
                    kf = f // 2
                    ln, payload, r = _read_packet(outs["nod"][s], "nod")
                    both = cn.new_samples(kf).astype(np.float64)              # the 10 Hz program's 1600 new samples of its frame kf
                    np.testing.assert_array_equal(r["x1"], both[s, 0])
                    np.testing.assert_array_equal(r["x2"], both[s, 1])
                    n = min(kf + 1, cn.T)
                    assert len(r["p_bc"]) == n
                    np.testing.assert_allclose(r["p_bc"], cn.z["p_bc"][kf][s][:n], rtol=0, atol=TOL)
                    for k in ("p_nod_short", "p_nod_long", "p_nod_long_p"):
                        np.testing.assert_allclose(r[k], cn.z[k][kf][s], rtol=0, atol=TOL)
                    assert payload == wire.encode_result(r, "nod") and ln == 8 + 2 * (4 + 8 * 1600) + 4 + 8 * n + 3 * 12
        st = srv.stats()
        assert st["frames_done"] == S * c.n_frames and st["numeric_resets"] == 0 and st["dropped_listeners"] == 0
        for sock in ins + [x for l in outs.values() for x in l]:
            sock.close()
    finally:
        srv.close()
        grp.close()
