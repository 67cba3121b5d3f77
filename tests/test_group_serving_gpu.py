"""Multi-model serving on one shared CPC trunk, from the engine's one-call group step (vapx_step_group: every model
device-resident, wire rows gathered by wire_pack_kernel, one compact copy) up to the TCP front-end (vapx_ingest_open_group) and the
``serve --mode a+b`` program — against the goldens of the three reference programs run side by side on one cpc_model file
(trunk_vap20 / trunk_bc20 / trunk_nod20: 2 streams, 54 frames, 20 Hz, T = 50: warm-up, a full window, four slides of the ring)."""
import os
import re
import signal
import socket
import struct
import subprocess
import sys
import time

import numpy as np
import pytest

from golden_util import Case

pytestmark = pytest.mark.gpu

TOL = 1e-4          # the project's parity bar (tests/test_trunk_gpu.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASES = {}


def _cases():
    if not _CASES:
        _CASES.update({"vap": Case("trunk_vap20"), "bc": Case("trunk_bc20"), "nod": Case("trunk_nod20")})
    return _CASES


def _group(order=("vap", "bc", "nod"), max_streams=2, **kw):
    from vap_realtime_amd import engine, weights as W
    cases = _cases()
    blobs = {m: W.pack_blob(cases[m].cpc_sd, cases[m].vap_sd, m) for m in order}
    c = cases["vap"]
    return cases, engine.TrunkGroup(blobs, c.frame_hz, c.ctx_sec, max_streams=max_streams, **kw)


def _check_wire_frame(cases, res, f):
    """The fields tests/test_trunk_gpu.py compares, minus vap ``logits`` (a wire row does not carry them)."""
    from vap_realtime_amd.engine import split_wire
    cv, cb, cn = cases["vap"], cases["bc"], cases["nod"]
    if "vap" in res:
        o = split_wire("vap", res["vap"])
        for k in ("p_now", "p_future", "vad"):
            np.testing.assert_allclose(o[k], cv.z[k][f], rtol=0, atol=TOL, err_msg=f"vap {k} frame {f}")
    if "bc" in res:
        o = split_wire("bc", res["bc"])
        np.testing.assert_allclose(o["aux"][:, 1], cb.z["p_bc_react"][f].reshape(-1), rtol=0, atol=TOL, err_msg=f"bc frame {f}")
        np.testing.assert_allclose(o["aux"][:, 2], cb.z["p_bc_emo"][f].reshape(-1), rtol=0, atol=TOL, err_msg=f"bc frame {f}")
    if "nod" in res:
        o = split_wire("nod", res["nod"])
        for i, k in ((1, "p_nod_short"), (2, "p_nod_long"), (3, "p_nod_long_p")):
            np.testing.assert_allclose(o["aux"][:, i], cn.z[k][f].reshape(-1), rtol=0, atol=TOL, err_msg=f"nod {k} frame {f}")
        n = min(f + 1, cn.T)
        assert o["n"].tolist() == [n, n]
        np.testing.assert_allclose(o["p_bc_rows"][:, :n], cn.z["p_bc"][f][:, :n], rtol=0, atol=TOL, err_msg=f"nod p_bc frame {f}")
    for m in res:
        assert not res[m][:, 13].any(), f"{m} status frame {f}"


@pytest.mark.parametrize("order", [("vap", "bc", "nod"), ("nod", "vap")])
def test_step_group_wire_rows_match_the_reference_programs(order):
    from vap_realtime_amd import engine
    cases, grp = _group(order)
    c = cases["vap"]
    assert grp.leader.group_wire_floats() == sum(engine.wire_floats(m, c.T) for m in order)
    pinned = engine.pinned_empty(2 * grp.leader.group_wire_floats())     # vapx_host_alloc memory: copied straight
    for f in range(c.n_frames):
        res = grp.step_wire(c.new_samples(f), out=pinned if f % 2 else None)
        assert list(res) == list(order) and all(res[m].shape == (2, engine.wire_floats(m, c.T)) for m in order)
        _check_wire_frame(cases, res, f)
    assert grp.leader.group_bad() == []
    grp.close()


@pytest.mark.parametrize("split_f16", [False, True], ids=["fp32", "split"])
def test_wire_rows_are_bit_identical_to_the_head_of_the_separate_steps_rows(split_f16):
    """Two groups, same weights and flags, one stepped with TrunkGroup.step (a host-output vapx_step per model), one with step_wire:
    the same kernels with the same launch shapes, so every wire row IS the first wire_floats floats of the matching output row.
    Permuted ids in a 5-slot table, stream 4 reset at frame 17 (the reset cascades from the leader)."""
    from vap_realtime_amd import engine
    order = ("vap", "bc", "nod")
    cases, a = _group(order, max_streams=5, split_f16=split_f16)
    _, b = _group(order, max_streams=5, split_f16=split_f16)
    c = cases["vap"]
    ids = [4, 1]
    for f in range(30):
        if f == 17:
            a.reset_stream(4)
            b.reset_stream(4)
        x = c.new_samples(f)
        full, wire_rows = a.step(x, ids), b.step_wire(x, ids)
        for m in order:
            wf = engine.wire_floats(m, c.T)
            np.testing.assert_array_equal(wire_rows[m], full[m][:, :wf], err_msg=f"{m} frame {f}")
    assert wire_rows["nod"][:, 10].tolist() == [13.0, 30.0]               # stream 4 restarted at frame 17
    # state and peeks behave after step_group as after the separate calls
    for m in order:
        sa, sb = a.engines[m].get_state(1), b.engines[m].get_state(1)
        assert sa["n_frames"] == sb["n_frames"] == 30
        np.testing.assert_array_equal(sa["ring"], sb["ring"])
    np.testing.assert_array_equal(a.leader.get_state(4)["lstm"], b.leader.get_state(4)["lstm"])
    np.testing.assert_array_equal(a.leader.peek("e", (2, 2, 256)), b.leader.peek("e", (2, 2, 256)))
    a.close()
    b.close()


def test_step_group_refusals_and_device_output():
    import torch
    from vap_realtime_amd import engine
    from vap_realtime_amd.engine import VapxError
    order = ("bc", "nod")
    cases, grp = _group(order)
    _, twin = _group(order)
    c = cases["vap"]
    with pytest.raises(VapxError, match="follower"):
        grp.engines["nod"].step_group(c.new_samples(0))
    grp.leader.step(c.new_samples(0))                       # a plain leader step leaves the follower behind ...
    with pytest.raises(VapxError, match="has not consumed"):
        grp.leader.step_group(c.new_samples(1))
    grp.engines["nod"].step_follow(2)                       # ... until it has followed
    twin.step_wire(c.new_samples(0))
    # device output: no copy, no synchronisation; the block on the device equals the host path's
    per = grp.leader.group_wire_floats()
    x = torch.from_numpy(np.ascontiguousarray(c.new_samples(1), np.float32)).cuda()
    dev = torch.full((2 * per,), -7.0, device="cuda")
    grp.leader.step_group_device(2, x.data_ptr(), c.hop, dev.data_ptr())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), twin.leader.step_group(c.new_samples(1)))
    grp.close()
    twin.close()


def test_a_poisoned_stream_is_named_per_model_and_the_others_equal_a_clean_twin():
    from vap_realtime_amd import engine
    order = ("vap", "bc", "nod")
    cases, grp = _group(order, max_streams=3)
    _, twin = _group(order, max_streams=3)
    c = cases["vap"]

    def audio(f):
        x = c.new_samples(f)
        return np.concatenate([x, x[:1]])

    for f in range(3):
        grp.step_wire(audio(f))
        twin.step_wire(audio(f))
    st = grp.leader.get_state(1)
    st["lstm"][:] = np.inf
    grp.leader.set_state(1, st)
    with pytest.raises(engine.VapxError, match="non-finite outputs for batch slot 1"):
        grp.step_wire(audio(3))
    assert grp.leader.group_bad() == [(1, 0), (1, 1), (1, 2)]
    got = grp.step_wire(audio(4), on_numeric="status")      # the LSTM state keeps it; the block is complete
    twin.step_wire(audio(3))
    want = twin.step_wire(audio(4))
    assert sorted(grp.leader.group_bad()) == [(1, 0), (1, 1), (1, 2)]
    for m in order:
        assert got[m][:, engine.OUT_STATUS].tolist() == [0.0, 1.0, 0.0]
        assert np.isfinite(got[m][[0, 2]]).all()
        np.testing.assert_array_equal(got[m][[0, 2]], want[m][[0, 2]])
    grp.reset_stream(1)
    out = grp.step_wire(audio(5))
    assert all(np.isfinite(out[m][:, :10]).all() and not out[m][:, engine.OUT_STATUS].any() for m in order)
    assert grp.leader.group_bad() == []
    grp.close()
    twin.close()


def _read_packet(sock, mode, timeout=20):
    from vap_realtime_amd import wire
    sock.settimeout(timeout)
    hdr = b""
    while len(hdr) < 4:
        hdr += sock.recv(4 - len(hdr))
    ln = struct.unpack("<I", hdr)[0]
    payload = b""
    while len(payload) < ln:
        payload += sock.recv(ln - len(payload))
    return ln, wire.decode_result(payload, mode)


def test_group_tcp_front_end_end_to_end_on_gpu():
    """Three reference programs' worth of serving behind ONE input port: reference-format packets in, each model's reference-format
    packets out on its own port, every field == the golden of that program, echo bit-exact."""
    from vap_realtime_amd import ingest, wire
    order = ("vap", "bc", "nod")
    cases, grp = _group(order, max_streams=4)
    c = cases["vap"]
    S = 2
    srv = ingest.NativeServer.for_group(grp, port_in=0, ports_out=[0, 0, 0], max_wait_s=0.5)
    try:
        assert set(srv.ports_out) == set(order) and len(set(srv.ports_out.values())) == 3
        ins = [socket.create_connection(("127.0.0.1", srv.port_in)) for _ in range(S)]
        while srv.stats()["in_connections"] < S:
            time.sleep(0.01)
        outs = {}
        for k, m in enumerate(order):
            outs[m] = [socket.create_connection(("127.0.0.1", srv.ports_out[m])) for _ in range(S)]
            while srv.stats()["out_connections"] < (k + 1) * S:
                time.sleep(0.01)
        for f in range(c.n_frames):
            new = c.new_samples(f).astype(np.float64)
            for p in range(c.hop // 160):
                for s in range(S):
                    ins[s].sendall(wire.encode_input(new[s, 0, p * 160:(p + 1) * 160], new[s, 1, p * 160:(p + 1) * 160]))
            for m in order:
                z = cases[m].z
                for s in range(S):
                    ln, r = _read_packet(outs[m][s], m)
                    np.testing.assert_array_equal(r["x1"], new[s, 0])
                    np.testing.assert_array_equal(r["x2"], new[s, 1])
                    if m == "vap":
                        assert ln == 12876
                        for k in ("p_now", "p_future", "vad"):
                            np.testing.assert_allclose(r[k], z[k][f][s], rtol=0, atol=TOL)
                    elif m == "bc":
                        np.testing.assert_allclose(r["p_bc_react"], z["p_bc_react"][f][s], rtol=0, atol=TOL)
                        np.testing.assert_allclose(r["p_bc_emo"], z["p_bc_emo"][f][s], rtol=0, atol=TOL)
                    else:
                        n = min(f + 1, c.T)
                        assert len(r["p_bc"]) == n                                  # every window row (vap_nod_main.py:276 quirk)
                        np.testing.assert_allclose(r["p_bc"], z["p_bc"][f][s][:n], rtol=0, atol=TOL)
                        for k in ("p_nod_short", "p_nod_long", "p_nod_long_p"):
                            np.testing.assert_allclose(r[k], z[k][f][s], rtol=0, atol=TOL)
        st = srv.stats()
        assert st["frames_done"] == S * c.n_frames and st["numeric_resets"] == 0 and st["dropped_listeners"] == 0
        for s in ins + [x for l in outs.values() for x in l]:
            s.close()
    finally:
        srv.close()
        grp.close()


def test_serve_program_with_a_plus_mode():
    """``python -m vap_realtime_amd.serve --mode bc+nod``: vap_bc_main.py and vap_nod_main.py side by side on one cpc_model, one input
    port; both output ports answer every frame in their own framing; SIGTERM stops it cleanly.  The front door is single-model."""
    from vap_realtime_amd import synth, wire
    hop = 800
    proc = subprocess.Popen([sys.executable, "-u", "-m", "vap_realtime_amd.serve", "--mode", "bc+nod", "--synthetic-weights", "3", "--streams", "2",
                             "--port_num_in", "0", "--port_num_out", "0,0", "--stats_sec", "0"],
                            cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        line = ""
        t0 = time.time()
        while "input :" not in line and time.time() - t0 < 180:
            line = proc.stdout.readline()
            assert line or proc.poll() is None, "serve exited early"
        pin, pbc, pnod = (int(x) for x in re.search(r"input :(\d+), output bc :(\d+), nod :(\d+)", line).groups())
        assert "bc+nod" in line and len({pin, pbc, pnod}) == 3
        ins, outs = [], {"bc": [], "nod": []}
        for _ in range(2):                       # one by one: arrival order = dialogue index
            ins.append(socket.create_connection(("127.0.0.1", pin)))
            time.sleep(0.1)
        for m, port in (("bc", pbc), ("nod", pnod)):
            for _ in range(2):
                outs[m].append(socket.create_connection(("127.0.0.1", port)))
                time.sleep(0.1)
        audio = synth.dialogue_batch([0, 1], hop * 10).astype(np.float64)
        for f in range(10):
            new = audio[:, :, f * hop:(f + 1) * hop]
            for s in range(2):
                ins[s].sendall(wire.encode_input(new[s, 0], new[s, 1]))
            for s in range(2):
                ln, r = _read_packet(outs["bc"][s], "bc", 30)
                assert ln == 8 + 2 * (4 + 8 * hop) + 2 * 12
                np.testing.assert_array_equal(r["x1"], new[s, 0])
                assert 0.0 <= r["p_bc_react"][0] <= 1.0 and 0.0 <= r["p_bc_emo"][0] <= 1.0
                ln, r = _read_packet(outs["nod"][s], "nod", 30)
                assert ln == 8 + 2 * (4 + 8 * hop) + (4 + 8 * (f + 1)) + 3 * 12 and len(r["p_bc"]) == f + 1
                np.testing.assert_array_equal(r["x2"], new[s, 1])
                assert all(0.0 <= v <= 1.0 for v in r["p_bc"] + r["p_nod_short"] + r["p_nod_long"] + r["p_nod_long_p"])
        for s in ins + outs["bc"] + outs["nod"]:
            s.close()
    finally:
        proc.send_signal(signal.SIGTERM)
        try:
            proc.wait(timeout=30)
        except subprocess.TimeoutExpired:
            proc.kill()
    assert proc.returncode == 0
    bad = subprocess.run([sys.executable, "-m", "vap_realtime_amd.serve", "--mode", "bc+nod", "--gpus", "2", "--synthetic-weights", "3"],
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    lines = [l for l in bad.stdout.splitlines() if l.strip()]
    assert bad.returncode != 0 and len(lines) == 1 and "single-model" in lines[0], bad.stdout
