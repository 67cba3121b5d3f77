"""The native front-end over a trunk group (vapx_ingest_open_group_fn): one input port, one output port per model, one step call per
tick that fills a model-major wire block (the layout of vapx_step_group).  Host logic only — a Python step function plants
recognisable rows (slot, frame counter, model index) so a routing, framing or layout error shows up in the numbers."""
import socket
import struct
import time

import numpy as np
import pytest

from vap_realtime_amd import engine, ingest, wire

MODES = ("vap", "bc", "nod")
HOP, HZ, T, S = 800, 20, 50, 3
A = engine.OUT_AUX


class GroupModel:
    """Rows of stream slot s at its frame f (counted per stream), model index mi, n = min(f + 1, T) window rows:
    vap  p_now = [s, f]  p_future = [mi, n]  vad = [s + .5, f + .5]
    bc   p_bc_react = 100 s + f   p_bc_emo = 1000 mi + f
    nod  p_bc[r] = 1000 s + f + r / 64 (r < n)   short = s   long = f   long_p = mi"""

    def __init__(self, poison=()):
        self.calls, self.shapes, self.resets = [], [], []
        self.frames = {}
        self.poison = set(poison)            # (slot, frame, mode): that row carries status 1

    def planted(self, s, f, mode):
        mi, n = MODES.index(mode), min(f + 1, T)
        if mode == "vap":
            return {"p_now": [s, f], "p_future": [mi, n], "vad": [s + 0.5, f + 0.5]}
        if mode == "bc":
            return {"p_bc_react": [100 * s + f], "p_bc_emo": [1000 * mi + f]}
        return {"p_bc": [1000 * s + f + r / 64 for r in range(n)], "p_nod_short": [s], "p_nod_long": [f], "p_nod_long_p": [mi]}

    def step(self, ids, audio, wire_rows):
        self.calls.append(ids.tolist())
        self.shapes.append({m: wire_rows[m].shape for m in wire_rows})
        for k, s in enumerate(int(i) for i in ids):
            f = self.frames.get(s, 0)
            self.frames[s] = f + 1
            for m in wire_rows:
                row, p = wire_rows[m][k], self.planted(s, f, m)
                row[engine.OUT_NVALID] = min(f + 1, T)
                if m == "vap":
                    row[0:2], row[2:4], row[4:6] = p["p_now"], p["p_future"], p["vad"]
                elif m == "bc":
                    row[A + 1], row[A + 2] = p["p_bc_react"][0], p["p_bc_emo"][0]
                else:
                    row[engine.OUT_LOGITS:engine.OUT_LOGITS + len(p["p_bc"])] = p["p_bc"]
                    row[A + 1], row[A + 2], row[A + 3] = s, f, MODES.index(m)
                if (s, f, m) in self.poison:
                    row[engine.OUT_STATUS] = 1.0
        return 0

    def reset(self, sid):
        self.resets.append(sid)


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


def _open(model, n_in, listeners=True, **kw):
    """Server + n_in dialogues (slots 0..n_in-1 in connection order) + one listener per dialogue on every port."""
    kw.setdefault("max_wait_s", 0.5)
    srv = ingest.NativeServer.over_group_function(model.step, MODES, S, HZ, T, reset=model.reset, **kw)
    ins, outs = [], {m: [] for m in MODES}
    for k in range(n_in):
        ins.append(socket.create_connection(("127.0.0.1", srv.port_in)))
        _wait(lambda: srv.stats()["in_connections"] == k + 1)
    total = 0
    for m in MODES if listeners else ():
        for k in range(n_in):                           # the k-th connection on a port hears the k-th dialogue
            outs[m].append(socket.create_connection(("127.0.0.1", srv.ports_out[m])))
            total += 1
            _wait(lambda: srv.stats()["out_connections"] == total)
    return srv, ins, outs


def _close(srv, ins, outs):
    srv.close()
    for s in ins + [c for l in outs.values() for c in l]:
        s.close()


def _check_packet(sock, mode, model, s, f, x):
    ln, r = _read(sock, mode)
    want = dict(model.planted(s, f, mode), t=r["t"], x1=x[0], x2=x[1])
    assert ln == len(wire.encode_result(want, mode))
    np.testing.assert_array_equal(r["x1"], x[0])        # float64 echo, bit-exact
    np.testing.assert_array_equal(r["x2"], x[1])
    for k, v in model.planted(s, f, mode).items():
        np.testing.assert_array_equal(r[k], np.asarray(v, np.float32).astype(np.float64), err_msg=f"{mode} slot {s} frame {f} {k}")
    return ln


def test_wire_floats():
    assert engine.wire_floats("vap", 50) == 16
    assert engine.wire_floats("bc", 200) == 16
    assert engine.wire_floats("nod", 50) == 68
    assert engine.wire_floats("nod", 250) == 268


def test_every_port_hears_only_its_model_for_its_stream_in_frame_order():
    m = GroupModel()
    srv, ins, outs = _open(m, 3)
    try:
        assert len(set(srv.ports_out.values())) == 3 and srv.port_out == srv.ports_out["vap"]
        x = np.random.default_rng(11).standard_normal((3, 4, 2, HOP))
        for f in range(4):
            for s in range(3):
                ins[s].sendall(wire.encode_input(x[s, f, 0], x[s, f, 1]))
            for mode in MODES:
                for s in range(3):
                    ln = _check_packet(outs[mode][s], mode, m, s, f, x[s, f])
                    if mode == "vap":
                        assert ln == 12876
        assert len(m.calls) == 4 and all(sorted(c) == [0, 1, 2] for c in m.calls)
        st = srv.stats()
        assert st["frames_done"] == 12 and st["ticks"] == 4 and st["numeric_resets"] == 0       # stream-frames, not packets
        assert st["answered"] == 12                                                            # one latency sample per stream-frame
        assert st["out_connections"] == 9
        assert st["tx_bytes"] == 3 * sum(4 + len(wire.encode_result(dict(m.planted(0, f, md), t=0.0, x1=x[0, 0, 0], x2=x[0, 0, 1]), md))
                                         for md in MODES for f in range(4))                    # summed over the ports
    finally:
        _close(srv, ins, outs)


def test_nod_packet_carries_exactly_n_rows_while_the_window_fills_and_after():
    m = GroupModel()
    srv, ins, outs = _open(m, 1)
    try:
        z = np.zeros(HOP)
        data = wire.encode_input(z, z)
        for f in range(53):
            ins[0].sendall(data)
            _, r = _read(outs["nod"][0], "nod")
            assert len(r["p_bc"]) == min(f + 1, T)
            np.testing.assert_array_equal(r["p_bc"], np.asarray(m.planted(0, f, "nod")["p_bc"], np.float32).astype(np.float64))
            assert r["p_nod_long"] == [float(f)]
    finally:
        _close(srv, ins, outs)


def test_a_stream_poisoned_in_one_model_is_reset_once_and_silent_on_every_port_that_tick():
    m = GroupModel(poison={(1, 0, "bc")})
    srv, ins, outs = _open(m, 3, reset_on_connect=False)
    try:
        x = np.random.default_rng(3).standard_normal((3, 2, 2, HOP))
        for f in range(2):
            for s in range(3):
                ins[s].sendall(wire.encode_input(x[s, f, 0], x[s, f, 1]))
            for mode in MODES:
                for s in (0, 2):                        # the healthy streams are served on all ports, both ticks
                    _check_packet(outs[mode][s], mode, m, s, f, x[s, f])
        for mode in MODES:
            _check_packet(outs[mode][1], mode, m, 1, 1, x[1, 1])   # stream 1: the FIRST packet on every port is frame 1
        assert m.resets.count(1) == 1                   # (connections queued carry-only resets: -1, -2, -3)
        assert sorted(r for r in m.resets if r < 0) == [-3, -2, -1]
        assert srv.stats()["numeric_resets"] == 1
    finally:
        _close(srv, ins, outs)


def test_ragged_tick_steps_only_the_ready_streams_and_lays_the_block_out_for_that_n():
    m = GroupModel()
    srv, ins, outs = _open(m, 3, max_wait_s=0.05)
    try:
        z = np.zeros(HOP)
        data = wire.encode_input(z, z)
        ins[0].sendall(data)
        ins[2].sendall(data)
        ins[1].sendall(data[:len(data) // 2])           # stream 1 lags: half a frame
        for mode in MODES:                              # the block of this tick has n = 2: model m's rows start at 2 x (floats before m)
            _check_packet(outs[mode][0], mode, m, 0, 0, (z, z))
            _check_packet(outs[mode][2], mode, m, 2, 0, (z, z))
        assert sorted(m.calls[0]) == [0, 2]
        assert m.shapes[0] == {"vap": (2, 16), "bc": (2, 16), "nod": (2, 68)}
        ins[1].sendall(data[len(data) // 2:])
        for mode in MODES:
            _check_packet(outs[mode][1], mode, m, 1, 0, (z, z))
        assert m.calls[1] == [1] and m.shapes[1]["nod"] == (1, 68)
    finally:
        _close(srv, ins, outs)


def test_a_listener_dropped_on_one_port_leaves_the_other_ports_serving_that_stream():
    m = GroupModel()
    srv, ins, outs = _open(m, 2)
    try:
        z = np.zeros(HOP)
        data = wire.encode_input(z, z)
        gone = outs["bc"][0]                            # stream 0's bc listener resets its connection
        gone.setsockopt(socket.SOL_SOCKET, socket.SO_LINGER, struct.pack("ii", 1, 0))
        gone.close()
        for f in range(3):
            for s in range(2):
                ins[s].sendall(data)
            for mode in MODES:
                for s in range(2):
                    if (mode, s) != ("bc", 0):
                        _check_packet(outs[mode][s], mode, m, s, f, (z, z))
        st = srv.stats()
        assert st["dropped_listeners"] == 1 and st["out_connections"] == 5
        late = socket.create_connection(("127.0.0.1", srv.ports_out["bc"]))     # fewest listeners OF THAT PORT: stream 0 again
        outs["bc"].append(late)
        _wait(lambda: srv.stats()["out_connections"] == 6)
        ins[0].sendall(data)
        _check_packet(late, "bc", m, 0, 3, (z, z))
    finally:
        _close(srv, ins, outs)


def test_group_configuration_errors_are_refused_with_a_message():
    m = GroupModel()
    with pytest.raises(engine.VapxError, match="passive"):
        ingest.NativeServer.over_group_function(m.step, MODES, S, HZ, T, port_in=-1, ports_out=[-1, 0, 0])
    with pytest.raises(engine.VapxError, match="passive"):
        ingest.NativeServer.over_group_function(m.step, MODES, S, HZ, T, port_in=-1)
    with pytest.raises(engine.VapxError, match="distinct"):
        ingest.NativeServer.over_group_function(m.step, ("bc", "nod", "bc"), S, HZ, T)
