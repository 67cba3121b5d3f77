"""The window sweep of tests/window_sweep.py has coverage and detection power, proved on the CPU.

Coverage: ``plan`` asserts, for every T of tests/test_window_sweep_gpu.py, that every valid-tile count, every multiple of 32 with its
neighbours, rot = T - 1 and a rotation that is a multiple of 32 occur, and that no two streams share a state.

Detection: the whole harness (tick program, anchored export, truth from the exported window, check) runs on a stand-in engine backed by
an oracle.  Backed by the fp32 oracle it is accepted at err / E32 <= 1 for a short, a long and an XL window.  Backed by the float64
oracle with one seeded fault it is rejected, and the message names the stream's n, the tile and the layer:

    1. the attention output of one layer off by 1e-3 (relative) on one 32-row tile, only in streams with 3, 5 or 7 valid tiles
       (long window) or 10 or 13 (XL): the counts the stepping tests never see
    2. one stream's window rotated by one row
    3. the newest row's attention skipping its own key, in the streams with n % 32 == 1
"""
import math
import re

import numpy as np
import pytest

import window_sweep as ws
from layer_rows import LAYER, TILE

HZ = 50
SHORT_T, LONG_T, XL_T = 37, 193, 385
GPU_TS = ws.SHORT + ws.LONG + ws.XL
FAULT_TILES = {3, 5, 7, 10, 13}
REL = 1e-3
ALL = ("o", "stereo0", "stereo1", "stereo2")


@pytest.mark.parametrize("T", GPU_TS)
def test_plan_covers_every_tile_count_edge_and_rotation(T):
    states = ws.plan(T)
    ws.check_plan(states, T)
    prog = ws.schedule(states, T)
    assert prog.ticks == max(T - 1, 1) and all(len(b) for b in prog.batches) and len(prog.batches[-1]) == len(states) and prog.max_streams > len(states)
    assert (prog.slot != np.arange(len(states))).any() and len(set(prog.slot.tolist())) == len(states)
    for (n, r), rows, steps in zip(states, prog.rows, prog.steps):
        assert min(rows + steps, T) == n and (steps == max(r, 1)) and rows <= T
        assert (rows + steps) - T == r if n == T else r == 0          # frames seen beyond T = the ring rotation
    if T <= 64:
        assert {n for n, _ in states} == set(range(1, T + 1)) and {r for n, r in states if n == T} == set(range(T))


def test_check_plan_refuses_a_thinned_edge():
    for drop in ((64, 0), (250, 249), (1, 0), (225, 0)):
        states = [s for s in ws.plan(250) if s != drop]
        with pytest.raises(AssertionError):
            ws.check_plan(states, 250)


class StandIn:
    """The ``Engine`` methods the harness uses, on an oracle: fp32 rings per slot, the oracle's encoder in ``step``, and ``layers`` of the
    final batch's windows behind ``peek``.  ``layers`` / ``roll`` seed the faults."""

    def __init__(self, orc, T, max_streams, layers=None, roll=None):
        self.o, self.T, self.max_streams, self.layers, self.roll = orc, T, max_streams, layers, roll or {}
        self.ring = [[] for _ in range(max_streams)]
        self.h = np.zeros((max_streams, 2, 2, 256))
        self.carry = np.zeros((max_streams, 2, 320), np.float32)
        self.ids, self.e, self.ref = None, None, None

    def reset_stream(self, sid):
        self.ring[sid], self.h[sid], self.carry[sid] = [], 0.0, 0.0

    def set_state(self, sid, state):
        assert state.get("lstm") is None and state.get("carry") is None
        ring = np.asarray(state["ring"], np.float32)
        self.ring[sid] = [ring[:, t].copy() for t in range(int(state["n_frames"]))]

    def step(self, audio, ids):
        import torch
        from oracle.vap_oracle import OracleState
        ids = np.asarray(ids)
        frame = np.concatenate([self.carry[ids], np.asarray(audio, np.float32)], axis=2)
        self.carry[ids] = frame[:, :, -320:]
        st = OracleState(len(ids), self.T, [], torch.from_numpy(self.h[ids, 0]).to(self.o.dtype), torch.from_numpy(self.h[ids, 1]).to(self.o.dtype))
        with torch.no_grad():
            e = self.o.encode(torch.from_numpy(frame).to(self.o.dtype), st).numpy().astype(np.float32)
        self.h[ids, 0], self.h[ids, 1] = st.h.numpy(), st.c.numpy()
        for b, sid in enumerate(ids):
            self.ring[sid] = (self.ring[sid] + [e[b]])[-self.T:]
        self.ids, self.e, self.ref = ids, e, None

    def _windows(self, ids):
        return [np.stack(self.ring[sid], axis=1) for sid in ids]

    def peek(self, name, shape):
        if name == "e":
            return self.e.copy()
        if self.ref is None:
            wins = [np.roll(w, self.roll.get(int(sid), 0), axis=1) for sid, w in zip(self.ids, self._windows(self.ids))]
            self.ref = ws.layers_by_n(self.o, wins, self.layers)
        if name == "last":
            return np.stack([r["stereo2"][:, -1] for r in self.ref]).astype(np.float32)
        out = np.full(shape, np.nan, np.float32)              # rows t >= n are undefined: the check must not look at them
        for b, r in enumerate(self.ref):
            out[b, :, :r[name].shape[1]] = r[name]
        return out

    def export_streams(self, ids, cache=False):
        from vap_realtime_amd import engine as E
        assert not cache
        rec = np.zeros((len(ids), E.state_record_floats(self.T)), np.float32)
        d = E.split_state(rec, self.T)
        for b, w in enumerate(self._windows(ids)):
            d["n_frames"][b] = w.shape[1]
            d["ring"][b, :, :w.shape[1]] = w
        return rec


class Bench:
    """One T: weights, oracles, program, donor rows, the run of the fp32 stand-in and the truth of its windows.  Every seeded fault
    re-uses that capture: a fault changes ``layers`` of some streams only, never the windows."""

    def __init__(self, T, don, cpc, vap):
        import torch
        from oracle.vap_oracle import VapOracle
        self.T = T
        ctx = (T + 0.5) / HZ
        self.o64, self.o32 = VapOracle(cpc, vap, HZ, ctx, dtype=torch.float64), VapOracle(cpc, vap, HZ, ctx)
        assert self.o64.T == T
        self.prog = ws.schedule(ws.plan(T), T)
        self.inject = ws.injected_rows(self.prog, T, don)
        self.cap = ws.drive(StandIn(self.o32, T, self.prog.max_streams), T, self.prog, self.inject, ws.step_audio(self.prog, HZ),
                            HZ, ALL, True, what="fp32 oracle")
        self.truth = ws.truth(self.o64, self.o32, self.cap)

    def faulty(self, rows, layers=None, roll=None):
        """(capture, truth) of batch rows ``rows`` as a float64 stand-in with a seeded fault shows them: the windows of the fp32 run,
        peeked through the fault."""
        eng = StandIn(self.o64, self.T, self.prog.max_streams, layers, roll)
        order = self.cap.order[rows]
        for b, i in zip(rows, order):
            eng.ring[self.prog.slot[i]] = [self.cap.windows[b][:, t] for t in range(self.cap.ns[b])]
        eng.ids, eng.e = self.prog.slot[order], self.cap.peeks["e"][rows]
        peeks = {b: eng.peek(b, (len(order), 2, self.T, 256)) for b in ALL}
        peeks["e"], peeks["last"] = eng.e, eng.peek("last", None)
        cap = ws.Capture(self.prog, order, [self.cap.ns[b] for b in rows], [self.cap.windows[b] for b in rows], peeks)
        return cap, ws.Truth([self.truth.ref64[b] for b in rows], [self.truth.ref32[b] for b in rows])

    def rows_where(self, pred):
        return [b for b, n in enumerate(self.cap.ns) if pred(n)]


@pytest.fixture(scope="module")
def benches():
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(23, HZ, "vap")
    don = ws.donor(cpc, vap, HZ, XL_T + ws.DONOR_EXTRA)
    made = {}

    def get(T):
        if T not in made:
            made[T] = Bench(T, don, cpc, vap)
        return made[T]
    return get


@pytest.mark.parametrize("T", [SHORT_T, LONG_T, XL_T])
def test_sweep_accepts_the_fp32_oracle(benches, T):
    bn = benches(T)
    worst = ws.check(bn.cap, bn.truth, ALL, T, what="fp32 oracle")
    assert set(worst) == set(ALL) | {"last"} and max(worst.values()) <= 1.0 + 1e-9, worst
    rows = bn.rows_where(lambda n: n in (1, T - 1, T))        # and the float64 oracle itself, rounded to the fp32 that ``peek`` returns
    worst = ws.check(*bn.faulty(rows), ALL, T, what="float64 oracle")
    assert max(worst.values()) < 1.0, worst


def _mha(o64, pre, q_in, kv_in, skip_own):
    """``VapOracle._mha`` with the newest query row blind to its own key (n = 1: nothing is left to attend to, the output row is 0)."""
    import torch
    v = o64.v
    B, n, _ = q_in.shape
    q = (q_in @ v[f"{pre}.query.weight"].T).view(B, n, 4, 64).transpose(1, 2)
    k = (kv_in @ v[f"{pre}.key.weight"].T).view(B, n, 4, 64).transpose(1, 2)
    val = (kv_in @ v[f"{pre}.value.weight"].T).view(B, n, 4, 64).transpose(1, 2)
    att = torch.einsum("bhid,bhjd->bhij", q, k) * (1.0 / math.sqrt(256))
    mask = torch.full((n, n), float("-inf")).triu(1)
    if skip_own:
        mask[n - 1, n - 1] = float("-inf")
    att = (att + (v[f"{pre}.m"].view(1, 4, 1, 1) * torch.arange(n, dtype=o64.dtype).view(1, 1, 1, n) + mask)).softmax(dim=-1)
    return torch.nan_to_num((att @ val).transpose(1, 2).reshape(B, n, 256), nan=0.0) @ v[f"{pre}.proj.weight"].T


def _faulty_layers(o64, pre, kind):
    """``layers(state)`` of the float64 oracle with a fault in the attention ``pre``: "tile" (REL on the rows of tile count // 2 where
    the valid-tile count is in FAULT_TILES) or "own_key" (streams with n % 32 == 1)."""
    def layers(st):
        n = len(st.ring)
        plain = o64._mha

        def mha(p, q_in, kv_in):
            if p != pre:
                return plain(p, q_in, kv_in)
            if kind == "own_key":
                return _mha(o64, p, q_in, kv_in, n % TILE == 1)
            y = plain(p, q_in, kv_in)
            if ws.tiles(n) in FAULT_TILES:
                t = ws.tiles(n) // 2
                y = y.clone()
                y[:, t * TILE:(t + 1) * TILE] *= 1.0 + REL
            return y
        o64._mha = mha
        try:
            return o64.layers(st)
        finally:
            del o64._mha
    return layers


def _named(msg):
    m = re.search(r"\(tile (\d+)\) of (\w+) \(([\w.]+)\).*n = (\d+)$", msg)
    assert m, msg
    return int(m.group(1)), m.group(2), m.group(3), int(m.group(4))


def test_own_key_reference_is_the_oracle_when_not_skipping(benches):
    import torch
    o64 = benches(SHORT_T).o64
    x = torch.randn(2, 33, 256, dtype=torch.float64)
    assert torch.equal(_mha(o64, "ar.layers.1.mha_cross", x, x.flip(0), False), o64._mha("ar.layers.1.mha_cross", x, x.flip(0)))


@pytest.mark.parametrize("T", [LONG_T, XL_T])
@pytest.mark.parametrize("buf,kind", [("o", "mha"), ("stereo0", "mha"), ("stereo0", "mha_cross"), ("stereo1", "mha_cross"), ("stereo2", "mha")])
def test_sweep_rejects_a_one_tile_error_at_an_unseen_tile_count(benches, T, buf, kind):
    bn = benches(T)
    assert {ws.tiles(n) for n in bn.cap.ns} >= ({3, 5, 7} if T == LONG_T else {10, 13})
    rows = bn.rows_where(lambda n: ws.tiles(n) in FAULT_TILES)
    cap, tr = bn.faulty(rows, layers=_faulty_layers(bn.o64, f"{LAYER[buf]}.{kind}", "tile"))
    with pytest.raises(AssertionError) as e:
        ws.check(cap, tr, ALL, T)
    tile, b, layer, n = _named(str(e.value))
    assert (b, layer) == (buf, LAYER[buf]) and ws.tiles(n) in FAULT_TILES and tile == ws.tiles(n) // 2, str(e.value)
    for k in range(len(rows)):                                # every stream with such a count is caught, not only the first
        one = cap._replace(order=cap.order[k:k + 1], ns=cap.ns[k:k + 1], windows=cap.windows[k:k + 1], peeks={buf: cap.peeks[buf][k:k + 1]})
        with pytest.raises(AssertionError, match=rf"\(tile {ws.tiles(cap.ns[k]) // 2}\) of {buf} "):
            ws.check(one, ws.Truth(tr.ref64[k:k + 1], tr.ref32[k:k + 1]), (buf,), T)


@pytest.mark.parametrize("T", [SHORT_T, LONG_T, XL_T])
def test_sweep_rejects_a_window_rotated_by_one_row(benches, T):
    bn = benches(T)
    for state in ((T, T - 1), (T, 0), (T, 32), (T - 1, 0), (2, 0)):
        i = bn.prog.states.index(state)
        row = int(np.flatnonzero(bn.cap.order == i)[0])
        cap, tr = bn.faulty([row - 1, row] if row else [row], roll={int(bn.prog.slot[i]): 1})
        with pytest.raises(AssertionError) as e:
            ws.check(cap, tr, ALL, T)
        tile, b, layer, n = _named(str(e.value))
        assert n == state[0] and b == "o" and layer == LAYER["o"] and f"stream {i} " in str(e.value), str(e.value)


@pytest.mark.parametrize("T", [SHORT_T, LONG_T])
@pytest.mark.parametrize("buf,kind", [("o", "mha"), ("stereo0", "mha_cross"), ("stereo1", "mha"), ("stereo2", "mha")])
def test_sweep_rejects_a_newest_row_blind_to_its_own_key(benches, T, buf, kind):
    bn = benches(T)
    rows = bn.rows_where(lambda n: n % TILE in (0, 1))        # the streams with the fault and their neighbours without
    cap, tr = bn.faulty(rows, layers=_faulty_layers(bn.o64, f"{LAYER[buf]}.{kind}", "own_key"))
    with pytest.raises(AssertionError) as e:
        ws.check(cap, tr, ALL, T)
    tile, b, layer, n = _named(str(e.value))
    assert (b, layer) == (buf, LAYER[buf]) and n % TILE == 1 and tile == (n - 1) // TILE, str(e.value)
    if buf == "stereo2":                                      # the pruned engines show the last layer through ``last`` alone
        pruned = cap._replace(peeks={k: v for k, v in cap.peeks.items() if k != "stereo2"})
        with pytest.raises(AssertionError) as e:
            ws.check(pruned, tr, ALL[:3], T)
        m = re.search(r"n = (\d+), rot = \d+, \d+ tiles\): last \(last_block_kernel\)", str(e.value))
        assert m and int(m.group(1)) % TILE == 1, str(e.value)
