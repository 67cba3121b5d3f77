"""The row bound of tests/layer_rows.py has detection power: on the CPU, for every window class of
tests/test_layer_rows_gpu.py and every per-layer buffer, it accepts the torch fp32 oracle against the float64
oracle and rejects a float64 oracle whose attention output carries a 1e-3 relative error in one 32-row tile
(an early and a middle tile), naming the layer and the tile.  A looser factor fails here."""
import numpy as np
import pytest

from layer_rows import BUFFERS, LAYER, TILE, check_rows

# (frame rate, context seconds, T): one window per attention dispatch class and edge, as in tests/test_layer_rows_gpu.py
WINDOWS = [(20, 2.5, 50), (50, 1.3, 65), (20, 5.0, 100), (50, 5.0, 250), (50, 5.12, 256), (50, 5.14, 257), (50, 10.24, 512)]
REL = 1e-3


@pytest.fixture(scope="module")
def rings():
    """Per frame rate: the float64 / fp32 oracles and their rings after the longest window of that rate (one dialogue);
    the window of a shorter T is the first T rows (the ring has not slid yet)."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth, weights as W
    out = {}
    for hz in sorted({w[0] for w in WINDOWS}):
        T_max = max(T for h, _, T in WINDOWS if h == hz)
        cpc, vap = W.synthetic_weights(23, hz, "vap")
        hop = 16000 // hz
        audio = synth.dialogue_batch([11], hop * T_max)
        o64 = VapOracle(cpc, vap, hz, T_max / hz, dtype=torch.float64)
        o32 = VapOracle(cpc, vap, hz, T_max / hz)
        s64, s32, fr = o64.new_state(1), o32.new_state(1), ServerFramer(1, hop)
        for f in range(T_max):
            frame = fr.frame(audio[:, :, f * hop:(f + 1) * hop])
            o64.advance(frame, s64)
            o32.advance(frame, s32)
        out[hz] = (o64, o32, s64, s32)
    return out


def _window(state, T):
    st = state.clone()
    st.ring = st.ring[:T]
    return st


def _perturbed_layers(o64, st, pre, tile):
    """o64.layers(st) with the attention output of ``pre`` off by REL (relative) on rows of one 32-row tile."""
    plain = o64._mha

    def mha(p, q_in, kv_in):
        y = plain(p, q_in, kv_in)
        if p == pre:
            y = y.clone()
            y[:, tile * TILE:(tile + 1) * TILE] *= 1.0 + REL
        return y
    o64._mha = mha
    try:
        return o64.layers(st)
    finally:
        del o64._mha


@pytest.mark.parametrize("hz,ctx,T", WINDOWS, ids=[f"T{w[2]}" for w in WINDOWS])
def test_row_bound_accepts_fp32_and_rejects_a_one_tile_error(rings, hz, ctx, T):
    assert int(ctx * hz) == T
    o64, o32, s64, s32 = rings[hz]
    w64, w32 = _window(s64, T), _window(s32, T)
    ref64, ref32 = o64.layers(w64), o32.layers(w32)
    for buf in BUFFERS:
        assert ref64[buf].shape == (1, 2, T, 256)
        ratio = check_rows(buf, ref32[buf].astype(np.float32), [T], ref64[buf], ref32[buf], what=f"T={T} fp32 oracle")
        assert ratio <= 1.0 + 1e-9
    tiles = sorted({0, max(1, (T - 1) // TILE // 2)})          # an early and a middle tile
    for buf in BUFFERS:
        kinds = ("mha",) if buf == "o" else ("mha", "mha_cross")
        for kind in kinds:
            for tile in tiles:
                bad = _perturbed_layers(o64, w64, f"{LAYER[buf]}.{kind}", tile)[buf]
                with pytest.raises(AssertionError) as e:
                    check_rows(buf, bad, [T], ref64[buf], ref32[buf], what=f"T={T}")
                msg = str(e.value)
                assert f"(tile {tile})" in msg and LAYER[buf] in msg, msg
