"""A trunk follower under VAPX_POISON_SCRATCH.  vapx_attach_trunk releases the follower's encoder scratch (h0 .. h3, z, gx, lstm_out),
three of which the poison refill would otherwise touch before every step: the refill must leave released buffers alone and still
cover everything the follower's own chain reads.  Each group is built twice, with and without the variable set at create, and fed
the same audio: every output finite, and each model's output bit-equal between the two (poison only refills buffers whose every
consumed element is rewritten within the tick, so it cannot change a result)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STREAMS, TICKS = 3, 25          # windows of 1.0 s fill and slide; the 10 Hz follower answers on every second tick

GROUPS = {
    "bc+nod_20Hz": ({"bc": 20, "nod": 20}, {"bc": 1.0, "nod": 1.0}),           # T = 20 each, R = 1
    "vap20+nod10": ({"vap": 20, "nod": 10}, {"vap": 1.0, "nod": 1.0}),         # nod: T = 10, R = 2
}


def _build(hz, ctx, poisoned):
    from vap_realtime_amd import engine as E, weights as W
    lead_hz = max(hz.values())
    cpc = W.synthetic_weights(61, lead_hz, "vap")[0]
    blobs = {m: W.pack_blob(cpc, W.synthetic_weights(62 + i, hz[m], m)[1], m) for i, m in enumerate(hz)}
    saved = os.environ.pop("VAPX_POISON_SCRATCH", None)      # read by vapx_create, once per engine
    try:
        if poisoned:
            os.environ["VAPX_POISON_SCRATCH"] = "1"
        return E.TrunkGroup(blobs, hz, ctx, max_streams=STREAMS)
    finally:
        os.environ.pop("VAPX_POISON_SCRATCH", None)
        if saved is not None:
            os.environ["VAPX_POISON_SCRATCH"] = saved


@pytest.mark.parametrize("name", list(GROUPS))
def test_follower_with_released_encoder_scratch_under_poison(name):
    from vap_realtime_amd import synth
    hz, ctx = GROUPS[name]
    plain, poisoned = _build(hz, ctx, False), _build(hz, ctx, True)
    assert plain.order == poisoned.order and len(plain.order) == 2
    slow = [m for m in hz if plain.R[m] > 1]
    assert slow == (["nod"] if name == "vap20+nod10" else [])
    hop = plain.hop
    audio = synth.dialogue_batch([70, 71, 72], hop * TICKS)
    for t in range(TICKS):
        new = audio[:, :, t * hop:(t + 1) * hop]
        a, b = plain.step(new), poisoned.step(new)
        for m in hz:
            assert np.isfinite(a[m]).all() and np.isfinite(b[m]).all(), f"{name} tick {t} {m}: non-finite outputs"
            assert np.array_equal(a[m], b[m]), f"{name} tick {t} {m}: poisoned and plain group differ"
            if m in slow:
                assert plain.due(m, b[m]).all() if t % 2 else not plain.due(m, b[m]).any(), f"{name} tick {t}"
    plain.close()
    poisoned.close()
