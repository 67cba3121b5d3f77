"""Ragged against full row tiles of the flat-row blocks (ffn_block_kernel, every mode): batch composition must not change a row.

The fp32 flat-row kernels see a step as M = streams x 2 x T rows cut into 32-row tiles.  A lane of ffn_block_kernel owns one row of the
tile and guards its hand-offs with one bound test, so the two cases that differ in the code are a launch whose last tile is ragged and a
launch of full tiles only.  The same three dialogues are stepped in two engines:

    A:  3 stream slots               M = 6 T   (T = 250: 1500 rows, T = 50: 300 rows; the last tile holds 28 / 12 rows)
    B: 16 slots, 13 filler dialogues M = 32 T  (8000 / 1600 rows: every tile is full)

The three dialogues sit at different batch positions in B (their rows start at other offsets inside a tile than in A) and one of them joins
late, so a step mixes valid lengths and ring rotations.  Both engines are stepped through the filling and the sliding window, one of them
with VAPX_POISON_SCRATCH (a read of a padding row or of an unwritten slot turns a valid row into NaN).  At the checkpoints the three
dialogues' outputs and every valid row of the peeked ``o`` / ``stereo0`` / ``stereo1`` buffers are compared between A and B.

The bound.  A row does not depend on what else is in the batch, so the first expectation was bit-equality.  The kernels BEFORE the
row-per-lane epilogues do not meet it, and the kernels after them differ by exactly the same figures: with 2 against 15 streams in the
batch (frames 1-7) everything is bit-equal; with 3 against 16 (from frame 8 on) the encoder output ``e`` and every row of ``o`` are
still bit-equal, but ``stereo0`` / ``stereo1`` differ by up to 1.26 / 1.33 x E32 at T = 250 (0.91 / 1.01 x at T = 50) and the logits by
2.1e-6.  So some step between ``o`` and ``stereo0`` sums in an order that depends on the batch size; it is not traced further here.  The
comparison is therefore held to the bound of tests/layer_rows.py, per dialogue and buffer: |A - B| <= 8 x max(E32, 1e-6 max|x|) with E32
the torch fp32 oracle's own error against the float64 oracle on that buffer of that window (for the outputs: on that output).  Both
engines' rows are also held against the float64 oracle itself (check_rows).  Where bit-equality ends and the worst |A - B| / E32 per
buffer are printed (run with -s).  T = 250 runs modes 1 and 2 (long-window chain), T = 50 mode 0."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LATE = 7
POS_B = (2, 7, 13)           # batch positions of the three dialogues in engine B
BUFFERS = ("o", "stereo0", "stereo1")
OUTPUTS = ("p_now", "p_future", "vad", "logits")


def _engine(blob, hz, ctx, slots, poison):
    from vap_realtime_amd import engine
    saved = os.environ.pop("VAPX_POISON_SCRATCH", None)
    try:
        if poison:
            os.environ["VAPX_POISON_SCRATCH"] = "1"      # read by vapx_create, once per engine
        return engine.Engine(blob, hz, ctx, max_streams=slots)
    finally:
        os.environ.pop("VAPX_POISON_SCRATCH", None)
        if saved is not None:
            os.environ["VAPX_POISON_SCRATCH"] = saved


def _run(hz, ctx, T, poison_a, seed=31):
    import torch
    from layer_rows import check_rows, row_bound
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import engine, synth, weights as W
    cpc, vap = W.synthetic_weights(seed, hz, "vap")
    blob = W.pack_blob(cpc, vap)
    hop = 16000 // hz
    cps = sorted({1, 2, 31, 33, T - 1, T, T + 1, T + 37})
    F_ = cps[-1]
    cohorts, starts = (2, 1), (0, LATE)                    # dialogues 0, 1 start at frame 0, dialogue 2 at frame LATE
    coh, pos = (0, 0, 1), (0, 1, 0)
    audio = [synth.dialogue_batch([seed + 100 * k + j for j in range(c)], hop * (F_ - starts[k])) for k, c in enumerate(cohorts)]
    fill = synth.dialogue_batch(list(range(seed + 1000, seed + 1013)), hop * F_)
    o64 = VapOracle(cpc, vap, hz, ctx, dtype=torch.float64)
    o32 = VapOracle(cpc, vap, hz, ctx)
    st64 = [o64.new_state(c) for c in cohorts]
    st32 = [o32.new_state(c) for c in cohorts]
    fr = [ServerFramer(c, hop) for c in cohorts]
    ea = _engine(blob, hz, ctx, 3, poison_a)
    eb = _engine(blob, hz, ctx, 16, not poison_a)
    assert ea.T == T and eb.T == T
    worst = {b: 0.0 for b in BUFFERS + OUTPUTS}
    seen_unequal = False
    try:
        for f in range(F_):
            live = [d for d in range(3) if f >= starts[coh[d]]]
            new = {d: audio[coh[d]][pos[d], :, (f - starts[coh[d]]) * hop:(f - starts[coh[d]] + 1) * hop] for d in live}
            # A: the live dialogues, slot = dialogue
            out_a = ea.step(np.stack([new[d] for d in live]), np.asarray(live, dtype=np.int32)).copy()
            # B: dialogue d at batch position POS_B[d] (until the late dialogue joins, the batch is one stream shorter)
            rows, ids, at = [], [], {}
            k = 0
            for p in range(16):
                if p in POS_B:
                    d = POS_B.index(p)
                    if d not in live:
                        continue
                    at[d] = len(rows)
                    rows.append(new[d])
                else:
                    rows.append(fill[k, :, f * hop:(f + 1) * hop])
                    k += 1
                ids.append(p)
            out_b = eb.step(np.stack(rows), np.asarray(ids, dtype=np.int32)).copy()
            if not seen_unequal:                           # (printed once: where bit-equality between the engines ends)
                da, db = engine.split_outputs(out_a), engine.split_outputs(out_b)
                for i, d in enumerate(live):
                    if not np.array_equal(out_a[i], out_b[at[d]]):
                        seen_unequal = True
                        print(f"T={T}: first unequal outputs at frame {f + 1} (batch {len(live)} vs {len(ids)}), dialogue {d}:",
                              {key: float(np.abs(da[key][i] - db[key][at[d]]).max()) for key in OUTPUTS + ("e",)})
            check = f + 1 in cps
            ref64, ref32 = {}, {}
            for k in range(len(cohorts)):
                if f < starts[k]:
                    continue
                frame = fr[k].frame(audio[k][:, :, (f - starts[k]) * hop:(f - starts[k] + 1) * hop])
                if check:                                  # one transformer pass gives the outputs and (collect) every layer's rows
                    for o, st, ref in ((o64, st64[k], ref64), (o32, st32[k], ref32)):
                        col = {}
                        ref[k] = dict(o.step(frame, st, col))
                        ref[k].update({b: col[b].numpy() for b in BUFFERS})
                else:
                    o64.advance(frame, st64[k])
                    o32.advance(frame, st32[k])
            if not check:
                continue
            what = f"T={T} frame {f + 1}"
            ga, gb = engine.split_outputs(out_a), engine.split_outputs(out_b)
            for i, d in enumerate(live):
                for key in OUTPUTS:
                    w64 = np.asarray(ref64[coh[d]][key][pos[d]], dtype=np.float64)
                    bound, e32 = row_bound(w64, np.asarray(ref32[coh[d]][key][pos[d]]))
                    diff = float(np.abs(ga[key][i].astype(np.float64) - gb[key][at[d]]).max())
                    worst[key] = max(worst[key], diff / max(e32, 1e-30))
                    assert np.isfinite(ga[key][i]).all() and np.isfinite(gb[key][at[d]]).all(), f"{what} dialogue {d}: non-finite {key}"
                    assert diff <= bound, f"{what} dialogue {d}: {key} differs between the 3-slot and the 16-slot engine by {diff:.3e} > {bound:.3e}"
            ns = [min(f + 1 - starts[coh[d]], T) for d in live]
            for b in BUFFERS:
                xa = ea.peek(b, (len(live), 2, T, 256))
                xb = eb.peek(b, (len(ids), 2, T, 256))[[at[d] for d in live]]
                w64 = [ref64[coh[d]][b][pos[d]] for d in live]
                w32 = [ref32[coh[d]][b][pos[d]] for d in live]
                check_rows(b, xa, ns, w64, w32, streams=live, what=what + " engine A (3 slots)")
                check_rows(b, xb, ns, w64, w32, streams=live, what=what + " engine B (16 slots)")
                for i, d in enumerate(live):
                    bound, e32 = row_bound(np.asarray(w64[i], dtype=np.float64), w32[i])
                    err = np.abs(xa[i, :, :ns[i]].astype(np.float64) - xb[i, :, :ns[i]]).max(axis=2)     # [2, n]
                    worst[b] = max(worst[b], float(err.max()) / max(e32, 1e-30))
                    if (err > bound).any():
                        c, t = np.argwhere(err > bound)[0]
                        raise AssertionError(f"{what} dialogue {d} {b}: channel {c} row {t} (flat row {(i * 2 + c) * T + t} of {len(live) * 2 * T} in A, "
                                             f"{(at[d] * 2 + c) * T + t} of {len(ids) * 2 * T} in B) differs by {err[c, t]:.3e} > bound {bound:.3e}")
    finally:
        ea.close()
        eb.close()
    print(f"T={T}: worst |A - B| / E32", {k: round(v, 3) for k, v in worst.items()})


def test_ragged_and_full_tiles_agree_long_window():
    """T = 250 at 50 Hz (the C3 shape): ffn_block_kernel<1, 1> and <1, 2>; the 3-slot engine runs poisoned."""
    _run(50, 5.0, 250, poison_a=True)


def test_ragged_and_full_tiles_agree_short_window():
    """T = 50 at 20 Hz: ffn_block_kernel<1, 0>; the 16-slot engine runs poisoned."""
    _run(20, 2.5, 50, poison_a=False)
