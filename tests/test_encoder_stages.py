"""The stage bound of tests/encoder_stages.py has detection power, shown on the CPU at 50, 20, 10 and 5 Hz with three dialogues at
1e-3 x, 1 x and 30 x the synthetic amplitude (what tests/test_layer_rows.py is for the transformer):

  * the torch fp32 oracle passes every stage against float64 (ratio <= 1 by construction) and its own error stays below 1e-5 of
    each stage's magnitude, so the yardstick is not vacuous;
  * a float64 oracle that carries one fault is rejected at the stage the fault sits in, on every frame, and the failure names
    that stage (and says so when the position is one that never reaches ``z[:, 1:-1]``);
  * the ChannelNorm epsilon faults at conv2 and conv4 move the step's outputs by less than 1e-4 (conv2: 3-6e-5 on every input
    tried; conv4: 7-10e-5, at the bar): the parity tests of the outputs cannot see them, which is why this test exists.

Smallest rejection margin (fault error / bound at FACTOR = 8) per stage over the four rates and FRAMES frames (printed by
``test_faults_are_rejected_at_their_stage``, run with -s):

    h0        593 x  (eps 1e-4 in conv0's ChannelNorm; conv0 dropping the last sample: 1e4 x, at a dead edge position)
    h1        6.8 x  (1e-4 relative in one 32 x 32 sub-tile of conv1's output; biased variance: 200 x and more)
    h2        5.7 x  (eps 1e-4 in conv2's ChannelNorm; the sub-tile fault: 7.3 x)
    h3        228 x  (biased variance in conv3's ChannelNorm)
    z         3.2 x  (the sub-tile fault in conv4's output; eps 1e-4 in conv4: 4.0 x)
    lstm_out  12 x   (1e-4 relative on the gates; a cell unit not persisted and a neighbour's initial h: 4e3 x and more)
    e         2369 x (downsample without the last 8 channels of the last step)

A stage's factor (``encoder_stages.STAGE_FACTOR``) may only be raised while every fault of that stage keeps a 1.5 x margin; the test
asserts it."""
import functools

import numpy as np
import pytest

import encoder_stages as ES

RATES = (50, 20, 10, 5)
AMPS = (1e-3, 1.0, 30.0)
FRAMES = 6
SEED = 23
SPEC = ((5, 3), (4, 2), (2, 1), (2, 1), (2, 1))
REL = 1e-4

# fault -> the stage that must reject it.  State faults show from the second frame on (the first starts from zeros).
FAULTS = {"eps0": "h0", "eps2": "h2", "eps4": "z", "biased_var1": "h1", "biased_var3": "h3",
          "tile1": "h1", "tile2": "h2", "tile4": "z", "conv0_drops_last_sample": "h0",
          "c_unit_not_persisted": "lstm_out", "last_row_h_from_row_before": "lstm_out", "gates_rel": "lstm_out",
          "down_drops_tail": "e"}
FROM_FRAME = {"c_unit_not_persisted": 1, "last_row_h_from_row_before": 1}


def faulty_oracle(fault, *args, **kw):
    import torch
    import torch.nn.functional as F
    from oracle.vap_oracle import DIM, VapOracle

    class Faulty(VapOracle):
        def cnn(self, x, collect=None):
            w = self.w
            if fault == "conv0_drops_last_sample":
                x = x.clone()
                x[..., -1] = 0
            for i, (s, p) in enumerate(SPEC):
                x = F.conv1d(x, w[f"gEncoder.conv{i}.weight"], w[f"gEncoder.conv{i}.bias"], stride=s, padding=p)
                mean = x.mean(dim=1, keepdim=True)
                var = x.var(dim=1, keepdim=True, unbiased=fault != f"biased_var{i}")
                x = (x - mean) * torch.rsqrt(var + (1e-4 if fault == f"eps{i}" else 1e-5))
                x = x * w[f"gEncoder.batchNorm{i}.weight"] + w[f"gEncoder.batchNorm{i}.bias"]
                x = F.relu(x)
                if fault == f"tile{i}":          # one 32-position x 32-channel sub-tile of the last (stream, channel)
                    x = x.clone()
                    lo = 1 if i == 4 else 0      # conv4: a position that survives z[:, 1:-1]
                    x[-1, 32:64, lo:lo + 32] *= 1.0 + REL
                if collect is not None:
                    collect[f"cnn{i}"] = x
            return x

        def lstm(self, z, h, c):
            if fault == "c_unit_not_persisted":
                c = c.clone()
                c[:, 7] = 0
            if fault == "last_row_h_from_row_before":
                h = h.clone()
                h[-1] = h[-2]
            if fault != "gates_rel":
                return super().lstm(z, h, c)
            w = self.w
            wih, whh = w["gAR.baseNet.weight_ih_l0"], w["gAR.baseNet.weight_hh_l0"]
            b = w["gAR.baseNet.bias_ih_l0"] + w["gAR.baseNet.bias_hh_l0"]
            outs = []
            for t in range(z.shape[1]):
                g = (z[:, t] @ wih.T + h @ whh.T + b) * (1.0 + REL)
                i, f, gg, o = g.split(DIM, dim=1)
                c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
                h = torch.sigmoid(o) * torch.tanh(c)
                outs.append(h)
            return torch.stack(outs, dim=1), h, c

        def downsample(self, y):
            if fault == "down_drops_tail":
                y = y.clone()
                y[:, -1, 248:] = 0
            return super().downsample(y)

    return Faulty(*args, **kw)


def scaled_dialogues(hz, frames):
    from vap_realtime_amd import synth
    hop = 16000 // hz
    audio = synth.dialogue_batch([SEED + i for i in range(len(AMPS))], hop * frames)
    return audio * np.asarray(AMPS, np.float32)[:, None, None]


def excess(stage, got, w64, w32):
    """max over the batch rows of err / bound: > 1 is a rejection."""
    r = 0.0
    for b in range(got.shape[0]):
        bound, _, _ = ES.stage_bound(stage, w64[b], w32[b])
        r = max(r, float(np.abs(got[b].astype(np.float64) - w64[b]).max()) / bound)
    return r


@functools.lru_cache(maxsize=None)
def run_rate(hz):
    """Steps the float64 and fp32 oracles and one float64 oracle per fault over FRAMES frames.  Returns
    (accept, faults): accept[stage] = (worst fp32 ratio, worst E32 / max|x|); faults[name] = per frame
    (first stage that rejects, its message, excess at the named stage)."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import weights as W
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cpc, vap = W.synthetic_weights(SEED, hz, "vap")
    hop, S = 16000 // hz, len(AMPS)
    audio = scaled_dialogues(hz, FRAMES)
    o64, o32 = VapOracle(cpc, vap, hz, 1.0, dtype=torch.float64), VapOracle(cpc, vap, hz, 1.0)
    bad = {f: faulty_oracle(f, cpc, vap, hz, 1.0, dtype=torch.float64) for f in FAULTS}
    s64, s32, sbad = o64.new_state(S), o32.new_state(S), {f: o.new_state(S) for f, o in bad.items()}
    fr = ServerFramer(S, hop)
    accept = {st: (0.0, 0.0) for st in ES.STAGES + ("h", "c")}
    faults = {f: [] for f in FAULTS}
    for t in range(FRAMES):
        frame = fr.frame(audio[:, :, t * hop:(t + 1) * hop])
        r64, r32 = ES.collect_stages(o64, frame, s64), ES.collect_stages(o32, frame, s32)
        geo = ES.geometry(hz)
        for st in ES.STAGES + ("h", "c"):
            assert r64[st].shape == (S, 2, geo.get(st, 1), 256), (st, r64[st].shape)
            ratio = ES.check_stage(st, ES.with_guards(st, r32[st]), r64[st], r32[st], what=f"{hz} Hz frame {t} fp32 oracle")
            rel = max(ES.stage_bound(st, r64[st][b], r32[st][b])[1] / ES.stage_bound(st, r64[st][b], r32[st][b])[2] for b in range(S))
            accept[st] = (max(accept[st][0], ratio), max(accept[st][1], rel))
        for f, o in bad.items():
            rb = ES.collect_stages(o, frame, sbad[f])
            first, msg = None, ""
            for st in ES.STAGES:
                try:
                    ES.check_stage(st, ES.with_guards(st, rb[st]), r64[st], r32[st], what=f"{hz} Hz frame {t} {f}")
                except AssertionError as e:
                    first, msg = st, str(e)
                    break
            faults[f].append((first, msg, excess(FAULTS[f], rb[FAULTS[f]], r64[FAULTS[f]], r32[FAULTS[f]])))
    return accept, faults


@pytest.mark.parametrize("hz", RATES)
def test_fp32_oracle_passes_every_stage_and_is_a_usable_yardstick(hz):
    accept, _ = run_rate(hz)
    for st, (ratio, rel) in accept.items():
        assert ratio <= 1.0 + 1e-9, (hz, st, ratio)
        assert rel < 1e-5, f"{hz} Hz {st}: E32 / max|x| = {rel:.2e}: the fp32 oracle is no yardstick for this input"
    print(f"{hz} Hz: E32 / max|x| per stage", {st: f"{rel:.1e}" for st, (_, rel) in accept.items()})


def test_faults_are_rejected_at_their_stage():
    margins = {}
    for hz in RATES:
        _, faults = run_rate(hz)
        for f, stage in FAULTS.items():
            for t, (first, msg, ex) in enumerate(faults[f]):
                if t < FROM_FRAME.get(f, 0):
                    continue
                assert first == stage, f"{hz} Hz frame {t}: fault {f} should be rejected at {stage}, first rejection: {first} {msg}"
                assert f": {stage} (" in msg and "32-column tile" in msg, msg
                margins[(stage, f)] = min(margins.get((stage, f), np.inf), ex)
            if f == "conv0_drops_last_sample":                   # position P0 - 1: dead, and the message says so
                assert "does not reach z[:, 1:-1]" in faults[f][0][1], faults[f][0][1]
            if f.startswith("tile"):
                assert "stream 2" in faults[f][0][1] and "channel 1" in faults[f][0][1] and "32-column tile 1)" in faults[f][0][1], faults[f][0][1]
    for stage in ES.STAGES:
        mine = {f: m for (s, f), m in margins.items() if s == stage}
        if mine:
            f = min(mine, key=mine.get)
            print(f"{stage}: smallest rejection margin {mine[f]:.1f} x bound ({f}); all:", {k: round(v, 1) for k, v in mine.items()})
            # excess() is measured with the stage's factor in force, so a raised factor has to leave MARGIN of every rejection
            assert mine[f] >= (ES.MARGIN if stage in ES.STAGE_FACTOR else 1.0), (stage, f, mine[f])


@pytest.mark.parametrize("stage", ["h0", "h1", "h2", "h3"])
def test_a_nonzero_guard_row_is_rejected(stage):
    """One guard value of the last stream's block set to the smallest subnormal: the values are right, the buffer is not."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import weights as W
    hz = 20
    cpc, vap = W.synthetic_weights(SEED, hz, "vap")
    o64, o32 = VapOracle(cpc, vap, hz, 1.0, dtype=torch.float64), VapOracle(cpc, vap, hz, 1.0)
    frame = ServerFramer(len(AMPS), 800).frame(scaled_dialogues(hz, 1))
    r64, r32 = ES.collect_stages(o64, frame, o64.new_state(3)), ES.collect_stages(o32, frame, o32.new_state(3))
    for row in (0, -1):
        got = ES.with_guards(stage, r32[stage]).copy()
        got[2, 1, row, 100] = np.float32(1e-45)
        with pytest.raises(AssertionError, match=f": {stage} .*guard row") as e:
            ES.check_stage(stage, got, r64[stage], r32[stage], what="guard")
        assert "stream 2" in str(e.value) and "channel 1" in str(e.value)


def test_carry_is_compared_bit_for_bit():
    frame = np.random.default_rng(0).standard_normal((2, 1120)).astype(np.float32)
    ES.check_carry(frame[:, -320:].copy(), frame)
    off = frame[:, -320:].copy()
    off[1, 319] = np.nextafter(off[1, 319], np.float32(2.0))
    with pytest.raises(AssertionError, match="carry channel 1 sample 319"):
        ES.check_carry(off, frame)
    zero = frame.copy()
    zero[0, -1] = 0.0
    neg = zero[:, -320:].copy()
    neg[0, -1] = -0.0
    with pytest.raises(AssertionError, match="carry channel 0 sample 319"):
        ES.check_carry(neg, zero)


@pytest.mark.parametrize("hz,ctx,frames", [(20, 2.5, 70), (50, 1.3, 80)])
def test_eps_faults_pass_the_output_bar(hz, ctx, frames):
    """The recorded reason for the stage tests: a path whose ChannelNorm epsilon is 1e-4 in conv2 or in conv4 moves p_now,
    p_future, vad and logits by less than the 1e-4 the output parity tests allow, on the audio those tests use (the synthetic
    dialogues at their own amplitude).  Both sides are float64, so the figure is the fault's own effect and does not depend on
    the rounding of a CPU's fp32 kernels (which adds about 1e-6).  If this stops holding, the docstrings are out of date.  The same three dialogues at
    1e-3 x, 1 x and 30 x ride along and are printed, not asserted.  Measured: conv2 3e-5 .. 6e-5 everywhere; conv4 7.4e-5 and
    9.9e-5 here, 1.2e-4 at 50 Hz on the quiet and the loud copy: the conv4 fault sits AT the output bar and passes or fails it
    with the audio, the conv2 fault is invisible to it on every input tried."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth, weights as W
    cpc, vap = W.synthetic_weights(SEED, hz, "vap")
    hop, S = 16000 // hz, len(AMPS)
    plain = synth.dialogue_batch([SEED + i for i in range(S)], hop * frames)
    audio = np.concatenate([plain, scaled_dialogues(hz, frames)])
    os_ = {"f64": VapOracle(cpc, vap, hz, ctx, dtype=torch.float64), "eps2": faulty_oracle("eps2", cpc, vap, hz, ctx, dtype=torch.float64),
           "eps4": faulty_oracle("eps4", cpc, vap, hz, ctx, dtype=torch.float64)}
    st = {k: o.new_state(2 * S) for k, o in os_.items()}
    fr = ServerFramer(2 * S, hop)
    moved = {k: np.zeros(2 * S) for k in ("eps2", "eps4")}
    for t in range(frames):
        frame = fr.frame(audio[:, :, t * hop:(t + 1) * hop])
        res = {k: o.step(frame, st[k]) for k, o in os_.items()}
        for k in moved:
            for q in ("p_now", "p_future", "vad", "logits"):
                d = np.abs(res[k][q].astype(np.float64) - res["f64"][q]).reshape(2 * S, -1).max(axis=1)
                moved[k] = np.maximum(moved[k], d)
    for k, v in moved.items():
        print(f"{hz} Hz {k}: outputs moved by {v[:S].max():.2e} at the dialogues' own amplitude; "
              f"at 1e-3 x / 1 x / 30 x: " + " ".join(f"{x:.2e}" for x in v[S:]))
        assert 0 < v[:S].max() < 1e-4, (hz, k, v)
