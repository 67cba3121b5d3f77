"""The stage bound of tests/head_stages.py has detection power, shown on the CPU at 20 Hz (vap, bc, nod) and 50 Hz (vap, nod) with three
dialogues at 1e-3 x, 1 x and 30 x the synthetic amplitude and windows of 10 / 12 frames that fill and then slide (what
tests/test_encoder_stages.py is for the encoder):

  * the torch fp32 oracle passes every stage against float64 (<= 1 / FACTOR of the bound by construction), and the restatement of the
    tail that carries the faults equals the oracle when it carries none;
  * a float64 oracle that carries one fault is rejected at the stage the fault sits in, on every tick on which the fault can act, and
    the failure names that stage and its device code;
  * ``test_faults_against_the_output_bar`` prints how far each fault moves the step's outputs and asserts the list of faults that stay
    under the 1e-4 of the output parity tests on every output: the reason tests/test_head_stages_gpu.py exists.

Faults (``FAULTS``: fault -> stage per mode), chosen from the ways last_block_kernel, attention_last_kernel, head_kernel and
pbc_rows_kernel can go wrong: the last layer's single-query self-attention drops the oldest key / the newest odd key (the tail of one
key parity); its n = 1 window counts a padded key in the softmax denominator; its cross-attention reads its own channel; head 1 takes
head 0's ALiBi slope; its scores scaled by 1 / sqrt(64) instead of 1 / sqrt(256); one wave's 32 output columns of the newest row scaled
by 1 + 1e-4 and by 1 + 3e-5; the combinator's LayerNorm with the unbiased variance, and one 32-column slice of its output scaled by
1 + 1e-4 (stage ``comb`` for nod, ``logits`` elsewhere: only nod materialises the combinator); one 32-column slice of vap_head scaled
by 1 + 1e-4; VAD from the stereo tower / from the row before; now / future bin weights swapped
for channel 1; future from bin 3 alone; the second VAD sigmoid a copy of the first; the aux softmax over 4 rows in bc mode and over 3
in nod mode; p_bc of the newest row taken from row n - 2.  Two more ride along without being required (``UNSEEN``): tanh-GELU in the
last-row FFN sits AT the bound, and a combinator LayerNorm epsilon of 1e-4 moves nothing on these weights.

Smallest rejection margin (fault error / bound at FACTOR = 8) per stage over the five cases (printed by
``test_faults_are_rejected_at_their_stage``, run with -s; ``test_faults_against_the_output_bar`` prints what each fault does to the outputs):

    last        2.4 x   (3e-5 relative in 32 columns; 1e-4: 8.1 x; wrong score scale 12.6 x; neighbour's slope 13.3 x; a dropped key 49 x)
    comb        5.9 x   (1e-4 relative in one slice of the combinator's LayerNorm; unbiased variance: 195 x)
    logits      3.3 x   (the same slice fault seen through vap_head; 1e-4 relative in one slice of vap_head itself: 8.4 x)
    vad_logit   5583 x  (the row before; the stereo tower instead of ``o``: 5e5 x)
    p_now       3358 x  (now / future bins swapped for channel 1)
    p_future    3552 x  (future from bin 3 alone)
    vad         635 x   (the second sigmoid a copy of the first)
    aux         19464 x (softmax over 4 rows in bc mode; over 3 rows in nod mode: 1e5 x)
    p_bc_rows   119 x   (the newest row's p_bc from row n - 2)

A stage's factor
(``head_stages.STAGE_FACTOR``) may only be raised while every fault of that stage keeps a 1.5 x margin; the test asserts it."""
import functools

import numpy as np
import pytest

import head_stages as HS

CASES = ((20, "vap"), (20, "bc"), (20, "nod"), (50, "vap"), (50, "nod"))
CTX = {20: 0.5, 50: 0.24}                                # T = 10, 12
AMPS = (1e-3, 1.0, 30.0)
SEED = 29
REL = 1e-4
REL_SMALL = 3e-5                                         # 500 ulp: still 2.4 x the bound of ``last``, and under the output bar
EXTRA = 4                                                # ticks after the window is full

ALL = ("vap", "bc", "nod")
# fault -> {mode: the stage that must reject it}
FAULTS = {
    "self_drops_oldest_key": dict.fromkeys(ALL, "last"),
    "self_drops_newest_odd_key": dict.fromkeys(ALL, "last"),
    "n1_counts_padded_key": dict.fromkeys(ALL, "last"),
    "cross_reads_own_channel": dict.fromkeys(ALL, "last"),
    "alibi_slope_from_neighbour": dict.fromkeys(ALL, "last"),
    "self_scale_from_head_dim": dict.fromkeys(ALL, "last"),
    "last_slice_rel": dict.fromkeys(ALL, "last"),
    "last_slice_rel_small": dict.fromkeys(ALL, "last"),
    "comb_unbiased_var": {"vap": "logits", "bc": "logits", "nod": "comb"},
    "comb_slice_rel": {"vap": "logits", "bc": "logits", "nod": "comb"},
    "head_slice_rel": {"vap": "logits", "bc": "logits"},
    "vad_reads_tower": dict.fromkeys(ALL, "vad_logit"),
    "vad_row_before": dict.fromkeys(ALL, "vad_logit"),
    "bins_swapped_ch1": dict.fromkeys(ALL, "p_now"),
    "future_bin3_only": dict.fromkeys(ALL, "p_future"),
    "vad_second_copies_first": dict.fromkeys(ALL, "vad"),
    "aux_4_rows_in_bc": {"bc": "aux"},
    "aux_3_rows_in_nod": {"nod": "aux"},
    "pbc_newest_from_row_before": {"nod": "p_bc_rows"},
}
# Faults that the bound does NOT separate on these weights; they run along and their figures are printed, nothing is asserted of them.
# tanh-GELU in the last-row FFN reaches 0.71 - 1.33 x the bound of ``last`` (at it: seen on some ticks only) and moves the outputs by 4e-5; a combinator LayerNorm
# epsilon of 1e-4 moves ``comb`` by less than the fp32 oracle's own error (the variance of the combinator's projections is in the
# hundreds, so no epsilon of that size shows) and the outputs by 9e-8.
UNSEEN = {"tanh_gelu_last_ffn": dict.fromkeys(ALL, "last"), "comb_eps": {"vap": "logits", "bc": "logits", "nod": "comb"}}
# the window fills (1-based n) on which a fault can act; default: every tick
ACTS = {"self_drops_oldest_key": lambda n: n >= 2, "self_scale_from_head_dim": lambda n: n >= 2, "self_drops_newest_odd_key": lambda n: n >= 2, "n1_counts_padded_key": lambda n: n == 1,
        "alibi_slope_from_neighbour": lambda n: n >= 2, "vad_row_before": lambda n: n >= 2, "pbc_newest_from_row_before": lambda n: n >= 2}


def faulty_oracle(fault, *args, **kw):
    """A VapOracle whose tail is restated here with one fault (None: none).  ``encode`` hands back ``next_e``, the clean oracle's
    embedding of the tick: the encoder is not the subject."""
    import math

    import torch
    import torch.nn.functional as F
    from oracle.vap_oracle import DIM, HEADS, VapOracle

    class Faulty(VapOracle):
        next_e = None

        def encode(self, audio, st, collect=None):
            return self.next_e

        def _mha(self, pre, q_in, kv_in):
            v = self.v
            B, n, _ = q_in.shape
            q = (q_in @ v[f"{pre}.query.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
            k = (kv_in @ v[f"{pre}.key.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
            val = (kv_in @ v[f"{pre}.value.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
            att = torch.einsum("bhid,bhjd->bhij", q, k) * (1.0 / math.sqrt(DIM))
            if pre == "ar.layers.2.mha" and fault == "self_scale_from_head_dim":       # 1 / sqrt(64) where the reference has 1 / sqrt(256)
                att = att.clone()
                att[:, :, -1] *= 2.0
            m = v[f"{pre}.m"].view(1, HEADS, 1, 1)
            j = torch.arange(n, dtype=self.dtype).view(1, 1, 1, n)
            bias = (m * j + torch.full((n, n), float("-inf")).triu(1)).clone()        # [1, H, n, n]
            if pre == "ar.layers.2.mha":                                              # the newest row's query only
                if fault == "alibi_slope_from_neighbour":
                    bias[0, 1, -1] = bias[0, 0, -1]
                if fault == "self_drops_oldest_key" and n >= 2:
                    bias[0, :, -1, 0] = float("-inf")
                if fault == "self_drops_newest_odd_key" and n >= 2:
                    bias[0, :, -1, n - 1 if (n - 1) % 2 else n - 2] = float("-inf")
            att = (att + bias).softmax(dim=-1)
            if pre == "ar.layers.2.mha" and fault == "n1_counts_padded_key" and n == 1:
                att = att * 0.5                          # one padded key with p = exp(0) = 1 in the denominator, no value row
            y = (att @ val).transpose(1, 2).reshape(B, n, DIM)
            return y @ v[f"{pre}.proj.weight"].T

        def _ln(self, x, name):
            eps = 1e-4 if fault == "comb_eps" and name == "ar.combinator.ln" else 1e-5
            if name == "ar.combinator.ln" and fault == "comb_unbiased_var":
                y = (x - x.mean(-1, keepdim=True)) * torch.rsqrt(x.var(-1, keepdim=True, unbiased=True) + eps)
                return y * self.v[f"{name}.weight"] + self.v[f"{name}.bias"]
            y = F.layer_norm(x, (DIM,), self.v[f"{name}.weight"], self.v[f"{name}.bias"], eps)
            if name == "ar.combinator.ln" and fault == "comb_slice_rel":
                y = y.clone()
                y[..., 32:64] *= 1.0 + REL
            return y

        def layer(self, pre, x, src):
            if pre != "ar.layers.2":
                return super().layer(pre, x, src)
            v = self.v
            x_in = x
            z = self._ln(x, f"{pre}.ln_self_attn")
            x = x + self._mha(f"{pre}.mha", z, z)
            z = self._ln(x, f"{pre}.ln_src_attn")
            x = x + self._mha(f"{pre}.mha_cross", z, x_in if fault == "cross_reads_own_channel" else src)
            z = self._ln(x, f"{pre}.ln_ffnetwork")
            hid = F.gelu(z @ v[f"{pre}.ffnetwork.0.weight"].T, approximate="tanh" if fault == "tanh_gelu_last_ffn" else "none")
            x = x + hid @ v[f"{pre}.ffnetwork.3.weight"].T
            if fault in ("last_slice_rel", "last_slice_rel_small"):   # one wave's 32 output columns of the newest row
                x = x.clone()
                x[:, -1, 32:64] *= 1.0 + (REL if fault == "last_slice_rel" else REL_SMALL)
            return x

        def step(self, audio, st, collect=None):
            with torch.no_grad():
                e = self.encode(audio, st, collect)
                st.ring.append(e)
                if len(st.ring) > self.T:
                    st.ring = st.ring[-self.T:]
                X = torch.stack(st.ring, dim=2)
                n = X.shape[2]
                o1, o2, a, b, h = self.transformer(X[:, 0], X[:, 1], collect)
                v = self.v
                va, vb = (a, b) if fault == "vad_reads_tower" else (o1, o2)
                r = -2 if fault == "vad_row_before" and n >= 2 else -1
                vad_logit = torch.stack([(va[:, r] @ v["va_classifier.weight"].T + v["va_classifier.bias"])[:, 0],
                                         (vb[:, r] @ v["va_classifier.weight"].T + v["va_classifier.bias"])[:, 0]], dim=1)
                vad = torch.sigmoid(vad_logit)
                if fault == "vad_second_copies_first":
                    vad = torch.stack([vad[:, 0], vad[:, 0]], dim=1)
                out = {"vad": vad.numpy()}
                logits = h[:, -1] @ v["vap_head.weight"].T + v["vap_head.bias"]
                if fault == "head_slice_rel":
                    logits = logits.clone()
                    logits[:, 32:64] *= 1.0 + REL
                probs = logits.softmax(dim=-1)
                w_now, w_fut = self.abp_now.clone(), self.abp_fut.clone()
                if fault == "bins_swapped_ch1":
                    w_now[:, 1], w_fut[:, 1] = self.abp_fut[:, 1], self.abp_now[:, 1]
                if fault == "future_bin3_only":
                    w_fut = torch.from_numpy(HS._BITS[:, :, 3]).to(self.dtype)
                pn, pf = probs @ w_now, probs @ w_fut
                out["logits"] = logits.numpy()
                out["p_now"] = (pn / (pn.sum(-1, keepdim=True) + 1e-5)).numpy()
                out["p_future"] = (pf / (pf.sum(-1, keepdim=True) + 1e-5)).numpy()
                if self.mode == "bc":
                    aux = h[:, -1] @ v["bc_head.weight"].T + v["bc_head.bias"]
                    sm = aux.softmax(-1)
                    if fault == "aux_4_rows_in_bc":      # the fourth weight row of a bc engine is zero: one more exp(0 - max)
                        sm = torch.cat([aux, torch.zeros_like(aux[:, :1])], dim=1).softmax(-1)[:, :3]
                elif self.mode == "nod":
                    aux = h[:, -1] @ v["nod_head.weight"].T + v["nod_head.bias"]
                    sm = aux.softmax(-1)
                    if fault == "aux_3_rows_in_nod":
                        sm = torch.cat([aux[:, :3].softmax(-1), torch.zeros_like(aux[:, :1])], dim=1)
                    pbc = torch.sigmoid(h @ v["bc_head.weight"].T + v["bc_head.bias"])[..., 0].clone()
                    if fault == "pbc_newest_from_row_before" and n >= 2:
                        pbc[:, -1] = pbc[:, -2]
                    out["p_bc"] = pbc.numpy()
                if collect is not None:
                    collect["vad_logit"] = vad_logit
                    if self.mode != "vap":
                        collect["aux"] = sm
                out["e"] = e.numpy()
            return out

    return Faulty(*args, **kw)


def scaled_dialogues(hz, frames):
    from vap_realtime_amd import synth
    hop = 16000 // hz
    audio = synth.dialogue_batch([SEED + i for i in range(len(AMPS))], hop * frames)
    return audio * np.asarray(AMPS, np.float32)[:, None, None]


OUTPUTS = ("p_now", "p_future", "vad", "logits", "aux", "p_bc_rows")


@functools.lru_cache(maxsize=None)
def run_case(hz, mode):
    """Steps the float64 and fp32 oracles and one float64 restatement per fault over T + EXTRA ticks.  Returns (accept, faults, moved):
    accept[stage] = worst fp32 err / bound; faults[name] = per tick (n, first rejecting stage, message, err / bound at the fault's own
    stage); moved[name] = the largest change of any output (float64 against float64)."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import weights as W
    torch.set_num_threads(min(8, torch.get_num_threads()))
    cpc, vap = W.synthetic_weights(SEED, hz, mode)
    hop, S = 16000 // hz, len(AMPS)
    o64, o32 = VapOracle(cpc, vap, hz, CTX[hz], mode=mode, dtype=torch.float64), VapOracle(cpc, vap, hz, CTX[hz], mode=mode)
    frames = o64.T + EXTRA
    audio = scaled_dialogues(hz, frames)
    names = [None] + [f for f, per in {**FAULTS, **UNSEEN}.items() if mode in per]
    bad = {f: faulty_oracle(f, cpc, vap, hz, CTX[hz], mode=mode, dtype=torch.float64) for f in names}
    s64, s32, sbad = o64.new_state(S), o32.new_state(S), {f: o.new_state(S) for f, o in bad.items()}
    fr = ServerFramer(S, hop)
    accept, faults, moved = {}, {f: [] for f in names}, {f: 0.0 for f in names}
    for t in range(frames):
        frame = fr.frame(audio[:, :, t * hop:(t + 1) * hop])
        r64, r32 = HS.collect_heads(o64, frame, s64), HS.collect_heads(o32, frame, s32)
        w64, w32 = [HS.row_of(r64, k) for k in range(S)], [HS.row_of(r32, k) for k in range(S)]
        what = f"{hz} Hz {mode} tick {t + 1}"
        HS.check_tick(mode, w32, w64, w32, what=what + " fp32 oracle", excess=accept)
        HS.check_own(w32, what=what + " fp32 oracle", excess=accept)
        for f, o in bad.items():
            o.next_e = torch.from_numpy(r64["e"])
            rb = HS.collect_heads(o, frame, sbad[f])
            rows = [HS.row_of(rb, k) for k in range(S)]
            first, msg = None, ""
            try:
                HS.check_tick(mode, rows, w64, w32, what=f"{what} {f}")
                HS.check_own(rows, what=f"{what} {f}")
            except AssertionError as e:
                msg = str(e)
                first = msg.split(": ", 1)[1].split(" (", 1)[0]
            ex = 0.0
            if f is not None:
                stage = {**FAULTS, **UNSEEN}[f][mode]
                e32 = HS.pooled_e32(stage, w64, w32)
                ex = max(float(np.abs(np.asarray(rows[k][stage], np.float64) - w64[k][stage]).max()) / HS.stage_bound(stage, e32, w64[k][stage])[0]
                         for k in range(S))
            faults[f].append((r64["n"], first, msg, ex))
            for q in OUTPUTS:
                if q in rb and q in r64:
                    moved[f] = max(moved[f], float(np.abs(np.asarray(rb[q], np.float64) - r64[q]).max()))
    return accept, faults, moved


@pytest.mark.parametrize("hz,mode", CASES)
def test_fp32_oracle_passes_and_the_restatement_is_the_oracle(hz, mode):
    accept, faults, moved = run_case(hz, mode)
    assert set(accept) == set(HS.stages_of(mode)) | {"own " + s for s in HS.OWN}, sorted(accept)
    for st, r in accept.items():
        assert r <= (1.0 / HS.STAGE_FACTOR.get(st, HS.FACTOR) if not st.startswith("own ") else 1.0) + 1e-9, (hz, mode, st, r)
    print(f"{hz} Hz {mode}: fp32 oracle err / bound per stage", {st: round(r, 3) for st, r in accept.items()})
    assert all(first is None for _, first, _, _ in faults[None]), faults[None]
    assert moved[None] < 1e-12, moved[None]              # float64 both: the restatement without a fault is the oracle


def test_faults_are_rejected_at_their_stage():
    margins = {}
    for hz, mode in CASES:
        _, faults, _ = run_case(hz, mode)
        for f, per in FAULTS.items():
            if mode not in per:
                continue
            stage, acted = per[mode], 0
            for n, first, msg, ex in faults[f]:
                if not ACTS.get(f, lambda n: True)(n):
                    assert first is None, f"{hz} Hz {mode} n = {n}: fault {f} cannot act here, yet: {msg}"
                    continue
                acted += 1
                assert first == stage, f"{hz} Hz {mode} n = {n}: fault {f} should be rejected at {stage}, first rejection: {first} {msg}"
                assert f": {stage} ({HS.kernel_of(stage)})" in msg, msg
                margins[(stage, f)] = min(margins.get((stage, f), np.inf), ex)
            assert acted, (hz, mode, f)
    for f, per in UNSEEN.items():                        # printed, not asserted: the bound does not promise to see these
        ex = [x for hz, mode in CASES if mode in per for _, _, _, x in run_case(hz, mode)[1][f]]
        print(f"{f} (not required): {min(ex):.2f} .. {max(ex):.2f} x bound at {sorted(set(per.values()))}")
    for stage in HS.STAGES:
        mine = {f: m for (s, f), m in margins.items() if s == stage}
        assert mine, f"no fault is seeded at stage {stage}"
        f = min(mine, key=mine.get)
        print(f"{stage}: smallest rejection margin {mine[f]:.1f} x bound ({f}); all:", {k: round(v, 1) for k, v in mine.items()})
        # measured with the stage's factor in force, so a raised factor has to leave MARGIN of every rejection
        assert mine[f] >= (HS.MARGIN if stage in HS.STAGE_FACTOR else 1.0), (stage, f, mine[f])


# the faults that move no output (p_now, p_future, vad, logits, aux, p_bc rows) by 1e-4 in any case of CASES: invisible to the output
# parity tests, and the recorded reason for tests/test_head_stages_gpu.py
UNDER_THE_OUTPUT_BAR = ("last_slice_rel_small",)


def test_faults_against_the_output_bar():
    worst = {}
    for hz, mode in CASES:
        _, _, moved = run_case(hz, mode)
        for f, d in moved.items():
            if f is not None:
                worst[f] = max(worst.get(f, 0.0), d)
    for f, d in worst.items():
        print(f"{f}: moves the outputs by at most {d:.2e}" + ("  (under the 1e-4 output bar)" if d < 1e-4 else ""))
    assert tuple(f for f in FAULTS if worst[f] < 1e-4) == UNDER_THE_OUTPUT_BAR, worst
    assert all(worst[f] < 1e-4 for f in UNSEEN), worst   # nor does the output bar see what the stage bound does not


def test_the_own_logits_check_sees_what_the_stage_bound_may_not():
    """p_future's denominator without its + 1e-5 moves p_future by 1e-5 relative: the stage bound (8e-6 of max|p| and more) may or may
    not see it, the check against the row's own logits (which has no upstream error to allow for) does."""
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((4, 256)) * 3.0
    vad_logit = rng.standard_normal((4, 2))
    own = HS.own_probabilities(logits, vad_logit)
    rows = [{"logits": logits[k], "vad_logit": vad_logit[k], **{s: own[s][k].astype(np.float32) for s in HS.OWN}} for k in range(4)]
    ex = {}
    HS.check_own(rows, excess=ex)
    assert max(ex.values()) < 0.02, ex                   # fp32 rounding of exact values: 6e-8 / 8e-6
    rows[2]["p_future"] = rows[2]["p_future"] * np.float32(1.0 + 1e-5)
    with pytest.raises(AssertionError, match=r"stream 2: p_future \(head_kernel\) differs from float64"):
        HS.check_own(rows)


def test_exact_fields_are_checked_exactly():
    T, ns = 6, [3, 6]
    out = np.zeros((2, 784), np.float32)
    e = np.random.default_rng(1).standard_normal((2, 2, 256)).astype(np.float32)
    out[:, 272:] = e.reshape(2, 512)
    out[:, 10] = ns
    out[:, 6:10] = 0.25
    out[0, 16:19] = 0.5
    out[1, 16:22] = 0.5
    HS.check_exact("nod", out, ns, e, T)
    for mode, col, val, word in (("nod", 10, 4.0, "OUT_NVALID"), ("nod", 13, 1.0, "status"), ("nod", 15, 1e-45, "reserved"),
                                 ("bc", 9, 0.25, "aux columns 3"), ("vap", 6, -0.0, "aux columns 0"), ("nod", 16 + 4, 0.5, "p_bc slots 3"),
                                 ("nod", 272 + 300, 7.0, "channel 1 column 44")):
        bad = out.copy()
        if mode != "nod":
            bad[:, 6:10] = 0.0
            if mode == "bc":
                bad[:, 6:9] = 0.3
        bad[0, col] = val
        with pytest.raises(AssertionError, match=f"stream 0.*{word}"):
            HS.check_exact(mode, bad, ns, e, T)


def test_nod_engine_refuses_more_than_256_context_frames():
    """An output row holds 256 p_bc slots, one per window row; pbc_rows_kernel used to drop rows >= 256 silently.  The refusal comes
    before vapx_create looks for a device."""
    from vap_realtime_amd import engine, weights as W
    cpc, vap = W.synthetic_weights(3, 50, "nod")
    blob = W.pack_blob(cpc, vap, "nod")
    with pytest.raises(engine.VapxError, match="nod mode needs ctx_frames <= 256 .got 257.: the output row holds 256 p_bc slots"):
        engine.Engine(blob, 50, 257 / 50 + 1e-9, max_streams=1, mode="nod")
