"""Every stage of the HIP path against the float64 oracle under weight regimes that feed the non-linearities what a trained checkpoint
can: tests/weight_regimes.py has the regimes, the fp32-derived thresholds they pass and the seeded faults; tests/test_weight_regimes.py
proves both on the CPU.  Every other float64-held module draws its weights from ``synthetic_weights`` alone, where no sigmoid
saturates, no GELU input leaves the fitted erfc and no softmax row spreads beyond 20.

The bound is the project's own, unchanged: 8 x max(E32, 1e-6 max|x|) per stream block (``encoder_stages.check_stage``,
``layer_rows.check_rows``, ``head_stages.check_tick`` / ``check_own``), E32 the torch fp32 oracle's error against float64 on the same inputs.

(a) encoder, teacher-forced (``weight_regimes.teacher_ticks``): before each of 12 checked ticks (frames 1-3 and 27-35 of 35) the float64
    state rounded to fp32 - h, c, carry, window - goes into the engine (``set_state``) and into both oracles; one step; h0 .. h3 (off the
    fused tail), z, lstm_out, e and the new h and c are held, the carry bit for bit.  3 dialogues at amplitudes 1e-3 / 1 / 30; regimes
    base, lstm, gains, tiny; 20 Hz fp32 fused tail, fp32 unfused_conv, split; 50 Hz fp32 and split.
    No free-running assertion under ``lstm``: the recurrence amplifies rounding, so the fp32 oracle's OWN free-running error is no
    yardstick there.  Measured on the MI355X machine (3 dialogues, 40 free-running frames at 20 Hz, error relative to max|lstm_out|):
    under ``base`` the fp32 oracle stays at 7e-7 (frame 1: 7.4e-7, frame 40: 6.5e-7) and the fp32 engine at 1.5e-6 - 2.1e-6; under ``lstm``
    the fp32 oracle goes from 4.0e-6 at frame 1 to 1.2e-4 at frame 40 (9.2e-4 on the way) and the engine from 2.1e-5 to 8.0e-4 (2.9e-3):
    k x E32 of such a run compares two amplified roundings.  One tick from a common state has no such history.
    Even one tick is five recurrent steps at 20 Hz, and with the fp32 oracle as the only reference the stages behind z come to
    0.94 (fp32) and 1.00 (split: h at 1.216e-5 against a bound of 1.215e-5, tick 29) of the bound under ``lstm``, 0.27 under ``base``.
    The cause is the rule itself, not a kernel: it allows a path 1e-6 max|z| on z, three times the fp32 oracle's own error there, and
    W_ih x 6 hands that on.  ``weight_regimes.recurrent_reference`` therefore adds a second reference for lstm_out / e / h / c, made of
    float64 and the fp32 oracle alone (the float64 LSTM fed the fp32 oracle's z error scaled to that allowance); the rule
    8 x max(E(reference), 1e-6 max|x|) is unchanged, h0 .. z keep the fp32 oracle, and both figures are printed.
(b) transformer rows: one ragged batch per window (``weight_regimes.row_states``: 33, T - 1, T and T + 37 frames) through
    ``window_sweep.drive``; the truth is both oracles' ``layers`` on the window the engine EXPORTS, so the encoder's error is not the
    subject.  Regimes ffn, ffn300, attn, gains; T = 50 (attn_block_kernel, FFN block mode 0), 100 (attention_long2 / f16x3 / proj_f16x3,
    flat-row blocks modes 1 / 2), 257 (attention_xl_kernel); fp32, split, fp32_full, and split_full at T = 100.  ``last`` (last_block_kernel)
    rides along where the last layer is pruned.  Under ffn300 both the fp32 and the split path (hid_scale < 1) are thus held against
    float64; tests/test_split_precision_gpu.py keeps comparing them with each other.
(c) heads: ``test_head_stages_gpu.run_case`` under heads and gains: vap / bc / nod with every small-batch variant (last_block_kernel<8>,
    head_kernel<2>, unfused_last_row, full_last_layer, split) at n = 1, 2, 3, 7, 8, 9, and B = 1025 (last_block_kernel<16>, head_kernel<4>;
    nod: run_combinator_all_rows, pbc_rows_kernel).
(c') the last-row path under attn: ``test_head_stages_gpu.run_case`` at 50 Hz, T = 130 with the checkpoints of its key-count case (n = 63,
    64, 65, 127 .. 131, 137): attention_last_kernel's 64-key chunks and their rescale ``expf(mx - mn)``, fp32 and split, and
    last_block_kernel, with query / key x 3.
(d) unit entries: vapx_gemm epi 1 and 5 with GELU inputs of +-30 and beyond, vapx_softmax256 with row spreads 50 / 104 / 200, tied
    maxima and a row of equal values, same bound.
Every case of (b), (c) and (c') asserts what the float64 oracle reached ON ITS OWN inputs (GELU input, softmax spread, head logit spread,
VAD logit), so a change of seed, donor or window that drops a regime back into the base range fails instead of passing quietly.
(e) the split path's static guarantee (each of the 16 norms): a ChannelNorm / LayerNorm with 16 |gamma| + |beta| >= 65504 in front of an unscaled f16 operand is
    refused by vapx_create under VAPX_FLAG_SPLIT_F16, by name, and accepted by the fp32 engine; ``gains`` (bound 131) is accepted.

Coverage map: non-linearity site -> the case that takes its input beyond the ``base`` range (reach printed per case with -s).

    site                                                           case                          input reached
    lstm_kernel: fast_sigmoid / fast_tanh (gates, cell)            (a) lstm; tiny                gates 20, cell 172; gates < 0.05
    gelu_erf in lstm_kernel's fused downsample                     (a) gains                     +-20
    gelu_fast, ffn_block_kernel mode 0                             (b) T = 50 fp32, ffn / gains  26 / 21
    gelu_fast, ffn_block_kernel modes 1 / 2                        (b) T = 100, 257 fp32         26 / 21; ffn300: 2000
    exp2 GELU of ffn_block_f16x3                                   (b) split, every T            the same; ffn300 with hid_scale = 1/4
    gelu_fast in last_block_kernel                                 (b) ``last`` of fp32 / split  the same
    gelu_erf, GEMM epi 1 / 5                                       (d)                           +-30 .. 45
    gelu_erf, Combinator (head_kernel, run_combinator_all_rows)    (c) gains, nod included       +-20
    softmax: attn_block_kernel                                     (b) attn T = 50               spread 165, |logit| 590
    softmax: attention_long2, attention_long_f16x3, proj_f16x3     (b) attn T = 100 fp32 / split spread 190
    softmax: attention_xl_kernel                                   (b) attn T = 257              spread 209
    softmax: last_block_kernel (newest row)                        (b) attn ``last``
    softmax: last-row path (attention_last_kernel), and            (c') attn, T = 130, n = 63 .. 65, 127 .. 137: unfused_last_row fp32 / split and the
      last_block_kernel across its key groups                      fused block; spread inside the newest row 238 (asserted > 104)
    softmax: attention_map_kernel                                  out of scope here, not out of reach: vapx_transformer_maps is held against the
                                                                   oracle's maps by tests/test_attention_maps_gpu.py under base only; a case under
                                                                   ``attn`` against softmax(collect["pre"]["att.*"]) would need a harness of its own
    head softmax, aux softmax, VAD sigmoid (head_kernel)           (c) heads                     spread 100, VAD logit 50
    p_bc sigmoid (pbc_rows_kernel)                                 (c) heads, nod
    vapx_softmax256                                                (d)                           spread 200

Worst err / bound (the asserted figure; every case prints its own with -s), measured on an MI355X, fp32 variants | split variants.
No kernel left the bound and none was changed; the module takes 40 s, its slowest case 2.5 s.

    (a) encoder, worst over 20 and 50 Hz           h0    h1    h2    h3    z     lstm_out  e     h     c
        base    fp32 | split                       0.05  0.20  0.14  0.15  0.16  0.19      0.21  0.18  0.18  |  0.05  0.17  0.12  0.13  0.17  0.15  0.18  0.16  0.14
        lstm    (cell 172, gates 20)               0.05  0.20  0.14  0.15  0.16  0.25      0.24  0.25  0.24  |  0.05  0.17  0.12  0.13  0.17  0.26  0.23  0.32  0.30
        gains   (cell 51, e 20)                    0.04  0.19  0.20  0.17  0.24  0.43      0.22  0.51  0.16  |  0.04  0.15  0.18  0.15  0.17  0.28  0.18  0.48  0.15
        tiny    (cell 0.045, h 0.023)              0.05  0.20  0.14  0.15  0.16  0.20      0.03  0.20  0.16  |  0.05  0.17  0.12  0.13  0.17  0.22  0.04  0.22  0.16
        with the fp32 oracle as the only reference, lstm_out / e / h / c:  base 0.27 0.21 0.27 0.19 | 0.19 0.18 0.19 0.15;
        lstm 0.87 0.55 0.94 0.88 | 0.96 0.44 1.00 0.50;  gains 0.53 0.22 0.61 0.30 | 0.66 0.18 0.66 0.23;  tiny as above
    (b) rows, worst over T = 50, 100, 257          o     stereo0  stereo1  stereo2  last
        ffn     (GELU input -28.7 .. 25.7)         0.23  0.27     0.27     0.28     0.09  |  0.14  0.22  0.18  0.21  0.10
        ffn300  (GELU input -2149 .. 1921)         0.20  0.25     0.25     0.24     0.13  |  0.16  0.23  0.20  0.17  0.07
        attn    (row spread 165 / 190 / 209)       0.21  0.38     0.34     0.53     0.38  |  0.20  0.35  0.29  0.31  0.28
        gains   (GELU -21.3 .. 18.1, spread 94)    0.32  0.34     0.33     0.31     0.15  |  0.21  0.20  0.23  0.28  0.18
    (c) heads, worst over vap / bc / nod, B = 3 and 1025
                  last  comb  logits  vad_logit  p_now  p_future  vad   aux   p_bc_rows  own p_now / p_future / vad
        heads     0.27  0.20  0.26    0.42       0.49   0.39      0.33  0.22  0.46       0.02 / 0.02 / 0.01   |  0.21  0.14  0.16  0.38  0.20  0.20  0.13  0.00  0.14
        gains     0.38  0.51  0.20    0.42       0.24   0.54      0.64  0.12  0.42       0.02 / 0.01 / 0.01   |  0.22  0.30  0.14  0.47  0.20  0.21  0.86  0.14  0.20
        Under ``heads`` each value p of vad / aux / p_bc_rows is held to max(the stage's own bound, a p (1 - p) B + r B^2), B the bound of
        its logits and p the float64 value (``head_stages.PROPAGATE``; a saturated p keeps its own bound): with the head weights x 8 the
        rule allows the VAD logit 8e-6 x 50, and an exact sigmoid turns that into up to 1e-4 of an unsaturated vad, where vad's own bound is 8e-6.  Without it vad came to 3.5 x its own bound (bc, fp32: 1.15e-5 against 3.3e-6 at a logit within 0.42 of
        ITS bound; the sigmoid alone, ``own vad``, is at 0.01) and the aux softmax of nod at B = 1025 to 1.07 x.  ``gains`` runs without it.
    (c') last-row path under attn, T = 130 (|logit| 777, spread inside the newest row 238):
                                  last  logits  vad_logit  p_now  p_future  vad   own p_now / p_future / vad
        fused (last_block_kernel) 0.71  0.93    0.49       0.62   0.47      0.29  0.01 / 0.01 / 0.01
        unfused_last_row          0.69  0.90    0.49       0.60   0.49      0.29  0.01 / 0.01 / 0.01
        split_unfused_last_row    0.53  0.42    0.30       0.19   0.36      0.20  0.02 / 0.01 / 0.01
    (d) vapx_gemm epi 1: 0.08, epi 5: 0.17 (every tile); vapx_softmax256: 0.01 on every row.
"""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import encoder_stages as ES
import test_encoder_stages_gpu as EG
import test_head_stages_gpu as HG
import weight_regimes as WR
import window_sweep as ws
from layer_rows import BUFFERS, FACTOR, FLOOR
from test_layer_rows_gpu import Variant, make_engine

pytestmark = pytest.mark.gpu

SEED = 23


# ---- (a) the encoder, teacher-forced -----------------------------------------------------------------------------------------------------
ENC_VARIANTS = {20: [EG.Variant("fp32_fused", "fused", poison=True), EG.Variant("fp32_unfused_conv", "chain", unfused_conv=True),
                     EG.Variant("split", "split", poison=True, split_f16=True)],
                50: [EG.Variant("fp32", "fused", poison=True), EG.Variant("split", "split", split_f16=True)]}
SLOTS = np.array([3, 0, 4], np.int32)


@pytest.mark.parametrize("regime", ["base", "lstm", "gains", "tiny"])
@pytest.mark.parametrize("hz", [20, 50])
def test_encoder_one_tick_from_the_float64_state(hz, regime):
    from vap_realtime_amd import engine, weights as W
    cpc, vap = WR.weights(regime, SEED, hz)
    blob, ctx = W.pack_blob(cpc, vap, "vap"), EG.CTX[hz]
    geo = ES.geometry(hz)
    engines = []
    for v in ENC_VARIANTS[hz]:
        with EG.debug_env(v.poison):
            engines.append(engine.Engine(blob, hz, ctx, max_streams=5, max_batch=3, **v.kw))
    T = engines[0].T
    excess = {v.label: {} for v in ENC_VARIANTS[hz]}
    plain = {v.label: {} for v in ENC_VARIANTS[hz]}
    reach: dict = {}
    allow: dict = {}
    failed: dict = {}
    try:
        for tick in WR.teacher_ticks(cpc, vap, hz, seed=SEED, ctx=ctx):
            n = tick.ring.shape[2]
            for v, eng in zip(ENC_VARIANTS[hz], engines):
                for s, sid in enumerate(SLOTS):
                    eng.reset_stream(int(sid))
                    if n:
                        ring = np.zeros((2, T, 256), np.float32)
                        ring[:, :n] = tick.ring[s]
                        eng.set_state(int(sid), {"ring": ring, "n_frames": n, "lstm": np.stack([tick.h[s], tick.c[s]], axis=1), "carry": tick.carry[s]})
                eng.step(tick.new, SLOTS)
                fused = EG.tail_is_fused(v, hz, 3)
                got = {st: eng.peek(st, (3, 2, geo[st] + 2 * ES.GUARD.get(st, 0), 256)) for st in EG.stages_of(fused)}
                lstm = np.stack([eng.get_state(int(sid))["lstm"] for sid in SLOTS])                  # [3, 2 channels, h / c, 256]
                got["h"], got["c"] = lstm[:, :, 0][:, :, None, :], lstm[:, :, 1][:, :, None, :]
                what = f"{regime} {hz} Hz {v.label}"
                if v.label in failed:
                    continue
                try:                                         # one variant's first failure does not hide the other variants'
                    for s, sid in enumerate(SLOTS):
                        ES.check_carry(eng.get_state(int(sid))["carry"], tick.frame[s], what=f"{what} tick {tick.k + 1} stream {s}")
                    WR.check_encoder_tick(tick, got, path=v.path if v.path != "fused" or fused else "chain", what=what, excess=excess[v.label],
                                          plain=plain[v.label])
                except AssertionError as ex:
                    failed[v.label] = str(ex)
            for key, st in (("cell", "c"), ("h", "h"), ("e", "e")):
                reach[key] = max(reach.get(key, 0.0), float(np.abs(tick.r64[st]).max()))
            for st, a in tick.allow.items():
                allow[st] = max(allow.get(st, 0.0), a)
    finally:
        for eng in engines:
            eng.close()
    print(f"\nencoder {regime} {hz} Hz: float64 max", {k: round(v, 3) for k, v in reach.items()},
          "E(second reference) / max(E32, floor)", {k: round(a, 2) for k, a in allow.items()})
    for v in ENC_VARIANTS[hz]:
        print(f"encoder {regime} {hz} Hz {v.label}: worst err/bound", {k: round(r, 2) for k, r in excess[v.label].items()},
              "| fp32 oracle as the only reference", {k: round(r, 2) for k, r in plain[v.label].items()})
    assert not failed, "\n".join(failed.values())
    for v in ENC_VARIANTS[hz]:
        assert set(excess[v.label]) == set(EG.stages_of(EG.tail_is_fused(v, hz, 3))) | {"h", "c"}


# ---- (b) transformer rows ----------------------------------------------------------------------------------------------------------------
HZ_ROWS = 50
ROW_WINDOWS = (50, 100, 257)
_RIGS: dict = {}


def rig(regime):
    """Weights, blob and both oracles of a regime at 50 Hz, and the donor rows: the fp32 oracle's encoder under the regime's encoder weights
    (only ``gains`` changes them)."""
    if regime not in _RIGS:
        import torch
        from oracle.vap_oracle import VapOracle
        from vap_realtime_amd import weights as W
        cpc, vap = WR.weights(regime, SEED, HZ_ROWS)
        dk = ("donor", "gains" if regime == "gains" else "base")
        if dk not in _RIGS:
            _RIGS[dk] = ws.donor(cpc, vap, HZ_ROWS, max(ROW_WINDOWS) + ws.DONOR_EXTRA)
        _RIGS[regime] = {"blob": W.pack_blob(cpc, vap, "vap"), "o64": VapOracle(cpc, vap, HZ_ROWS, 1.0, dtype=torch.float64),
                         "o32": VapOracle(cpc, vap, HZ_ROWS, 1.0), "donor": _RIGS[dk]}
    return _RIGS[regime]


def layers_and_reach(o64, acc):
    """``o64.layers`` that also folds the inputs of the GELUs and softmaxes into ``acc`` (what the case reached on the exported windows)."""
    import torch

    def layers(st):
        with torch.no_grad():
            X = torch.stack(st.ring, dim=2)
            collect = {"pre": {}}
            o64.transformer(X[:, 0], X[:, 1], collect)
        WR.fold(collect["pre"], acc)
        return {k: collect[k].numpy() for k in BUFFERS}
    return layers


def row_variants(T):
    v = [Variant("fp32", poison=True), Variant("split", poison=True, split_f16=True), Variant("fp32_full", full_last_layer=True)]
    return v + ([Variant("split_full", split_f16=True, full_last_layer=True)] if T == 100 else [])


@pytest.mark.parametrize("T", ROW_WINDOWS)
@pytest.mark.parametrize("regime", ["ffn", "ffn300", "attn", "gains"])
def test_transformer_rows_on_the_exported_window(regime, T):
    r = rig(regime)
    ctx = (T + 0.5) / HZ_ROWS
    prog = ws.schedule(WR.row_states(T), T, seed=3)
    inject = ws.injected_rows(prog, T, r["donor"])
    audio = ws.step_audio(prog, HZ_ROWS)
    truths, reach = {}, {}
    for v in row_variants(T):
        eng = make_engine(r["blob"], HZ_ROWS, ctx, prog.max_streams, v, "vap")
        try:
            assert eng.T == T
            pruned = "stereo2" not in v.buffers("vap")
            cap = ws.drive(eng, T, prog, inject, audio, HZ_ROWS, v.buffers("vap"), pruned, what=f"{regime} {v.label}")
        finally:
            eng.close()
        key = hashlib.sha1(b"".join(w.tobytes() for w in cap.windows)).digest()
        if key not in truths:
            truths[key] = ws.truth(r["o64"], r["o32"], cap, layers64=layers_and_reach(r["o64"], reach))
        excess: dict = {}
        ws.check(cap, truths[key], v.buffers("vap"), T, what=f"{regime} {v.label}", path="fused_split" if v.kw.get("split_f16") else "fused",
                 excess=excess)
        print(f"\nrows {regime} T={T} {v.label}: worst err/bound", {b: round(x, 2) for b, x in excess.items()})
        assert set(excess) == set(v.buffers("vap")) | ({"last"} if pruned else set())
    print(f"rows {regime} T={T}: reached", {k: round(x, 1) for k, x in sorted(reach.items()) if k.startswith(("gelu_ffn", "attn"))})
    assert ROW_REACH[regime](reach), (regime, T, reach)      # on the exported windows of THIS case, not only in the CPU proof


ROW_REACH = {"ffn": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"]) > 20.0,
             "ffn300": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"]) > 300.0 * WR.ERFC_END,
             "attn": lambda r: r["attn_spread"] > WR.EXP_UNDERFLOW,
             "gains": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"]) > WR.ERFC_END}


# ---- (c) heads ---------------------------------------------------------------------------------------------------------------------------
def reach_hook(acc):
    """``pre_hook`` of the heads harness: folds what the float64 oracle fed its non-linearities at the checkpoints into ``acc``, with the
    logit spread of the NEWEST query row of the last layer (what the last-row kernels see) under ``last_row_spread``."""
    def hook(pre):
        for name in ("att.ar.layers.2.mha", "att.ar.layers.2.mha_cross"):
            for x in pre.get(name, ()):
                row = x[:, :, -1, :]                         # the newest row attends to every key: no -inf
                acc["last_row_spread"] = max(acc.get("last_row_spread", 0.0), float((row.amax(-1) - row.amin(-1)).max()))
                acc["last_row_keys"] = max(acc.get("last_row_keys", 0), row.shape[-1])
        WR.fold(pre, acc)
    return hook


HEAD_REACH = {"heads": lambda r: r["head_spread"] > WR.HEAD_SPREAD and r["vad_abs"] > WR.SIGMOID_SAT,
              "gains": lambda r: min(r["gelu_erf_pos"], r["gelu_erf_neg"]) > WR.ERFC_END}


def heads_case(regime, *args, **kw):
    reach: dict = {}
    HG.run_case(*args, weights=WR.transform(regime), propagate=regime == "heads", pre_hook=reach_hook(reach), **kw)
    print(f"{kw['label']}: reached", {k: round(v, 1) for k, v in sorted(reach.items()) if k.startswith(("head", "vad", "aux", "p_bc", "gelu_erf", "last_row"))})
    assert HEAD_REACH[regime](reach), (regime, reach)
    return reach


@pytest.mark.parametrize("regime", ["heads", "gains"])
@pytest.mark.parametrize("mode", ["vap", "bc", "nod"])
def test_heads_small_batch(mode, regime):
    heads_case(regime, 20, 20, HG.small_variants(mode), label=f"{regime} small", cps=(1, 2, 3, 7, 8, 9))


def test_last_row_path_across_key_chunks_under_attn():
    """attention_last_kernel (unfused_last_row, fp32 and split) and last_block_kernel under ``attn``, 50 Hz, T = 130, at n = 63 .. 65,
    127 .. 130 and slid 131, 137: the -1e30 sentinel and the rescale ``expf(mx - mn)`` between 64-key chunks with a logit spread beyond
    104 inside the newest row, so a chunk's running maximum can sit an underflow below the next one's."""
    reach: dict = {}
    HG.run_case(50, 130, [HG.Variant("fused", poison=True), HG.Variant("unfused_last_row", path="unfused", unfused_last_row=True),
                          HG.Variant("split_unfused_last_row", path="unfused_split", poison=True, split_f16=True, unfused_last_row=True)],
                label="attn edges", seed=67, cps=HG.EDGE_CP, weights=WR.transform("attn"), pre_hook=reach_hook(reach))
    print("attn edges: reached", {k: round(v, 1) for k, v in sorted(reach.items()) if k.startswith(("last_row", "attn"))})
    assert reach["last_row_spread"] > WR.EXP_UNDERFLOW and reach["last_row_keys"] == 130, reach


@pytest.mark.parametrize("regime", ["heads", "gains"])
@pytest.mark.parametrize("mode", ["vap", "nod"])
def test_heads_1025_streams(mode, regime):
    heads_case(regime, 20, 20, [HG.Variant(f"{mode}_B1025", mode, "full" if mode == "nod" else "fused", poison=True)], label=f"{regime} tiles", seed=71,
                n_dialogues=4, copies=1025, slots=1028, cps=(1, 2, 4), late=False)


# ---- (d) unit entries --------------------------------------------------------------------------------------------------------------------
def held(name, got, want64, want32):
    """The project's bound on one block: 8 x max(E32, 1e-6 max|x|)."""
    want64 = np.asarray(want64, np.float64)
    e32 = float(np.abs(np.asarray(want32, np.float64) - want64).max())
    bound = FACTOR * max(e32, FLOOR * float(np.abs(want64).max()))
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite value at {tuple(int(i[0]) for i in np.nonzero(~np.isfinite(got)))}"
    err = np.abs(got - want64)
    at = tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
    print(f"\n{name}: worst err/bound {err.max() / bound:.2f} (E32 {e32:.2e}, max|x| {np.abs(want64).max():.3g})")
    assert err.max() <= bound, f"{name}: index {at} is off by {err.max():.3e} > bound {bound:.3e} (E32 {e32:.3e}; got {got[at]!r}, want {want64[at]!r})"


@pytest.mark.parametrize("tile", [32, 64, 0])
@pytest.mark.parametrize("epi,N,K,M", [(1, 768, 256, 257), (5, 256, 1280, 70)])
def test_gemm_gelu_epilogues_at_30(epi, N, K, M, tile):
    """EPI_GELU on accumulators of std 10 (+-30 and beyond), EPI_BIAS_LN_GELU with gamma = +-8 (1 +- 0.2): gelu_erf far outside +-6."""
    import torch
    import torch.nn.functional as F
    from vap_realtime_amd import engine
    lib = engine.load_library()
    g = torch.Generator().manual_seed(77 + epi)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * ((10.0 if epi == 1 else 1.0) / K ** 0.5)
    bias = torch.randn(N, generator=g) * 0.3
    gamma = 8.0 * (1 + 0.2 * torch.randn(N, generator=g)) * torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0)
    beta = 2.0 * torch.randn(N, generator=g)

    def ref(dt):
        acc = A.to(dt) @ W.to(dt).T
        if epi == 1:
            return acc, F.gelu(acc)
        y = F.layer_norm(acc + bias.to(dt), (256,), gamma.to(dt), beta.to(dt), 1e-5)
        return y, F.gelu(y)
    (pre64, want64), (_, want32) = ref(torch.float64), ref(torch.float32)
    assert pre64.max() > 30 and pre64.min() < -30
    dA, dW, db, dg, dbe = (t.cuda().contiguous() for t in (A, W, bias, gamma, beta))
    dC = torch.full((M, N), float("nan"), device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.vapx_gemm(None, M, N, K, p(dA), p(dW), p(dC), epi, p(db) if epi == 5 else None, p(dg), p(dbe), None, None, tile)
    assert rc == 0, lib.vapx_last_error(None)
    torch.cuda.synchronize()
    held(f"vapx_gemm epi {epi} tile {tile} (GELU input {float(pre64.min()):.0f} .. {float(pre64.max()):.0f})", dC.cpu().numpy(), want64.numpy(), want32.numpy())


def test_softmax256_wide_rows():
    """Row spreads 50, 104 (fp32 exp underflows) and 200, the maximum tied 2, 3 and 256 times (a row of equal values), at both ends and in
    the middle of the row; 4 rows per workgroup, so 11 rows leave a partial one."""
    import torch
    from vap_realtime_amd import engine
    lib = engine.load_library()
    rng = np.random.default_rng(5)
    rows = []
    for spread in (50.0, 104.0, 200.0):
        x = rng.uniform(-spread, 0.0, 256)
        x[rng.integers(256)] = 0.0
        x[rng.integers(256)] = -spread
        rows.append(x + rng.uniform(-300, 300))
        y = x.copy()
        y[[0, 255]] = 0.0                                    # tied maxima at both ends
        rows.append(y)
        z = x.copy()
        z[[100, 101, 102]] = 0.0
        rows.append(z - 1000.0)
    rows += [np.full(256, 37.5), np.full(256, -1e4)]
    X = torch.from_numpy(np.stack(rows).astype(np.float32))
    dX = X.cuda()
    dY = torch.full(X.shape, float("nan"), device="cuda")
    assert lib.vapx_softmax256(X.shape[0], dX.data_ptr(), dY.data_ptr(), None) == 0
    torch.cuda.synchronize()
    got, want64, want32 = dY.cpu().numpy(), X.double().softmax(-1).numpy(), X.softmax(-1).numpy()
    for r in range(X.shape[0]):
        held(f"vapx_softmax256 row {r} (spread {float(X[r].max() - X[r].min()):.0f})", got[r], want64[r], want32[r])
    assert np.allclose(got[-1], 1.0 / 256, rtol=1e-6) and np.allclose(got[-2], 1.0 / 256, rtol=1e-6)


# ---- (e) the split path's static guarantee for its unscaled f16 operands -----------------------------------------------------------------
LAYERS = ("ar_channel.layers.0", "ar.layers.0", "ar.layers.1", "ar.layers.2")
NORMS = ([("cpc", f"gEncoder.batchNorm{i}", f"cn{i}") for i in range(5)] +
         [("vap", f"{pre}.{long}", f"L{l}.{short}") for l, pre in enumerate(LAYERS)
          for long, short in (("ln_self_attn", "ln_self"), ("ln_src_attn", "ln_src"), ("ln_ffnetwork", "ln_ffn")) if l or short != "ln_src"])
HOWS = [(n, how) for k, n in enumerate(NORMS) for how in (("gamma", "beta", "nan") if k % 5 == 0 else ("gamma",))]   # all 16 norms


@pytest.mark.parametrize("which,key,name,how", [n + (how,) for n, how in HOWS], ids=[f"{n[2]}-{how}" for n, how in HOWS])
def test_split_create_refuses_a_norm_beyond_the_f16_range(which, key, name, how):
    """16 |gamma| + |beta| >= 65504 in ONE channel of a norm whose output the split path converts to f16 unscaled: vapx_create refuses by
    name under VAPX_FLAG_SPLIT_F16 and accepts on the fp32 path.  No kernel runs."""
    from vap_realtime_amd import engine, weights as W
    cpc, vap = (dict(d) for d in W.synthetic_weights(SEED, 20, "vap"))
    sd = cpc if which == "cpc" else vap
    field = key + (".bias" if how == "beta" else ".weight")
    t = sd[field].copy()
    t.reshape(-1)[137] = {"gamma": -4094.0, "beta": 65504.0, "nan": np.nan}[how]      # 16 x 4094 = 65504; the bias alone; not finite
    sd[field] = t
    blob = W.pack_blob(cpc, vap, "vap")
    with pytest.raises(engine.VapxError, match=rf"VAPX_FLAG_SPLIT_F16: the norm {name} has 16 \|gamma\| \+ \|beta\| .* in channel 137"):
        engine.Engine(blob, 20, 1.0, max_streams=1, split_f16=True)
    if how != "nan":
        engine.Engine(blob, 20, 1.0, max_streams=1).close()


def test_split_create_accepts_the_largest_bound_below_and_the_gains_regime():
    from vap_realtime_amd import engine, weights as W
    cpc, vap = (dict(d) for d in W.synthetic_weights(SEED, 20, "vap"))
    t = cpc["gEncoder.batchNorm4.weight"].copy()
    t.reshape(-1)[5] = 4000.0                                # 64000 + |beta| < 65504
    cpc["gEncoder.batchNorm4.weight"] = t
    engine.Engine(W.pack_blob(cpc, vap, "vap"), 20, 1.0, max_streams=1, split_f16=True).close()
    cpc, vap = WR.weights("gains", SEED, 20)
    assert 100.0 < WR.norm_bound(cpc, vap) <= 138.0
    engine.Engine(W.pack_blob(cpc, vap, "vap"), 20, 1.0, max_streams=1, split_f16=True).close()
