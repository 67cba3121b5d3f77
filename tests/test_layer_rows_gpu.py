"""Every valid row of every transformer layer of the HIP path against the float64 oracle, per window class.

The step's outputs see the window through the newest row of the last layer; older rows of layers 0-2 reach them only through
attention weights, so a kernel that is wrong on some rows can pass the output parity tests.  Here ``o``, ``stereo0`` and
``stereo1`` (and ``stereo2`` where the engine materialises it: ``full_last_layer`` and nod) are peeked and every row t < n of
every stream is held against the float64 oracle with the bound of tests/layer_rows.py (8 x the torch fp32 oracle's own error
on that buffer).  One window per attention dispatch class and edge:

    T = 50   attn_block_kernel (fused short-window block)
    T = 65   first long window: attention_long2_kernel / attention_f16x3_kernel with a 1-row last tile
    T = 100, 250 (C3), 256 (8 full key tiles, the last T before the XL kernel)
    T = 257  first attention_xl_kernel window, T = 512 its limit

Each case steps 3 dialogues in 5 stream slots (permuted ids, one dialogue joins late, so one step mixes valid lengths inside a
32-row tile) through the filling window (n = 1, 2, 31, 32, 33, T - 1, T) and slid states whose ring rotation is not a multiple
of 32; some engines run with VAPX_POISON_SCRATCH, so any read of a padding row or an unwritten ring slot turns a valid row into
NaN.  The worst err / E32 per buffer is printed (run with -s)."""
import os

import numpy as np
import pytest

from layer_rows import check_rows

pytestmark = pytest.mark.gpu

WINDOWS = [(20, 2.5, 50), (50, 1.3, 65), (20, 5.0, 100), (50, 5.0, 250), (50, 5.12, 256), (50, 5.14, 257), (50, 10.24, 512)]
LATE = 7                     # first frame of the late dialogue: its ring rotation differs from the others' by 7


def checkpoints(T):
    return sorted({1, 2, 31, 32, 33, T - 1, T, T + 1, T + 37, 2 * T + 5})


class Variant:
    """One engine configuration: Engine(...) keyword flags, plus the two debug knobs vapx_create reads from the environment."""
    def __init__(self, label, poison=False, force_xl=False, **kw):
        self.label, self.poison, self.force_xl, self.kw = label, poison, force_xl, kw

    def buffers(self, mode):
        return ("o", "stereo0", "stereo1") + (("stereo2",) if self.kw.get("full_last_layer") or mode == "nod" else ())


def base_variants(T):
    v = [Variant("fp32"), Variant("fp32_full", poison=True, full_last_layer=True),
         Variant("split", poison=True, split_f16=True), Variant("split_full", split_f16=True, full_last_layer=True)]
    if T in (65, 256):       # the XL kernel on windows the tuned kernel also takes: a 1-row last tile, 8 full tiles
        v.append(Variant("fp32_force_xl", poison=True, force_xl=True))
    if T == 250:
        v += [Variant("unfused_proj", unfused_proj=True), Variant("split_unfused_proj", poison=True, split_f16=True, unfused_proj=True),
              Variant("split_qkv_in_ffn", split_f16=True, split_qkv_in_ffn=True)]
    return v


def make_engine(blob, hz, ctx, slots, var, mode):
    from vap_realtime_amd import engine
    env = {"VAPX_POISON_SCRATCH": var.poison, "VAPX_FORCE_ATTENTION_XL": var.force_xl}
    saved = {k: os.environ.pop(k, None) for k in env}
    try:
        for k, on in env.items():
            if on:
                os.environ[k] = "1"                  # read by vapx_create, once per engine
        return engine.Engine(blob, hz, ctx, max_streams=slots, mode=mode, **var.kw)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(hz, ctx, T, variants, *, seed=23, mode="vap", cohorts=(2, 1), slots=5, label=""):
    """cohorts: dialogues starting at frame 0 and at frame LATE; each cohort steps one batched float64 and one fp32
    oracle.  The engine batch interleaves the cohorts in a fixed shuffled order over a permuted slot assignment."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth, weights as W
    cpc, vap = W.synthetic_weights(seed, hz, mode)
    blob = W.pack_blob(cpc, vap, mode)
    hop = 16000 // hz
    cps = checkpoints(T)
    F_ = cps[-1]
    starts = (0, LATE)
    rng = np.random.default_rng(seed + T)
    D = sum(cohorts)
    coh = np.repeat(np.arange(len(cohorts)), cohorts)                     # cohort of each dialogue
    pos = np.concatenate([np.arange(c) for c in cohorts])                 # index inside its cohort
    order = rng.permutation(D)                                            # batch order of the dialogues
    slot = rng.permutation(slots)[:D].astype(np.int32)                    # stream slot of each dialogue
    audio = [synth.dialogue_batch(list(range(100 * k + seed, 100 * k + seed + c)), hop * (F_ - starts[k]))
             for k, c in enumerate(cohorts)]
    o64 = VapOracle(cpc, vap, hz, ctx, mode=mode, dtype=torch.float64)
    o32 = VapOracle(cpc, vap, hz, ctx, mode=mode)
    st64 = [o64.new_state(c) for c in cohorts]
    st32 = [o32.new_state(c) for c in cohorts]
    fr = [ServerFramer(c, hop) for c in cohorts]
    engines = [make_engine(blob, hz, ctx, slots, v, mode) for v in variants]
    for e in engines:
        assert e.T == T, (hz, ctx, e.T, T)
    worst = {(v.label, b): 0.0 for v in variants for b in v.buffers(mode)}
    try:
        for f in range(F_):
            live = [d for d in order if f >= starts[coh[d]]]
            new = np.stack([audio[coh[d]][pos[d], :, (f - starts[coh[d]]) * hop:(f - starts[coh[d]] + 1) * hop] for d in live])
            ids = slot[live]
            for e in engines:
                e.step(new, ids)
            for k in range(len(cohorts)):
                if f >= starts[k]:
                    frame = fr[k].frame(audio[k][:, :, (f - starts[k]) * hop:(f - starts[k] + 1) * hop])
                    o64.advance(frame, st64[k])
                    o32.advance(frame, st32[k])
            if f + 1 not in cps:
                continue
            ref64 = {k: o64.layers(st64[k]) for k in range(len(cohorts)) if f >= starts[k]}
            ref32 = {k: o32.layers(st32[k]) for k in range(len(cohorts)) if f >= starts[k]}
            ns = [min(f + 1 - starts[coh[d]], T) for d in live]
            for v, e in zip(variants, engines):
                for b in v.buffers(mode):
                    got = e.peek(b, (len(live), 2, T, 256))
                    r = check_rows(b, got, ns, [ref64[coh[d]][b][pos[d]] for d in live], [ref32[coh[d]][b][pos[d]] for d in live],
                                   streams=[f"{d} (slot {slot[d]})" for d in live],
                                   what=f"{label} T={T} {v.label} frame {f + 1}")
                    worst[(v.label, b)] = max(worst[(v.label, b)], r)
    finally:
        for e in engines:
            e.close()
    for v in variants:
        print(f"{label} T={T} {v.label}: worst err/E32", {b: round(worst[(v.label, b)], 2) for b in v.buffers(mode)})
    return worst


@pytest.mark.parametrize("hz,ctx,T", WINDOWS, ids=[f"T{w[2]}" for w in WINDOWS])
def test_layer_rows_against_float64(hz, ctx, T):
    """fp32 and split_f16, each pruned (default) and full last layer; T = 250 adds the unfused projections (both precisions)
    and split_qkv_in_ffn, T = 65 / 256 the forced XL kernel."""
    run_case(hz, ctx, T, base_variants(T), label="vap")


def test_layer_rows_nod_long_window():
    """nod materialises stereo2 (its p_bc reads every row of the last layer) on the default path."""
    run_case(10, 10.0, 100, [Variant("nod_fp32", poison=True), Variant("nod_split", split_f16=True)],
             seed=17, mode="nod", label="nod")


def test_layer_rows_with_overlap_groups():
    """groups = 2 splits a batch of >= 64 streams over two HIP streams (each group's scratch slice is contiguous, so one peek
    sees both); 68 dialogues in 72 slots, 4 of them joining late."""
    run_case(50, 1.3, 65, [Variant("fp32_groups2", poison=True, groups=2), Variant("split_groups2", split_f16=True, groups=2)],
             seed=29, cohorts=(64, 4), slots=72, label="groups")
