"""The tail of the step on the HIP path against the float64 oracle, per dispatch class: the newest row of the last stereo layer, the
combinator, vap_head, the VAD and the bc / nod heads.

The encoder (tests/test_encoder_stages_gpu.py) and every row of layers 0-2 (tests/test_layer_rows_gpu.py) are held against float64;
what comes after them was seen only through the outputs, at 1e-4 against goldens or at 2e-5 against the engine's own unfused variant.
Here ``last`` (``peek("last")``, or row n - 1 of ``stereo2`` where the whole layer runs), ``comb`` (nod), ``logits``, ``vad_logit``,
``p_now``, ``p_future``, ``vad``, every ``aux`` column and the ``p_bc_rows`` of nod are held to the bound of tests/head_stages.py
(8 x max(pooled fp32-oracle error, 1e-6 max|x|)); p_now / p_future / vad are also recomputed in float64 from the engine's OWN logits
and vad_logit and held to 8e-6 max|p| (the device's softmax, aggregation and sigmoid alone); n, status, the reserved slots, the
undefined aux slots and the ``e`` copy are compared exactly.

Classes, and the dispatches each one reaches:

    paths x modes, 20 Hz, T = 20, 3 dialogues in 7 slots (M = 6: a partial last_block_kernel<8> tile; head_kernel<2> with an odd tail)
        vap, bc   default (last_block_kernel), unfused_last_row (gather_last_ln_kernel, attention_last_kernel, M = 2B GEMMs),
                  full_last_layer (head_kernel reads stereo2 with x_last_only = 0), split_f16, split_f16 + unfused_last_row
        nod       fp32 and split_f16: x_last_only = 0, run_combinator_all_rows, pbc_rows_kernel
        checkpoints n = 1 (last_block_kernel's empty key parity), 2, 3, 7, 8, 9 (its ragged 8-key groups), T - 1, T, and slid T + 1, T + 7
    key-count edges, 50 Hz, T = 130: fused, unfused_last_row, split_f16 at n = 63, 64, 65, 127, 128, 129, 130 and slid 131, 137:
        attention_last_kernel's 64-key chunk boundary and cross-chunk rescale at n = 64 / 65 / 128 / 129; the late dialogue sits at
        n - 2 in the same tile
    batch tile edges, vap fp32, T = 20
        B = 1, 5          last_block_kernel<8> partial tiles (M = 2, 10), head_kernel<2> odd tail
        B = 1024          the last batch of last_block_kernel<8> / head_kernel<2>
        B = 1025 .. 1027  last_block_kernel<16> with a 2-, 4-, 6-row last tile; head_kernel<4> with tails 1, 2, 3
        B = 1027          also split_f16, bc, and groups = 2 (two scratch slices of 513 / 514 streams, one ``last`` peek over both)
        B = 1025          also nod: run_combinator_all_rows and pbc_rows_kernel over 1025 x T rows, head_kernel<4> with x_last_only = 0
    trunk followers: vap leading bc and nod, fp32 and split_f16: every engine's heads against the oracle of ITS weights, bn from the leader

Dialogues carry the amplitudes 1e-3 x, 1 x, 30 x; slot ids are permuted inside a larger table; in the small cases one dialogue joins
late, so one tile mixes window fills.  Where a case needs hundreds of streams, 4 distinct dialogues are tiled over the slots (the
oracles run 4 streams, every copy is checked).  Some engines run with VAPX_POISON_SCRATCH.

Worst err / E32 and worst err / bound over all classes, measured on an MI355X (printed per class and engine with -s).  E32 is pooled
over the tick's streams and sits below FLOOR = 1e-6 of max|x| on most stages, so err / E32 may pass 8 (aux, p_now: probabilities near
1 whose fp32-oracle error is a single ulp) while err / bound, the figure that is asserted, cannot pass 1.  "own": against float64
softmax / aggregation / sigmoid of the engine's own logits and vad_logit, bound 8e-6 max|p|.

                    fp32                    split_f16
    stage           err/E32   err/bound     err/E32   err/bound
    last            2.98      0.28          2.60      0.22
    comb            3.76      0.29          2.24      0.22
    logits          3.44      0.22          2.71      0.15
    vad_logit       5.36      0.63          5.07      0.63
    p_now           5.62      0.09          11.88     0.10
    p_future        9.09      0.07          3.72      0.07
    vad             7.76      0.76          7.19      0.82
    aux             12.05     0.35          12.05     0.17
    p_bc_rows       4.27      0.43          2.08      0.19
    own p_now       -         0.02          -         0.02
    own p_future    -         0.02          -         0.02
    own vad         -         0.01          -         0.01

So __expf and the absorbed Wk / deferred Wv of last_block_kernel, its key-parity merge and n = 1 case, the online softmax of
attention_last_kernel across chunks, gelu_fast and the block reductions of head_kernel all stay within 0.3 of the bound on ``last`` /
``comb`` / ``logits``; the VAD (a 256-term dot product of ``o``, whose own error the bound of 2 numbers per stream barely covers) comes
closest with 0.82.  No stage's factor is raised, and no kernel had to change.

Tried by hand with three faults planted in a scratch build (not committed): last_block_kernel's attention dropping key 0 once the
window holds two rows, head_kernel's aux softmax running over 4 rows in bc mode, pbc_rows_kernel taking the newest row's p_bc from
row n - 2.  16 of the 17 tests here fail (the peek refusals pass).  Every engine on the fused block fails at tick 2 as ``last
(last_block_kernel)`` at 3.5e3 - 1.2e4 x the bound, at B = 1, 5, 1024 .. 1027, with groups = 2, fp32 and split, and at tick 63 of the
T = 130 case, while the unfused_last_row and full_last_layer engines of the same cases pass ``last``; every bc engine fails at tick 1
on the exact field (aux column 3 of a bc engine holds 0.43); every nod engine, the 1025-stream one and the trunk follower included,
fails at tick 2 as ``p_bc_rows (pbc_rows_kernel)``, index 1 of 2, at 9e2 - 1e4 x the bound.  These three are coarse: the golden parity
test and test_fused_last_row_block_equals_the_ten_launch_path fail with that build too; what they show is that each stage names its
own kernel and that every dispatch class above reaches the faulty code.

What tests/test_head_stages.py shows on the CPU about the 1e-4 output bar: of the seeded faults that the stage bound rejects, one stays
under 1e-4 on every output (``last_slice_rel_small``: one wave's 32 output columns of the newest row of the last layer off by 3e-5
relative: outputs move 6.2e-5, rejected at ``last`` with 2.4 x); the 1e-4 slice faults of ``last``, the combinator and vap_head move the
logits by 2.1e-4 .. 4.8e-4, every other fault by 5e-3 and more: most of what this file checks the output bar would see too, given an
input that exercises the branch, and the point of the classes above is that they do exercise it.  Two faults neither check separates:
tanh-GELU in the last-row FFN (0.7 - 1.3 x the bound of ``last``, outputs 4e-5) and a combinator LayerNorm epsilon of 1e-4 (nothing
moves: the variance of the combinator's projections is in the hundreds).
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import head_stages as HS

pytestmark = pytest.mark.gpu

AMPS = (1e-3, 1.0, 30.0)
LATE = 2                                             # first tick of the late dialogue
SMALL_CP = (1, 2, 3, 7, 8, 9, 19, 20, 21, 27)        # T = 20
EDGE_CP = (63, 64, 65, 127, 128, 129, 130, 131, 137)  # T = 130
TOTAL: dict = {}                                     # (precision, stage) -> [worst err / E32, worst err / bound] over the session


@contextmanager
def debug_env(poison):
    """VAPX_POISON_SCRATCH is read by vapx_create, once per engine."""
    saved = os.environ.pop("VAPX_POISON_SCRATCH", None)
    if poison:
        os.environ["VAPX_POISON_SCRATCH"] = "1"
    try:
        yield
    finally:
        os.environ.pop("VAPX_POISON_SCRATCH", None)
        if saved is not None:
            os.environ["VAPX_POISON_SCRATCH"] = saved


class Variant:
    """One engine of a case.  ``path``: "fused" / "unfused" / "full" (head_stages.kernel_of), "_split" appended on the split path."""

    def __init__(self, label, mode="vap", path="fused", poison=False, **kw):
        self.label, self.mode, self.path, self.poison, self.kw = label, mode, path, poison, kw
        self.worst, self.excess = {}, {}


def small_variants(mode):
    if mode == "nod":
        return [Variant("nod_fp32", "nod", "full", poison=True), Variant("nod_split", "nod", "full_split", split_f16=True)]
    return [Variant(f"{mode}_fused", mode, "fused", poison=True),
            Variant(f"{mode}_unfused_last_row", mode, "unfused", unfused_last_row=True),
            Variant(f"{mode}_full_last_layer", mode, "full", full_last_layer=True),
            Variant(f"{mode}_split", mode, "fused_split", poison=True, split_f16=True),
            Variant(f"{mode}_split_unfused_last_row", mode, "unfused_split", split_f16=True, unfused_last_row=True)]


class Dialogue:
    """One dialogue's latest frame and oracle results: ``new`` [2, hop], ``r64`` / ``r32`` = {oracle key: head_stages.row_of}."""

    def __init__(self, start):
        self.start, self.new, self.r64, self.r32 = start, None, {}, {}


class Cast:
    """The dialogues of a case on the CPU.  Dialogues that start on the same tick share one oracle call per tick (S > 1), which is
    what keeps a 137-tick case at a few seconds; per oracle key the float64 and the fp32 oracle keep their own state."""

    def __init__(self, oracles, audio, hop, starts, pre_hook=None):
        from oracle.vap_oracle import ServerFramer
        self.oracles, self.audio, self.hop, self.pre_hook = oracles, audio, hop, pre_hook
        self.dlg = [Dialogue(s) for s in starts]
        self.troupes = []
        for s in sorted(set(starts)):
            idx = [k for k, x in enumerate(starts) if x == s]
            self.troupes.append({"start": s, "idx": idx, "pos": 0, "fr": ServerFramer(len(idx), hop),
                                 "state": {k: (o64.new_state(len(idx)), o32.new_state(len(idx))) for k, (o64, o32) in oracles.items()}})

    def step(self, f, full):
        """Advance every dialogue that has started by one frame; ``full``: also run the transformer and the heads (a checkpoint)."""
        for tr in self.troupes:
            if f < tr["start"]:
                continue
            new = self.audio[tr["idx"]][:, :, tr["pos"] * self.hop:(tr["pos"] + 1) * self.hop]
            frame = tr["fr"].frame(new)
            tr["pos"] += 1
            for j, d in enumerate(tr["idx"]):
                self.dlg[d].new = new[j]
            for k, (o64, o32) in self.oracles.items():
                s64, s32 = tr["state"][k]
                if not full:
                    o64.advance(frame, s64)
                    o32.advance(frame, s32)
                    continue
                pre = {} if self.pre_hook else None
                r64, r32 = HS.collect_heads(o64, frame, s64, pre), HS.collect_heads(o32, frame, s32)
                if pre is not None:                          # the inputs of the float64 oracle's non-linearities at this checkpoint
                    self.pre_hook(pre)
                for j, d in enumerate(tr["idx"]):
                    self.dlg[d].r64[k], self.dlg[d].r32[k] = HS.row_of(r64, j), HS.row_of(r32, j)


def oracle_pair(cpc, vap, hz, T, mode):
    import torch
    from oracle.vap_oracle import VapOracle
    ctx = (T + 0.5) / hz
    o64, o32 = VapOracle(cpc, vap, hz, ctx, mode=mode, dtype=torch.float64), VapOracle(cpc, vap, hz, ctx, mode=mode)
    assert o64.T == T == o32.T
    return o64, o32


def make_cast(oracles, hz, n, frames, seed, late, pre_hook=None):
    from vap_realtime_amd import synth
    hop = 16000 // hz
    audio = synth.dialogue_batch([seed + 100 * k for k in range(n)], hop * frames)
    audio = audio * np.asarray([AMPS[k % len(AMPS)] for k in range(n)], np.float32)[:, None, None]
    return Cast(oracles, audio, hop, [LATE if late and n > 1 and k == n - 1 else 0 for k in range(n)], pre_hook)


def check_engine(eng, var, key, out, batch, dlg, slot, T, what, propagate=False):
    """Every stage and every exact field of one engine after a step of ``batch`` = [(dialogue index, copy index)]."""
    from vap_realtime_amd import engine
    B, mode = len(batch), var.mode
    assert out.shape == (B, engine.OUT_STRIDE)
    o = engine.split_outputs(out)
    w64, w32 = [dlg[d].r64[key] for d, _ in batch], [dlg[d].r32[key] for d, _ in batch]
    ns = [w["n"] for w in w64]
    names = [f"{i} (dialogue {d}, slot {slot[i]}, batch row {r}, n = {ns[r]})" for r, (d, i) in enumerate(batch)]
    HS.check_exact(mode, out, ns, eng.peek("e", (B, 2, 256)), T, streams=names, what=what)
    if var.path.startswith("full"):
        s2 = eng.peek("stereo2", (B, 2, T, 256))
        last = np.stack([s2[r, :, ns[r] - 1] for r in range(B)])
    else:
        last = eng.peek("last", (B, 2, 256))
    comb = eng.peek("comb", (B, T, 256)) if mode == "nod" else None
    got = []
    for r in range(B):
        row = {"last": last[r], "vad_logit": o["vad_logit"][r], "p_now": o["p_now"][r], "p_future": o["p_future"][r], "vad": o["vad"][r]}
        if mode == "nod":
            row["comb"], row["p_bc_rows"] = comb[r, :ns[r]], out[r, engine.OUT_LOGITS:engine.OUT_LOGITS + ns[r]]
        else:
            row["logits"] = o["logits"][r]
        if mode != "vap":
            row["aux"] = o["aux"][r, :HS.AUX_COLS[mode]]
        got.append(row)
    HS.check_tick(mode, got, w64, w32, path=var.path, streams=names, what=what, worst=var.worst, excess=var.excess, propagate=propagate)
    HS.check_own(got, streams=names, what=what, excess=var.excess)


def run_case(hz, T, variants, *, label, seed=61, n_dialogues=3, copies=3, slots=7, frames=None, cps=SMALL_CP, late=True,
             engine_kw=None, group=None, weights=None, propagate=False, pre_hook=None):
    """Steps every engine variant and the oracles over ``frames`` ticks; ``copies`` engine streams tile the ``n_dialogues`` dialogues
    (copy i plays dialogue i % n_dialogues).  ``group``: {mode: vap state dict} of a TrunkGroup (the first leads); then ``variants``
    holds one entry per mode and they are the group's engines.  ``weights``: (cpc, vap) -> (cpc, vap), applied to the synthetic weights
    of every mode (tests/weight_regimes.py); ``propagate``: ``head_stages.check_tick``'s, for head weights scaled up; ``pre_hook``: called at
    every checkpoint with the inputs of the float64 oracle's non-linearities (``VapOracle._collect_pre``), so that a case can assert what it reached."""
    from vap_realtime_amd import engine, weights as W
    frames = max(cps) if frames is None else frames
    modes = list(group) if group else sorted({v.mode for v in variants})
    cpc = W.synthetic_weights(seed, hz, "vap")[0]
    sd = group or {m: W.synthetic_weights(seed, hz, m)[1] for m in modes}
    if weights is not None:
        sd = {m: weights(cpc, v)[1] for m, v in sd.items()}
        cpc = weights(cpc, sd[modes[0]])[0]
    oracles = {m: oracle_pair(cpc, sd[m], hz, T, m) for m in modes}
    blobs = {m: W.pack_blob(cpc, sd[m], m) for m in modes}
    import torch
    torch.set_num_threads(min(4, torch.get_num_threads()))     # the oracles' per-tick tensors are small
    cast = make_cast(oracles, hz, n_dialogues, frames, seed, late, pre_hook)
    dlg = cast.dlg
    owner = [i % n_dialogues for i in range(copies)]
    rng = np.random.default_rng(seed + hz + copies)
    slot = rng.permutation(slots)[:copies].astype(np.int32)
    order = list(rng.permutation(copies))
    ctx = (T + 0.5) / hz
    grp, engines = None, []
    if group:
        with debug_env(variants[0].poison):
            grp = engine.TrunkGroup(blobs, hz, ctx, max_streams=slots, max_batch=copies, **dict(engine_kw or {}))
        engines = [grp.engines[v.mode] for v in variants]
    else:
        for v in variants:
            with debug_env(v.poison):
                engines.append(engine.Engine(blobs[v.mode], hz, ctx, max_streams=slots, max_batch=copies, mode=v.mode,
                                             **dict(engine_kw or {}, **v.kw)))
    assert all(e.T == T for e in engines)
    failed = {}
    try:
        for f in range(frames):
            full = f + 1 in cps
            batch = [(owner[i], i) for i in order if f >= dlg[owner[i]].start]
            cast.step(f, full)
            new = np.stack([dlg[d].new for d, _ in batch])
            ids = slot[[i for _, i in batch]]
            if grp:
                outs = grp.step(new, ids)
                outs = [outs[v.mode] for v in variants]
            else:
                outs = [e.step(new, ids) for e in engines]
            if not full:
                continue
            for v, e, out in zip(variants, engines, outs):
                if v.label in failed:
                    continue
                try:                                         # one variant's first failure does not hide the other variants'
                    check_engine(e, v, v.mode, out, batch, dlg, slot, T, f"{label} {hz} Hz {v.label} tick {f + 1} (B = {len(batch)})",
                                 propagate)
                except AssertionError as ex:
                    failed[v.label] = str(ex)
    finally:
        if grp:
            grp.close()
        else:
            for e in engines:
                e.close()
    for v in variants:
        print(f"{label} {hz} Hz {v.label}: worst err/E32", {st: round(r, 2) for st, r in v.worst.items()},
              "worst err/bound", {st: round(r, 2) for st, r in v.excess.items()})
        prec = "split" if "split" in v.path or (engine_kw or {}).get("split_f16") else "fp32"
        for st, r in v.excess.items():
            t = TOTAL.setdefault((prec, st), [0.0, 0.0])
            t[0], t[1] = max(t[0], v.worst.get(st, 0.0)), max(t[1], r)
    print("so far:", {f"{p} {st}": (round(a, 2), round(b, 2)) for (p, st), (a, b) in sorted(TOTAL.items())})
    assert not failed, "\n".join(failed.values())
    for v in variants:                                       # every stage the mode has was looked at
        assert set(v.worst) == set(HS.stages_of(v.mode)), (v.label, sorted(v.worst))


@pytest.mark.parametrize("mode", ["vap", "bc", "nod"])
def test_paths_and_modes_small_batch(mode):
    """default / unfused_last_row / full_last_layer / split_f16 / split_f16 + unfused_last_row (nod: fp32, split_f16) at n = 1, 2, 3, 7, 8,
    9, T - 1, T and slid T + 1, T + 7; the late dialogue is two rows behind in the same last_block_kernel<8> tile."""
    run_case(20, 20, small_variants(mode), label="small")


def test_key_count_edges_t130():
    """attention_last_kernel's 64-key chunks (n = 63 .. 65, 127 .. 129: boundary and cross-chunk rescale) and last_block_kernel's ragged
    8-key groups, fp32 fused / unfused_last_row and split_f16, one 50 Hz window of 130 frames that fills and slides."""
    run_case(50, 130, [Variant("fused", poison=True), Variant("unfused_last_row", path="unfused", unfused_last_row=True),
                       Variant("split", path="fused_split", split_f16=True)], label="edges", seed=67, cps=EDGE_CP)


TILE_CASES = [
    pytest.param(1, "vap", {}, id="B1-last_block8_M2-head2_odd_tail"),
    pytest.param(5, "vap", {}, id="B5-last_block8_M10-head2_odd_tail"),
    pytest.param(1024, "vap", {}, id="B1024-last_block8_last_batch-head2_last_batch"),
    pytest.param(1025, "vap", {}, id="B1025-last_block16_tail2-head4_tail1"),
    pytest.param(1026, "vap", {}, id="B1026-last_block16_tail4-head4_tail2"),
    pytest.param(1027, "vap", {}, id="B1027-last_block16_tail6-head4_tail3"),
    pytest.param(1027, "vap", {"split_f16": True}, id="B1027-split_f16"),
    pytest.param(1027, "bc", {}, id="B1027-bc"),
    pytest.param(1025, "nod", {}, id="B1025-nod-run_combinator_all_rows-pbc_rows_kernel-head4_x_last_only0"),
    pytest.param(1027, "vap", {"groups": 2}, id="B1027-groups2-last_peeked_across_both_slices"),
]


@pytest.mark.parametrize("B,mode,kw", TILE_CASES)
def test_batch_tile_edges(B, mode, kw):
    """4 distinct dialogues tiled over B slots, 4 ticks, checked at n = 1, 2 and 4 (T = 20)."""
    path = ("full" if mode == "nod" else "fused") + ("_split" if kw.get("split_f16") else "")
    run_case(20, 20, [Variant(f"{mode}_B{B}", mode, path, poison=B <= 1025, **kw)], label="tiles", seed=71,
             n_dialogues=min(B, 4), copies=B, slots=B + 3, cps=(1, 2, 4), late=False)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split_f16"])
def test_trunk_followers_heads(split):
    """Leader vap, followers bc and nod on one CPC weight set; the followers' own weights are drawn with other seeds.  Window fill and
    ring slot (bn) come from the leader's conv0; every engine is held against the oracle of its own weights."""
    from vap_realtime_amd import weights as W
    seed, hz = 73, 20
    sd = {"vap": W.synthetic_weights(seed, hz, "vap")[1]}
    sd.update({m: W.synthetic_weights(seed + 1 + k, hz, m)[1] for k, m in enumerate(("bc", "nod"))})
    sfx = "_split" if split else ""
    variants = [Variant("leader_vap", "vap", "fused" + sfx, poison=True), Variant("follower_bc", "bc", "fused" + sfx),
                Variant("follower_nod", "nod", "full" + sfx)]
    run_case(hz, 20, variants, label="trunk", seed=seed, cps=(1, 2, 3, 8, 9, 20, 23), group=sd, engine_kw={"split_f16": split})


def test_peek_last_and_comb_refuse_by_name():
    from vap_realtime_amd import engine, synth, weights as W
    hz, T = 20, 20
    audio = synth.dialogue_batch([1, 2], 800)
    for mode, kw, refused, word in (("vap", {}, "comb", "only materialised in nod mode"), ("vap", {}, "stereo2", "VAPX_FLAG_FULL_LAST_LAYER"),
                                    ("vap", {"full_last_layer": True}, "last", "peek \"stereo2\" and take row n - 1"),
                                    ("nod", {}, "last", "peek \"stereo2\" and take row n - 1")):
        cpc, vap = W.synthetic_weights(5, hz, mode)
        eng = engine.Engine(W.pack_blob(cpc, vap, mode), hz, 1.0, max_streams=2, mode=mode, **kw)
        try:
            eng.step(audio)
            with pytest.raises(engine.VapxError, match=word):
                eng.peek(refused, (2, 2, 256))
        finally:
            eng.close()
    cpc, vap = W.synthetic_weights(5, hz, "nod")                 # two overlap groups: comb's slices are not contiguous
    eng = engine.Engine(W.pack_blob(cpc, vap, "nod"), hz, 1.0, max_streams=64, mode="nod", groups=2)
    try:
        eng.step(np.tile(audio, (32, 1, 1)))
        with pytest.raises(engine.VapxError, match="not contiguous when the latest step ran in 2 overlap groups"):
            eng.peek("comb", (64, T, 256))
        eng.step(audio)                                          # 2 streams: one group
        assert np.isfinite(eng.peek("comb", (2, T, 256))[:, :2]).all()
    finally:
        eng.close()
