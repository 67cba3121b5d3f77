"""vapx_prefill in the dispatch classes production engines use, against the float64 oracle: the cases, their plan, the truth and the checker.

tests/test_prefill_gpu.py runs prefill on engines of max_batch 8 and 11: chunks of one to three frames, every GEMM in the 32-row tile, the
fused conv tail on every fp32 chunk, and equality with a stepped twin as the one strong assertion.  A serving engine has max_batch in the
hundreds or thousands and attaches a few callers at a time: the call is ONE chunk of hundreds of (frame, stream) entries.  Then conv1 runs
in 64- or 128-row tiles, the conv chain leaves the fused tail past 512 entries, the chunk is longer than the window (the in-kernel skip of
ring_append_kernel decides what lands), and one LSTM launch walks hundreds of frames.  ``CASES`` reaches each of these; ``plan`` asks the
library's own tile rule (``vapx_gemm_tile_rows``) for every GEMM of every chunk and asserts that each case reaches what it is here for.

The truth is ``VapOracle(dtype=float64)`` driven by ``ServerFramer``, one dialogue at a time (S = 1), next to the torch fp32 oracle on the
same frames; a few distinct dialogues are tiled over a call's streams in shuffled slot order and every replica is held against its
dialogue.  The bound is ``encoder_stages.stage_bound`` unchanged: FACTOR x max(E32, FLOOR x max|x|) per stream block, E32 the fp32
oracle's own error on that block after the same frames.  ``run_case`` is the whole checker; tests/test_prefill_classes_gpu.py runs it on
engines, tests/test_prefill_classes.py on a stand-in backed by an oracle (``StandIn``), with and without seeded faults.

Windows are short on purpose (T = 12 at 20 Hz, 20 at 50 Hz, 8 at 10 Hz, 4 at 5 Hz): a large max_batch then costs little scratch and
every long chunk is also longer than the window."""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import encoder_stages as ES

T_OF = {20: 12, 50: 20, 10: 8, 5: 4}
WEIGHT_SEED = 29
AUDIO_SEEDS = (70, 71, 72)
CONT = 3                                   # ordinary steps after each case
TOL_OUT = 1e-4                             # tests/test_engine_gpu.py: the step's output rows against the oracle
EPI_STORE, EPI_CN_RELU = 0, 4              # gemm_f32.h
FUSED_MAX = 512                            # run_conv_chain: the fused conv tail serves up to 512 entries
PEEKABLE = ("h0", "h1", "h2", "h3", "z", "e")
REFUSED = ("lstm_out", "o", "stereo0", "stereo1", "last")


class Case(NamedTuple):
    id: str
    hz: int
    n: int                                 # streams of the call
    distinct: int                          # dialogues tiled over them
    max_batch: int
    program: Tuple[Tuple[str, int], ...]   # ("step", frames) | ("prefill", frames)
    paths: Tuple[str, ...]                 # "fp32" | "split"
    routes: Tuple[str, ...]                # "device" | "pageable"
    must: Dict[str, frozenset]             # path -> what plan() has to find

    @property
    def T(self):
        return T_OF[self.hz]

    @property
    def hop(self):
        return 16000 // self.hz

    @property
    def ctx_sec(self):
        return (self.T + 0.5) / self.hz

    @property
    def frames(self):
        return sum(k for _, k in self.program)


def _must(fp32=(), split=None):
    d = {"fp32": frozenset(fp32)}
    if split is not None:
        d["split"] = frozenset(split)
    return d


# The table of the issue.  A and C on the split path are its case D.  V (entries per chunk) follows from floor(max_batch / n): H's two calls
# of 200 and 150 frames of three streams are chunks of 600 entries (GEMM chain) and 450 (fused tail).
CASES = {c.id: c for c in (
    Case("A", 20, 1, 1, 512, (("prefill", 300),), ("fp32", "split"), ("device", "pageable"),
         _must({"fused_tail", "conv1_64", "fc>T", "lstm_walk>=1500", "ncpc_5"}, {"split_32", "split_64"})),
    Case("B", 20, 3, 3, 1024, (("prefill", 360),), ("fp32",), ("device",),
         _must({"chain", "conv1_64", "conv2_64", "conv3_64", "conv4_32", "gx_32", "fused_after_chain", "chunk_boundary", "fc>T"})),
    Case("C", 20, 8, 3, 1840, (("prefill", 230),), ("fp32", "split"), ("device", "pageable"),
         _must({"chain", "conv1_128", "conv2_64", "conv3_64", "conv4_64", "gx_128", "V==max_batch", "fc>T"},
               {"split_32", "split_64", "split_128", "V==max_batch"})),
    Case("E", 50, 1, 1, 512, (("prefill", 500),), ("fp32", "split"), ("device",),
         _must({"fused_tail", "conv1_64", "ncpc_2", "lstm_walk>=1000", "fc>T"}, {"split_64", "ncpc_2"})),
    Case("F", 10, 2, 2, 128, (("prefill", 64),), ("fp32", "split"), ("device", "pageable"),
         _must({"ncpc_10", "no_fused_tail_at_this_rate", "conv1_64", "fc>T"}, {"ncpc_10", "split_64"})),
    Case("G", 5, 1, 1, 64, (("prefill", 40),), ("fp32",), ("device",),
         _must({"ncpc_20", "no_fused_tail_at_this_rate", "conv1_64", "fc>T"})),
    Case("H", 20, 3, 3, 1024, (("step", 5), ("prefill", 200), ("prefill", 150)), ("fp32",), ("device",),
         _must({"nonempty_ring", "nonzero_bhead", "second_call", "fc>T", "chain", "fused_tail"})),
)}
# everything the set of cases has to reach, whatever case reaches it
MUST_REACH = frozenset({"fused_tail", "chain", "fused_after_chain", "chunk_boundary", "fc>T", "V==max_batch", "lstm_walk>=1500",
                        "conv1_64", "conv1_128", "conv2_64", "conv3_64", "conv4_32", "conv4_64", "gx_32", "gx_128",
                        "split_32", "split_64", "split_128", "ncpc_2", "ncpc_5", "ncpc_10", "ncpc_20", "no_fused_tail_at_this_rate",
                        "nonempty_ring", "nonzero_bhead", "second_call", "pageable_long_chunk"})


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
class Chunk(NamedTuple):
    f0: int                                # first frame, counted from the call's first
    fc: int
    fills: bool
    V: int
    fused: bool
    gemms: Dict[str, tuple]                # name -> (M, N, K, epi, tile rows the library picks)


class Call(NamedTuple):
    start: int                             # frames the streams have seen before the call
    frames: int
    chunks: List[Chunk]


class Plan(NamedTuple):
    calls: List[Call]
    reached: frozenset
    launches: List[Dict[str, int]]         # per call: what profile_read must say


def positions(hz: int) -> Dict[str, int]:
    geo = ES.geometry(hz)
    return {"P1": geo["h1"], "P2": geo["h2"], "P3": geo["h3"], "ncpc": geo["z"]}


def chunk_gemms(hz: int, V: int, fused: bool, fills: bool) -> Dict[str, tuple]:
    """Every GEMM run_conv_chain and vapx_prefill launch for a chunk of V entries: shapes from the encoder's geometry, the tile class from
    the library (nothing of the rule is restated here)."""
    from vap_realtime_amd import engine
    p = positions(hz)
    shapes = {"conv1": (V * 2 * p["P1"], 256, 2048, EPI_CN_RELU)}
    if not fused:
        shapes["conv2"] = (V * 2 * p["P2"], 256, 1024, EPI_CN_RELU)
        shapes["conv3"] = (V * 2 * p["P3"], 256, 1024, EPI_CN_RELU)
        shapes["conv4"] = (V * 2 * p["ncpc"], 256, 1024, EPI_CN_RELU)
    shapes["gx"] = (V * 2 * p["ncpc"], 1024, 256, EPI_STORE)
    if fills:
        shapes["qkv"] = (V * 2, 768, 256, EPI_STORE)
    return {k: s + (engine.gemm_tile_rows(*s),) for k, s in shapes.items()}


def plan(case: Case, path: str = "fp32", routes: Sequence[str] = ("device",), must: Optional[frozenset] = None) -> Plan:
    """The chunks of every prefill call of ``case`` as the engine walks them, the tile class of every GEMM (asked of the library), the
    launch counts per call, and the set of things reached.  Asserts ``case.must[path]`` (or ``must``) is among them."""
    from vap_realtime_amd import engine
    T, ncpc = case.T, positions(case.hz)["ncpc"]
    calls, launches, reached, seen = [], [], set(), 0
    for op, k in case.program:
        if op == "step":
            seen += k
            continue
        chunks = []
        for f0, fc, fills in engine.prefill_chunks(case.max_batch, case.n, k, T):
            V = case.n * fc
            assert V <= case.max_batch
            fused = case.hz in (50, 20) and path == "fp32" and V <= FUSED_MAX
            chunks.append(Chunk(f0, fc, fills, V, fused, chunk_gemms(case.hz, V, fused, fills)))
        calls.append(Call(seen, k, chunks))
        launches.append({"conv0": len(chunks), "lstm": len(chunks), "gather_ln": sum(c.fills for c in chunks),
                         "conv_tail": sum(c.fused for c in chunks), "gemm_cn_relu": sum(1 if c.fused else 4 for c in chunks),
                         "gemm_store": len(chunks) + sum(c.fills for c in chunks)})
        reached.add(f"ncpc_{ncpc}")
        if case.hz not in (50, 20):
            reached.add("no_fused_tail_at_this_rate")
        if seen:
            reached.add("nonempty_ring")
        if seen % T:
            reached.add("nonzero_bhead")
        if len(calls) > 1:
            reached.add("second_call")
        if len(chunks) > 1:
            reached.add("chunk_boundary")
        for i, c in enumerate(chunks):
            if path == "fp32":
                reached.add("fused_tail" if c.fused else "chain" if c.V > FUSED_MAX else "chain_by_rate")
                if c.fused and i and not chunks[i - 1].fused and chunks[i - 1].V > FUSED_MAX:
                    reached.add("fused_after_chain")
                reached.update(f"{name}_{g[4]}" for name, g in c.gemms.items())
            else:
                reached.update(f"split_{g[4]}" for g in c.gemms.values())
            if c.fc > T:
                reached.add("fc>T")
                if "pageable" in routes:
                    reached.add("pageable_long_chunk")
            if c.V == case.max_batch:
                reached.add("V==max_batch")
            reached.update(f"lstm_walk>={s}" for s in (1000, 1500) if c.fc * ncpc >= s)
        seen += k
    want = case.must.get(path, frozenset()) if must is None else must
    assert want <= reached, f"case {case.id} {path}: the plan does not reach {sorted(want - reached)}; it reaches {sorted(reached)}"
    return Plan(calls, frozenset(reached), launches)


def check_coverage(cases: Sequence[Case]) -> frozenset:
    """Every item of MUST_REACH is reached by some (case, path, route) of ``cases``."""
    reached = set()
    for c in cases:
        for path in c.paths:
            reached |= plan(c, path, c.routes).reached
    assert MUST_REACH <= reached, f"the cases do not reach {sorted(MUST_REACH - reached)}"
    return frozenset(reached)


def population(case: Case):
    """(slots [n], owner [n], max_streams): the call's streams in shuffled slots of a larger table, dialogue owner[k] on stream k."""
    rng = np.random.default_rng(1000 + sum(map(ord, case.id)) + case.n)
    max_streams = max(case.max_batch, case.n + 5)                                        # vapx_create: max_batch <= max_streams
    slots = rng.permutation(max_streams)[:case.n].astype(np.int32)
    owner = rng.permutation(np.arange(case.n) % case.distinct)
    return slots, owner, max_streams


# ---- the truth --------------------------------------------------------------------------------------------------------------------------
class Truth:
    """Both oracles over one rate's dialogues, S = 1 each, once for every case of that rate: ``snap[frames][d]`` the state after that many
    frames (ring, cache, h, c of both oracles, the latest frame), ``stages[(g, d)]`` = (float64, fp32) stage blocks of frame g where some
    case looks at them, ``cont[(g, d)]`` the float64 oracle's output rows of ``step`` at frame g."""

    def __init__(self, hz: int, cases: Sequence[Case], weights=None):
        import torch
        from oracle.vap_oracle import ServerFramer, VapOracle
        from vap_realtime_amd import synth, weights as W
        assert cases and all(c.hz == hz for c in cases)
        self.hz, self.T, self.hop = hz, T_OF[hz], 16000 // hz
        self.cpc, self.vap = weights or W.synthetic_weights(WEIGHT_SEED, hz, "vap")
        D = max(c.distinct for c in cases)
        total = max(c.frames for c in cases) + CONT
        self.audio = synth.dialogue_batch(list(AUDIO_SEEDS[:D]), self.hop * total)
        ctx = cases[0].ctx_sec
        self.o64, self.o32 = VapOracle(self.cpc, self.vap, hz, ctx, dtype=torch.float64), VapOracle(self.cpc, self.vap, hz, ctx)
        assert self.o64.T == self.T
        want_snap, want_stage, want_cont = {}, set(), set()
        for c in cases:
            seen = 0
            for i, (op, k) in enumerate(c.program):
                seen += k
                if op == "prefill":
                    want_snap.setdefault(seen, set()).update(range(c.distinct))
            last = plan(c, c.paths[0], must=frozenset()).calls[-1]
            f0 = last.start + last.chunks[-1].f0
            want_stage.update((g, d) for g in range(f0, f0 + last.chunks[-1].fc) for d in range(c.distinct))
            want_cont.update((g, d) for g in range(c.frames, c.frames + CONT) for d in range(c.distinct))
        self.snap: Dict[int, dict] = {f: {} for f in want_snap}
        self.stages: Dict[tuple, tuple] = {}
        self.cont: Dict[tuple, dict] = {}
        torch.set_num_threads(min(8, torch.get_num_threads()))
        for d in range(D):
            s64, s32, fr = self.o64.new_state(1), self.o32.new_state(1), ServerFramer(1, self.hop)
            for g in range(total):
                frame = fr.frame(self.audio[d:d + 1, :, g * self.hop:(g + 1) * self.hop])
                if (g, d) in want_cont:
                    out = self.o64.step(frame, s64.clone())
                    self.cont[(g, d)] = {k: out[k][0] for k in ("p_now", "p_future", "vad", "logits")}
                r64, r32 = ES.collect_stages(self.o64, frame, s64), ES.collect_stages(self.o32, frame, s32)
                for o, s, r in ((self.o64, s64, r64), (self.o32, s32, r32)):
                    s.ring = (s.ring + [torch.from_numpy(r["e"][:, :, 0]).to(o.dtype)])[-self.T:]
                if (g, d) in want_stage:
                    self.stages[(g, d)] = ({k: r64[k][0] for k in PEEKABLE}, {k: r32[k][0] for k in PEEKABLE})
                if d in want_snap.get(g + 1, ()):
                    self.snap[g + 1][d] = self._snapshot(s64, s32, frame[0])

    def _snapshot(self, s64, s32, frame):
        import torch
        snap = {"frame": frame.copy()}
        for tag, o, s in (("64", self.o64, s64), ("32", self.o32, s32)):
            with torch.no_grad():
                ring = torch.stack(s.ring, dim=2)                                          # [1, 2, n, 256] oldest -> newest
                v = o.v
                xn = torch.nn.functional.layer_norm(ring, (256,), v["ar_channel.layers.0.ln_self_attn.weight"],
                                                    v["ar_channel.layers.0.ln_self_attn.bias"], 1e-5)
                wqkv = torch.cat([v[f"ar_channel.layers.0.mha.{k}.weight"] for k in ("query", "key", "value")])
                snap["ring" + tag], snap["cache" + tag] = ring[0].numpy().copy(), (xn @ wqkv.T)[0].numpy().copy()
            snap["h" + tag], snap["c" + tag] = s.h[0, :, None, :].numpy().copy(), s.c[0, :, None, :].numpy().copy()
        return snap


# ---- the checker ------------------------------------------------------------------------------------------------------------------------
def check_block(field, got, w64, w32, where, row_name, figures):
    """One stream's block of one field, [2, rows, W], under encoder_stages.stage_bound.  ``row_name(t)`` says what row t is."""
    got = np.asarray(got)
    assert got.shape == w64.shape, f"{where}: {field} has shape {got.shape}, the oracle's block {w64.shape}"
    g = got.astype(np.float64)
    if not np.isfinite(g).all():
        c, t, col = (int(v[0]) for v in np.nonzero(~np.isfinite(g)))
        raise AssertionError(f"{where}: {field} {row_name(t)} channel {c} column {col} is not finite")
    bound, e32, scale = ES.stage_bound(field, w64, w32)
    diff = np.abs(g - w64)
    err = diff.max(axis=2)
    if (err > bound).any():
        t = int(np.flatnonzero((err > bound).any(axis=0))[0])
        c = int(np.flatnonzero(err[:, t] > bound)[0])
        col = int(diff[c, t].argmax())
        raise AssertionError(f"{where}: {field} {row_name(t)} channel {c} column {col} is off by {err[c, t]:.3e} > bound {bound:.3e} "
                             f"(E32 {e32:.3e}, max|x| {scale:.3e}; worst of the block {err.max():.3e} = {err.max() / bound:.2f} x bound)")
    f = figures.setdefault(field, {"err/E32": 0.0, "err/bound": 0.0, "E32": 0.0})
    f["err/E32"] = max(f["err/E32"], float(err.max()) / max(e32, 1e-30))
    f["err/bound"] = max(f["err/bound"], float(err.max()) / bound)
    f["E32"] = max(f["E32"], e32)


def check_state(eng, case, truth, slots, owner, seen, what, figures):
    """Every field of every stream's record after ``seen`` frames against the oracles' snapshot of its dialogue."""
    from vap_realtime_amd import engine
    T = case.T
    n = min(seen, T)
    rec = eng.export_streams(slots, cache=True)
    s = engine.split_state(rec, T)
    for k, (slot, d) in enumerate(zip(slots, owner)):
        where = f"case {what} stream {k} (slot {slot}, dialogue {d}) after frame {seen - 1}"
        snap = truth.snap[seen][d]
        assert int(s["n_frames"][k]) == n, f"{where}: n_frames is {int(s['n_frames'][k])}, {n} expected"
        for field in ("ring", "cache"):
            tail = s[field][k][:, n:]
            assert not tail.any(), f"{where}: {field} rows beyond the fill ({n}) are not zero in the record"

            def row_name(t):
                g = seen - n + t
                return f"row {t} (frame {g}, ring slot {g % T})"
            check_block(field, s[field][k][:, :n], snap[field + "64"], snap[field + "32"], where, row_name, figures)
        for i, field in enumerate(("h", "c")):
            check_block(field, s["lstm"][k][:, i][:, None, :], snap[field + "64"], snap[field + "32"], where, lambda t: "(LSTM state)", figures)
        ES.check_carry(s["carry"][k], snap["frame"], what=where)
    return rec


def expect_refusal(eng, name, match, where):
    try:
        eng.peek(name, (1,))
    except AssertionError:
        raise
    except Exception as ex:                                                                # VapxError, or the stand-in's
        assert match in str(ex), f"{where}: peek({name!r}) was refused with {ex!s}, a message with {match!r} was expected"
        return
    raise AssertionError(f"{where}: peek({name!r}) after a prefill returned data; it must be refused")


def check_stages(eng, case, path, truth, call, slots, owner, what, figures):
    """The encoder buffers of the call's last chunk, every entry: entry v = j * n + k is frame j of the chunk, stream k of the call."""
    ch = call.chunks[-1]
    geo = ES.geometry(case.hz)
    kpath = "fused" if ch.fused else "split" if path == "split" else "chain"
    tiles = {"h1": "conv1", "h2": "conv2", "h3": "conv3", "z": "conv4"}
    entries = [(v // case.n, v % case.n) for v in range(ch.V)]
    where = f"case {what} last chunk (V = {ch.V})"
    for st in PEEKABLE:
        if st in ("h2", "h3") and ch.fused:
            expect_refusal(eng, st, "fused conv tail", where)
            continue
        P = geo[st]
        got = eng.peek(st, (ch.V, 2, P + 2 * ES.GUARD.get(st, 0), 256))
        names = []
        for v, (j, k) in enumerate(entries):
            name = f"{k} (slot {slots[k]}, dialogue {owner[k]}) frame {call.start + ch.f0 + j} (chunk frame {j}, entry {v})"
            gm = ch.gemms.get(tiles.get(st, ""))
            if gm:
                name += f" {tiles[st]} {gm[4]}-row tiles {v * 2 * P // gm[4]} .. {((v + 1) * 2 * P - 1) // gm[4]}"
            names.append(name)
        blocks = [truth.stages[(call.start + ch.f0 + j, owner[k])] for j, k in entries]
        ex = {}
        r = ES.check_stage(st, got, [b[0][st] for b in blocks], [b[1][st] for b in blocks], path=kpath, streams=names, what=where, excess=ex)
        f = figures.setdefault(st, {"err/E32": 0.0, "err/bound": 0.0})
        f["err/E32"], f["err/bound"] = max(f["err/E32"], r), max(f["err/bound"], ex.get(st, 0.0))
    for name in REFUSED:
        expect_refusal(eng, name, "not written by vapx_prefill", where)


def check_launches(got: Dict[str, int], want: Dict[str, int], where: str):
    for k, v in want.items():
        assert got.get(k, 0) == v, f"{where}: {v} {k} launches expected, profile_read says {got}"
    extra = set(got) - set(want)
    assert not extra, f"{where}: a prefill launched {sorted(extra)}: {got}"


def outputs_of(out):
    if isinstance(out, dict):
        return out
    from vap_realtime_amd import engine
    return engine.split_outputs(out)


def run_case(eng, case: Case, path: str, truth: Truth, route: str = "device", stages: bool = True, what: Optional[str] = None) -> dict:
    """The whole checker on one engine (or stand-in): walks the case's program, checks every stream's record after every prefill call, the
    launch counts where the engine counts launches, the encoder buffers of the last chunk, and three ordinary steps afterwards.  Returns
    {"figures": per field worst err / E32, err / bound and E32; "records": the records after the last call; "cont": worst output error}."""
    what = what or f"{case.id} {path} {route}"
    pl = plan(case, path, (route,))
    slots, owner, _ = population(case)
    audio = truth.audio[owner]
    hop, figures, seen, calls = case.hop, {}, 0, iter(zip(pl.calls, pl.launches))
    rec = None
    counts = hasattr(eng, "profile_read")
    for op, k in case.program:
        if op == "step":
            for f in range(seen, seen + k):
                eng.step(audio[:, :, f * hop:(f + 1) * hop], slots)
        else:
            call, launches = next(calls)
            block = np.ascontiguousarray(audio[:, :, seen * hop:(seen + k) * hop])
            if counts:
                eng.profile_enable(range(16))
                eng.profile_read()
            if route == "device":
                import torch
                dev = torch.from_numpy(block).cuda()
                assert eng.prefill(dev, slots) == k
                torch.cuda.synchronize()
            else:
                assert eng.prefill(block, slots) == k
            if counts:
                check_launches({name: int(v[1]) for name, v in eng.profile_read().items()}, launches, f"case {what} call at frame {seen}")
                eng.profile_enable(())
        seen += k
        if op == "prefill":
            rec = check_state(eng, case, truth, slots, owner, seen, what, figures)
    if stages:
        check_stages(eng, case, path, truth, call, slots, owner, what, figures)
    worst = 0.0
    for f in range(seen, seen + CONT):
        o = outputs_of(eng.step(audio[:, :, f * hop:(f + 1) * hop], slots))
        assert np.all(np.asarray(o["n"]) == min(f + 1, case.T)), f"case {what} step at frame {f}: n is {o['n']}"
        for k, d in enumerate(owner):
            for key, want in truth.cont[(f, d)].items():
                err = float(np.abs(np.asarray(o[key][k], np.float64) - want).max())
                worst = max(worst, err)
                assert err <= TOL_OUT, f"case {what} stream {k} (slot {slots[k]}, dialogue {d}) step at frame {f}: {key} is off by {err:.3e} > {TOL_OUT}"
    if stages:                                                                             # the step has cleared the prefill's view
        eng.peek("lstm_out", (case.n, 2, ES.geometry(case.hz)["lstm_out"], 256))
    return {"figures": figures, "records": rec, "cont": worst}


# ---- a stand-in engine backed by an oracle (tests/test_prefill_classes.py) ------------------------------------------------------------------
class Refused(RuntimeError):
    pass


class StandIn:
    """The ``Engine`` methods ``run_case`` uses, on a ``VapOracle`` of either precision: ``prefill`` walks the engine's own chunk plan over
    (frame, stream) entries - the CNN per entry, the LSTM per stream along the chunk's frames, the ring fill with the in-kernel skip - and
    ``fault`` seeds one thing a kernel could get wrong:

        "overwritten_wins"  a frame that a later frame of the same chunk overwrites is written anyway, and last
        "stream_major"      the LSTM reads entry k * fc + j for frame j of stream k (the virtual batch is frame-major: j * n + k)
        "lstm_restart"      a call's second chunk starts from the LSTM state the call started from
        "carry_prefix"      the first frame of a later chunk is prefixed by the stream's carry, not by the block's own 320 samples
        "bhead0"            the call's first frame goes to ring slot 0 whatever the ring holds
        "tile128"           h1 of the last chunk is off by 1e-3 (relative) in rows 128 .. 255 of conv1's output
        "c_rel"             the exported c is off by 1e-4 (relative)"""

    def __init__(self, orc, case: Case, max_streams: int, fault: Optional[str] = None):
        import torch
        self.o, self.case, self.T, self.hop, self.fault = orc, case, case.T, case.hop, fault
        self.max_batch = case.max_batch
        self.h = [torch.zeros(2, 256, dtype=orc.dtype) for _ in range(max_streams)]
        self.c = [torch.zeros(2, 256, dtype=orc.dtype) for _ in range(max_streams)]
        self.carry = np.zeros((max_streams, 2, 320), np.float32)
        self.ring = [dict() for _ in range(max_streams)]                                    # slot -> [2, 256]
        self.seen = [0] * max_streams
        self.last = None                                                                   # ("prefill", stages, fused) | ("step",)

    def _window(self, sid):
        fs, n = self.seen[sid], min(self.seen[sid], self.T)
        return [self.ring[sid][(fs - n + t) % self.T] for t in range(n)]

    def step(self, audio, ids):
        import torch
        from oracle.vap_oracle import OracleState
        outs = []
        for k, sid in enumerate(int(s) for s in ids):
            frame = np.concatenate([self.carry[sid], np.asarray(audio[k], np.float32)], axis=1)
            self.carry[sid] = frame[:, -320:]
            st = OracleState(1, self.T, [r[None] for r in self._window(sid)], self.h[sid][None], self.c[sid][None])
            out = self.o.step(frame[None], st)
            self.h[sid], self.c[sid] = st.h[0], st.c[0]
            self.ring[sid][self.seen[sid] % self.T] = st.ring[-1][0]
            self.seen[sid] += 1
            out["n"] = np.array([len(st.ring)])
            outs.append(out)
        self.last = ("step",)
        return {k: np.concatenate([np.asarray(o[k]) for o in outs]) for k in ("p_now", "p_future", "vad", "logits", "n")}

    def prefill(self, audio, ids):
        import torch
        from vap_realtime_amd import engine
        o, T, hop, fault = self.o, self.T, self.hop, self.fault
        audio = np.asarray(audio, np.float32)
        ids = [int(s) for s in ids]
        n, frames = len(ids), audio.shape[2] // hop
        bhead = [0 if fault == "bhead0" else self.seen[s] % T for s in ids]
        h0 = [self.h[s].clone() for s in ids]
        c0 = [self.c[s].clone() for s in ids]
        with torch.no_grad():
            for ci, (f0, fc, fills) in enumerate(engine.prefill_chunks(self.max_batch, n, frames, T)):
                V = n * fc
                zs, stages = [], {st: [] for st in PEEKABLE}
                for v in range(V):
                    j, k = v // n, v % n
                    g = f0 + j
                    pre = audio[k][:, g * hop - 320:g * hop] if g else self.carry[ids[k]]
                    if fault == "carry_prefix" and j == 0:
                        pre = self.carry[ids[k]]
                    x = torch.from_numpy(np.concatenate([pre, audio[k][:, g * hop:(g + 1) * hop]], axis=1)).to(o.dtype)
                    col = {}
                    zs.append(o.cnn(x.reshape(2, 1, o.L), col).transpose(1, 2)[:, 1:-1, :])
                    for i in range(4):
                        stages[f"h{i}"].append(col[f"cnn{i}"].transpose(1, 2).numpy())
                    stages["z"].append(zs[-1].numpy())
                e = {}
                for k, sid in enumerate(ids):
                    if fault == "lstm_restart" and ci == 1:
                        self.h[sid], self.c[sid] = h0[k], c0[k]
                    for j in range(fc):
                        z = zs[k * fc + j] if fault == "stream_major" else zs[j * n + k]
                        y, self.h[sid], self.c[sid] = o.lstm(z, self.h[sid], self.c[sid])
                        e[(j, k)] = o.downsample(y)
                stages["e"] = [e[(v // n, v % n)][:, None, :].numpy() for v in range(V)]
                fused = self.case.hz in (50, 20) and V <= FUSED_MAX
                self.last = ("prefill", {st: np.ascontiguousarray(np.stack(b)) for st, b in stages.items()}, fused)
                if not fills:
                    continue
                order = range(fc - 1, -1, -1) if fault == "overwritten_wins" else range(fc)
                for j in order:
                    g = f0 + j
                    if g + T < frames and fault != "overwritten_wins":
                        continue
                    for k, sid in enumerate(ids):
                        self.ring[sid][(bhead[k] + g) % T] = e[(j, k)]
        for k, sid in enumerate(ids):
            self.carry[sid] = audio[k][:, -320:]
            self.seen[sid] += frames
        if fault == "tile128":
            h1 = self.last[1]["h1"]
            flat = h1.reshape(-1, 256)                                                     # [V * 2 * P1] rows: conv1's output
            assert np.shares_memory(flat, h1) and flat.shape[0] >= 256
            flat[128:256] *= 1.0 + 1e-3
        return frames

    def peek(self, name, shape):
        if self.last[0] == "prefill":
            if name not in PEEKABLE:
                raise Refused(f"\"{name}\" is not written by vapx_prefill")
            if name in ("h2", "h3") and self.last[2]:
                raise Refused(f"\"{name}\" stays in LDS in the fused conv tail")
            return ES.with_guards(name, self.last[1][name]).astype(np.float32).reshape(shape)
        return np.zeros(shape, np.float32)

    def export_streams(self, ids, cache=False):
        import torch
        from vap_realtime_amd import engine as E
        assert cache
        rec = np.zeros((len(ids), E.state_record_floats(self.T, True)), np.float32)
        d = E.split_state(rec, self.T)
        v = self.o.v
        wqkv = torch.cat([v[f"ar_channel.layers.0.mha.{k}.weight"] for k in ("query", "key", "value")])
        for b, sid in enumerate(int(s) for s in ids):
            win = self._window(sid)
            d["n_frames"][b] = len(win)
            d["lstm"][b][:, 0], d["lstm"][b][:, 1] = self.h[sid].numpy(), self.c[sid].numpy() * (1.0 + 1e-4 if self.fault == "c_rel" else 1.0)
            d["carry"][b] = self.carry[sid]
            if win:
                with torch.no_grad():
                    ring = torch.stack(win, dim=1)[None]                                   # [1, 2, n, 256]
                    xn = torch.nn.functional.layer_norm(ring, (256,), v["ar_channel.layers.0.ln_self_attn.weight"],
                                                        v["ar_channel.layers.0.ln_self_attn.bias"], 1e-5)
                    d["ring"][b][:, :len(win)], d["cache"][b][:, :len(win)] = ring[0].numpy(), (xn @ wqkv.T)[0].numpy()
        return rec
