"""Random programs of the state-changing calls of the C ABI against float64: the program, the dialogue-level model, the checker and a
slot-level stand-in (the CPU proof is tests/test_stream_program.py, the engines run in tests/test_stream_program_gpu.py).

``draw(profile, seed)`` draws the whole program before anything runs: a list of ticks, each a list of *chains* of operations, one ragged
step, and (after a step with ``defer_join``) the chains that run between that step and its join.  A chain is one or more operations that
run back to back; the state audit follows the chain, on the slots it touched.  The audit itself is a state call and applies every queued
reset, so an ordering such as "a reset queued on a slot, then an import into that slot" has to sit inside one chain: between two audits
nothing is left queued.  Single full resets are drawn with and without an audit of their own, so both the step and a state call get to
apply them; the crowd's flush of 17 resets has none, the step of that tick applies it.  A carry-only reset or a class change is always
audited: a carry that survived it moves the step's outputs by far less than 1e-4 and is gone after the step, so only the audit sees it
(tests/test_stream_program.py shows that with the fault "carry_survives_class_change").

The truth is dialogue-level and knows nothing about slots: per dialogue a float64 and a torch-fp32 ``VapOracle`` state behind one
``ServerFramer``.  ``Truth`` walks the program once and keeps, per stepped row, the float64 outputs, and per audit the snapshot of every
dialogue it covers (ring, layer-0 Q|K|V cache as LN(ring) . Wqkv^T, h, c of both oracles, the carry).  Resets are applied to the model where
the program requests them; the engine queues them, which has to be indistinguishable.

    reset_stream                        fresh oracle state, fresh framer
    reset_carry                         fresh framer; window and LSTM kept
    mig_state   get_state -> reset_stream(src) -> set_state(dst)                                  identity
    mig_rec     export_streams -> reset_stream(src) -> import_streams(dst), cache yes / no, records on the host / the device   identity
    mig_engine  the same through host records without cache into an engine of the other precision                         identity
    attach      (reset_stream of the slot the dialogue leaves, if it lives) prefill of k frames into a free slot, or into the slot it left:
                a fresh dialogue advanced over k frames
    cont        prefill of the next k frames of a live stream: advanced over k frames
    maps, peek, encode_free (vapx_encode_audio on a FREE slot, then its reset), the audit's own export                    nothing

Checks.  Every stepped row: the outputs the mode publishes (``_compare`` of tests/test_random_ops_gpu.py) against float64 at 1e-4, ``n``
exactly.  Every audit (``export_streams(cache=True)``): n_frames exactly, ring and cache rows beyond the fill zero, ring, cache, h, c per
stream under ``encoder_stages.stage_bound`` unchanged (``prefill_classes.check_block``), the carry bit for bit
(``encoder_stages.check_carry``); a slot that holds no dialogue has n_frames 0 and a zero LSTM, carry, ring and cache.  A peek of ``e`` is
the latest step's ``e`` columns bit for bit.  The runner counts the rows compared and the slot audits made; the tests hold the counts
against the program's.

Input at another rate and in another format (rate_8k_mulaw, rate_48k_s16): the dialogue's audio is a signal at that rate through
``pcm.encode``; the model decodes it and runs ``resample.stream_ref`` in front of the float64 oracle and the same filter in float32
(``stream_f32``) in front of the fp32 one, so E32 includes an fp32 resampler's error as the engine's does.  Both resets restart the
resampler, get / set_state restarts it too (the call has no place for the history), a record carries it.  The audit then also holds
``resample_hist`` and ``resample_started`` exactly (decoded samples are exact in fp32) and the carry within the bound
tests/test_resample_gpu.py derives, K . 2^-24 . max sum|h| . max|x|.  ``vapx_prefill`` must be refused and change nothing.

A class table (class_table): every dialogue has a class per channel; its audio exists as a signal at every class's rate in that
class's format, and a step feeds each channel the row of its class (packed input).  ``set_stream_class`` and
``set_stream_channel_classes`` restart the framer and BOTH channels' resamplers and keep window and LSTM; a get / set_state migration
sets the destination's classes first.  Export, import and prefill must be refused (``VapxError``; the stand-in's ``Refused``), so the
audit goes through ``get_state``: n_frames, ring, LSTM and the carry per channel at its class's bar.  format_16k_alaw reaches the
refusal of prefill for a format alone.

Trunk groups (group_same_rate, group_mixed): a dialogue has one oracle pair per model at that model's own rate and window, behind a
framer of that model's hop, fed R leader hops per frame counted from the dialogue's (re)start (``_GroupModel``).  ``TrunkGroup.step`` and
``step_wire`` alternate; a model's row is compared where its phase says a frame is due and must be STATUS_NO_FRAME and otherwise exactly
zero where not.  ``reset_stream`` restarts every model's window and a slower follower's frame.  At one rate, records move dialogues into
other slots and the audit reads every model's record; with a slower follower export must be refused and the audit reads every model's
``get_state``.  Dialogue d takes its first step on leader tick d % 4, so phases differ inside a batch from the start.

The profiles here: plain_short, plain_long, crowd, two_engines on 16 kHz fp32 input, rate_8k_mulaw, rate_48k_s16, format_16k_alaw,
class_table, group_same_rate and group_mixed."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import encoder_stages as ES
import prefill_classes as PC
from test_random_ops_gpu import _compare

TOL_OUT = 1e-4                               # the project's bar for output rows (tests/test_engine_gpu.py, tests/test_random_ops_gpu.py)
ACTING = 6
PERIOD = 8                                   # every live slot is audited every PERIOD ticks and at the end
X = -1                                       # the crowd's extra streams: one dialogue, held against one oracle


class Profile(NamedTuple):
    name: str
    hz: int
    ctx: float
    T: int
    mode: str
    slots: int                               # per engine
    max_batch: int
    groups: int
    extras: int
    engines: int
    ticks: int
    paths: Tuple[str, ...]
    singles: Tuple[str, ...]
    combos: Tuple[str, ...]
    after: Tuple[str, ...]                   # chains between a deferred step and its join
    weight_seed: int
    input_hz: int = 16000
    input_format: str = "f32"
    table: Tuple[Tuple[str, int], ...] = ()      # an input-class table: (format, rate) per class; every stream has a class per channel
    group: Tuple[Tuple[str, int, int], ...] = () # a trunk group: (mode, frame rate, window) per model, the leader (hz, T, mode above) first

    @property
    def classes(self):
        """(format, rate) per input class; an engine with one rate and format is a table of one class."""
        return self.table or ((self.input_format, self.input_hz),)

    @property
    def decoded(self):
        """The engine decodes or resamples what it is fed (anything but 16 kHz fp32)."""
        return bool(self.table) or self.resampled or self.input_format != "f32"

    @property
    def exports(self):
        """Export is not refused (no class table, no follower slower than its leader): the audit reads records, cache included."""
        return not self.table and all(hz == self.hz for _, hz, _ in self.group)

    @property
    def hop(self):
        return 16000 // self.hz

    @property
    def hop_in(self):
        return self.input_hz // self.hz

    @property
    def resampled(self):
        return self.input_hz != 16000


_PLAIN = ("reset_stream", "reset_carry", "mig_state", "mig_rec", "attach", "cont", "maps", "peek", "encode_free")
_PLAIN_COMBOS = ("P0", "P1", "P2", "P3", "P3b", "P4", "P7", "P8", "P9")
_RATE = ("reset_stream", "reset_carry", "mig_state", "mig_rec", "refuse_prefill")
_RATE_COMBOS = ("P0", "P1", "P2", "P4", "P7", "P9")
_TABLE = ("reset_stream", "reset_carry", "mig_state", "set_class", "set_channel_classes", "refuse_prefill", "refuse_export", "refuse_import")
_TABLE_COMBOS = ("P0", "P2", "P5", "P6")
PROFILES = {p.name: p for p in (
    # max_batch 8 < the window: an import's cache rebuild runs one pass per 8 streams, a prefill of k > 8 frames in several chunks
    Profile("plain_short", 20, 0.625, 12, "vap", 24, 8, 0, 0, 1, 60, ("fp32", "split"), _PLAIN, _PLAIN_COMBOS, (), 41),
    # T = 65: the first long-window class, a last tile of one row
    Profile("plain_long", 50, 1.3, 65, "nod", 16, 8, 0, 0, 1, 52, ("fp32", "split"), _PLAIN, _PLAIN_COMBOS, (), 42),
    # 64 extra streams replay dialogue 0's audio: every batch has >= 64 rows, so groups=2 really splits it over two HIP streams
    # 88 slots: 24 besides the extras, so 17 distinct resets can queue without touching the extras, which replay uninterrupted
    Profile("crowd", 20, 0.625, 12, "vap", 88, 80, 2, 64, 1, 40, ("fp32", "split"),
            ("reset_stream", "reset_carry", "mig_state", "mig_rec", "maps", "peek"), ("P0", "P1", "P2", "P4", "P7", "P9", "FLUSH"),
            ("mig_state", "maps", "mig_rec"), 43),
    # engine 0 runs fp32, engine 1 split precision; dialogues move between them through records without cache
    Profile("two_engines", 20, 0.625, 12, "vap", 12, 12, 0, 0, 2, 50, ("mixed",),
            ("reset_stream", "reset_carry", "mig_engine"), ("P4",), (), 44),
    # an input rate and a format: the resampler history restarts with get / set_state, travels in a record; prefill is refused
    Profile("rate_8k_mulaw", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 50, ("fp32", "split"), _RATE, _RATE_COMBOS, (), 45, 8000, "mulaw"),
    Profile("rate_48k_s16", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 50, ("fp32",), _RATE, _RATE_COMBOS, (), 46, 48000, "s16"),
    # a format alone: nothing is resampled, prefill is refused for the format's own reason
    Profile("format_16k_alaw", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 40, ("fp32",), _RATE, _RATE_COMBOS, (), 47, 16000, "alaw"),
    # four classes, streams with equal and with different channel classes, packed input; export / import / prefill are refused, so the
    # audit goes through get_state (ring, LSTM, carry)
    Profile("class_table", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 60, ("fp32",), _TABLE, _TABLE_COMBOS, (), 48,
            table=(("f32", 16000), ("mulaw", 8000), ("s16", 48000), ("alaw", 32000))),
    # three models on one trunk at one rate, each with its own window: step and step_wire alternate, records move between slots
    Profile("group_same_rate", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 44, ("fp32", "split"), ("reset_stream", "mig_rec"), ("P1", "P7"), (), 49,
            group=(("vap", 20, 12), ("bc", 20, 15), ("nod", 20, 10))),
    # followers at 1/2 and 1/4 of the leader's rate: a frame every R-th leader hop of the stream, counted from its (re)start
    Profile("group_mixed", 20, 0.625, 12, "vap", 16, 16, 0, 0, 1, 48, ("fp32",), ("reset_stream", "refuse_export"), (), (), 50,
            group=(("vap", 20, 12), ("nod", 10, 8), ("bc", 5, 4))),
)}
# (profile, seed) pairs the tests run; tests/test_stream_program.py asserts ``check_coverage`` for each
COMMITTED = (("plain_short", 2), ("plain_long", 4), ("crowd", 1), ("two_engines", 1), ("rate_8k_mulaw", 1), ("rate_48k_s16", 1),
             ("format_16k_alaw", 2), ("class_table", 1), ("group_same_rate", 1), ("group_mixed", 1))

# ordered pairs (triples) of calls on one slot with no step and no audit in between; 12: a full reset subsumes a queued carry-only one
PAIRS = {
    1: ("reset_stream", "import"), 2: ("reset_stream", "set_state"), 3: ("reset_stream", "prefill_attach"), 4: ("reset_carry", "export"),
    5: ("set_stream_channel_classes", "reset_stream"), 6: ("reset_stream", "set_stream_class"), 7: ("import_cache", "reset_stream"),
    8: ("prefill_cont", "export_nocache", "import_nocache"), 9: ("set_state", "export_cache", "import_cache"),
    10: ("step_defer", "get_state"), 11: ("step_defer", "maps"), 12: ("reset_carry", "reset_stream"),
}


class Op(NamedTuple):
    kind: str
    d: Optional[int] = None                  # dialogue, None for a free slot's or a bystander's
    src: Optional[int] = None                # global slot: engine * slots + slot
    dst: Optional[int] = None
    k: int = 0                               # frames of a prefill, rows of a maps call, rows of a peek
    pos: int = 0                             # first audio frame of a prefill
    cache: bool = False
    device: bool = False
    seed: int = 0
    clean: bool = False                      # a migration that also resets its destination before it fills it


class Chain(NamedTuple):
    label: str
    ops: Tuple[Op, ...]
    audit: Tuple[Tuple[int, Optional[int]], ...]   # (global slot, dialogue | None for a free slot | X)
    audit_id: int                                  # -1: no audit


class Step(NamedTuple):
    route: str                                     # "host" | "device" | "defer"
    members: Tuple[Tuple[int, int, int], ...]      # (dialogue | X, global slot, audio frame) in batch order


class Tick(NamedTuple):
    chains: Tuple[Chain, ...]
    step: Optional[Step]
    after: Tuple[Chain, ...]


class Program(NamedTuple):
    profile: Profile
    seed: int
    ticks: Tuple[Tick, ...]
    slots: int                                     # per engine (the crowd's CPU variant has fewer extras)
    extras: Tuple[int, ...]                        # their slots
    start: Tuple[Tuple[int, int, int, int], ...]   # (dialogue, global slot, class of channel 1, of channel 2) before the first tick
    frames: int                                    # audio frames any dialogue needs
    n_rows: int
    n_audits: int                                  # slot audits


def events(op: Op) -> List[Tuple[str, Optional[int]]]:
    """The calls of one operation, with the slot each names."""
    c = "cache" if op.cache else "nocache"
    if op.kind in ("reset_stream", "reset_carry"):
        return [(op.kind, op.src)]
    wipe = [("reset_stream", op.dst)] if op.clean else []
    if op.kind == "mig_state":
        return [("get_state", op.src), ("reset_stream", op.src)] + wipe + [("set_state", op.dst)]
    if op.kind in ("mig_rec", "mig_engine"):
        return [("export_" + c, op.src), ("reset_stream", op.src)] + wipe + [("import_" + c, op.dst)]
    if op.kind == "attach":
        return ([("reset_stream", op.src)] if op.src is not None else []) + [("prefill_attach", op.dst)]
    if op.kind == "cont":
        return [("prefill_cont", op.src)]
    if op.kind == "encode_free":
        return [("encode_audio", op.src), ("reset_stream", op.src)]
    if op.kind == "set_class":
        return [("set_stream_class", op.src)]
    if op.kind == "set_channel_classes":
        return [("set_stream_channel_classes", op.src)]
    return [(op.kind, None)]


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------
class _Drawer:
    def __init__(self, p: Profile, seed: int, ticks: int, extras: int):
        self.p, self.rng = p, np.random.default_rng([seed, sum(map(ord, p.name))])
        self.S = p.slots - p.extras + extras
        self.ticks = ticks
        perm = self.rng.permutation(self.S)
        self.extras = tuple(int(s) for s in perm[:extras])
        pool = [int(s) for s in perm[extras:]] + [e * self.S + s for e in range(1, p.engines) for s in range(self.S)]
        self.free = set(pool)
        self.slot_of: Dict[int, int] = {}
        self.pos = [0] * ACTING
        self.xpos = 0
        self.last_step_n = [0] * p.engines                # rows of the engine's latest step while its ``e`` is still what a peek returns
        self.seen: Dict[int, int] = {}                    # frames_seen per slot (``_track_seen``)
        self.members: List[int] = []                      # the dialogues of this tick's step
        self.n_audit = 0
        self.n_slot_audits = 0
        self.k_cycle = 0
        prefill = "attach" in p.singles
        start = ACTING - 2 if prefill else ACTING
        order = [int(s) for s in self.rng.permutation(sorted(self.free))]
        for d in range(start):
            self._place(d, order[d])
        self.join_tick = {d: int(self.rng.integers(1, 5)) for d in range(start, ACTING)}
        nc = len(p.classes)                               # dialogue d starts with both channels in class d % nc, every third in two classes
        self.cls = {d: (d % nc, (d + 1 + d // 3) % nc if d % 3 == 2 else d % nc) for d in range(ACTING)}
        self.start = tuple((d, g) + self.cls[d] for d, g in sorted(self.slot_of.items()))

    def _place(self, d, g):
        self.slot_of[d] = g
        self.free.discard(g)

    def engine_of(self, g):
        return g // self.S

    def _free_in(self, e, also=()):
        return sorted(g for g in self.free | set(also) if self.engine_of(g) == e)

    def _pick(self, seq):
        return seq[int(self.rng.integers(len(seq)))]

    def _live(self):
        return sorted(self.slot_of)

    def _next_k(self):
        T = self.p.T
        k = (1, T - 1, T, T + 5)[self.k_cycle % 4]
        self.k_cycle += 1
        return k

    # single operations: each returns the Op and moves the draw's own books
    def reset(self, kind, d=None):
        d = self._pick(self._live()) if d is None else d
        return Op(kind, d, self.slot_of[d])

    def set_classes(self, kind, d=None):
        d = self._pick(self._live()) if d is None else d
        nc = len(self.p.classes)
        c1 = int(self.rng.integers(nc))
        c2 = c1 if kind == "set_class" else int((c1 + 1 + self.rng.integers(nc - 1)) % nc)
        self.cls[d] = (c1, c2)
        return Op(kind, d, self.slot_of[d], k=c1, pos=c2)

    def mig(self, kind, d=None, dst=None, cache=None, device=None):
        d = self._pick(self._live()) if d is None else d
        src = self.slot_of[d]
        e = self.engine_of(src)
        if kind == "mig_engine":
            e, cache, device = 1 - e, False, False
        if dst is None:
            dst = self._pick(self._free_in(e))
        cache = bool(self.rng.integers(2)) if cache is None else cache
        device = bool(self.rng.integers(2)) if device is None else device
        if self.p.group:
            device = False                                                                 # TrunkGroup moves host records
        self.free.add(src)
        self._place(d, dst)
        if kind == "mig_state":
            cache = device = False
            if self.p.table:                                                               # the destination's classes are set first
                return Op(kind, d, src, dst, k=self.cls[d][0], pos=self.cls[d][1])
        elif not cache:
            self.last_step_n[self.engine_of(dst)] = 0                                      # the cache rebuild runs through the step's scratch
        return Op(kind, d, src, dst, cache=cache, device=device)

    def attach(self, d=None, same_slot=False, dst=None):
        if d is None:
            d = self._pick(self._live())
        src = self.slot_of.get(d)
        if src is not None:
            self.free.add(src)
        if dst is None:
            dst = src if same_slot else self._pick(self._free_in(0))
        k = self._next_k()
        op = Op("attach", d, src, dst, k=k, pos=self.pos[d], device=bool(self.rng.integers(2)))
        self._place(d, dst)
        self.pos[d] += k
        self.last_step_n[self.engine_of(dst)] = 0
        return op

    def cont(self, d=None):
        d = self._pick(self._live()) if d is None else d
        k = self._next_k()
        op = Op("cont", d, self.slot_of[d], k=k, pos=self.pos[d], device=bool(self.rng.integers(2)))
        self.pos[d] += k
        self.last_step_n[self.engine_of(op.src)] = 0
        return op

    def chain(self, kind, t) -> Optional[Tuple[str, List[Op], Optional[List[int]]]]:
        """(label, operations, slots to audit | None for every slot) or None where the program's state does not allow ``kind`` now."""
        rng, live = self.rng, self._live()
        if kind in ("reset_stream", "reset_carry"):
            op = self.reset(kind)                      # a full reset is left to the step half the time, where this tick's step has the stream
            return kind, [op], ([op.src] if kind == "reset_carry" or rng.random() < 0.5 or op.d not in self.members else [])
        if kind in ("mig_state", "mig_rec", "mig_engine"):
            op = self.mig(kind)
            return kind, [op], [op.src, op.dst]
        if kind == "attach":
            op = self.attach()
            return kind, [op], [op.src, op.dst]
        if kind == "cont":
            op = self.cont()
            return kind, [op], [op.src]
        if kind == "maps":
            self.last_step_n[0] = 0                    # a level-3 call shares the step's scratch: a peek then sees its batch, not the step's
            return kind, [Op("maps", k=int(rng.integers(1, self.p.T + 1)), pos=int(rng.integers(1, min(self.p.max_batch, 4) + 1)),
                             seed=int(rng.integers(1 << 30)))], None
        if kind == "peek":
            e = int(rng.integers(self.p.engines))
            if not self.last_step_n[e]:
                return None
            return kind, [Op("peek", src=e, k=self.last_step_n[e])], None
        if kind in ("refuse_prefill", "refuse_export", "refuse_import"):
            return kind, [Op(kind, src=self._pick(sorted(self.free | set(self.slot_of.values()))))], None
        if kind in ("set_class", "set_channel_classes"):
            op = self.set_classes(kind)
            return kind, [op], [op.src]
        if kind == "P0":
            a = self.reset("reset_carry")
            b = self.reset("reset_stream", a.d)
            return "P0: reset_carry, reset_stream of the same slot", [a, b], [a.src]
        if kind == "P5":
            a = self.set_classes("set_channel_classes")
            b = self.reset("reset_stream", a.d)
            return "P5: set_stream_channel_classes, reset_stream", [a, b], [a.src]
        if kind == "P6":
            a = self.reset("reset_stream")
            b = self.set_classes("set_class", a.d)
            return "P6: reset_stream, set_stream_class", [a, b], [a.src]
        if kind == "encode_free":
            g = self._pick(self._free_in(0))
            self.last_step_n[0] = 0
            return kind, [Op("encode_free", None, g, seed=int(rng.integers(1 << 30)))], None
        if kind in ("P1", "P2"):                       # a careful server: the destination is reset too, and that request is still queued
            how = "mig_rec" if kind == "P1" else "mig_state"          # when the import / set_state into it begins
            a = self.mig(how)._replace(clean=True)
            return f"{kind}: {how} that resets its destination first", [a], [a.src, a.dst]
        if kind == "P3":                               # hang up and attach a new dialogue in the same slot
            op = self.attach(same_slot=True)
            return "P3: reset_stream, prefill attach into the same slot", [op], [op.dst]
        if kind == "P3b":                              # a slot vacated by set_state's migration takes an attach
            if len(live) < 2:
                return None
            d1, d2 = (int(v) for v in rng.permutation(live)[:2])
            a = self.mig("mig_state", d1)
            b = self.attach(d2, dst=a.src)
            return "P3b: mig_state out of a slot, prefill attach into it", [a, b], [a.src, a.dst, b.src]
        if kind == "P4":
            a = self.reset("reset_carry")
            b = self.mig("mig_engine" if self.p.engines > 1 else "mig_rec", a.d)
            return "P4: reset_carry, export, import", [a, b], [b.src, b.dst]
        if kind == "P7":
            a = self.mig("mig_rec", cache=True)
            b = self.reset("reset_stream", a.d)
            return "P7: import with cache, reset_stream", [a, b], [a.src, a.dst]
        if kind == "P8":
            a = self.cont()
            b = self.mig("mig_rec", a.d, cache=False)
            return "P8: prefill continue, export without cache, import", [a, b], [b.src, b.dst]
        if kind == "P9":
            slid = [d for d in live if self.seen.get(self.slot_of[d], 0) > self.p.T] or live   # a re-based ring that had a rotation
            a = self.mig("mig_state", self._pick(slid))
            b = self.mig("mig_rec", a.d, cache=True)
            return "P9: set_state, export with cache, import", [a, b], [a.src, a.dst, b.dst]
        if kind == "FLUSH":                            # 17 requests in one flush: 16 carry-only and full mixed, then one more
            seen = [d for d in self.members if self.seen.get(self.slot_of[d], 0) > 0]
            if not seen:
                return None
            last = self._pick(seen)                        # the 17th: a full reset of a stream this tick's step has, with a window to lose
            pool = sorted(self.free) + [self.slot_of[d] for d in live if d != last]
            pool = [int(g) for g in rng.permutation(pool)][:16]
            ops = []
            for i, g in enumerate(pool):
                d = next((d for d in live if self.slot_of[d] == g), None)
                ops.append(Op("reset_carry" if i % 3 == 1 else "reset_stream", d, g))
            ops.append(Op("reset_stream", last, self.slot_of[last]))
            return "FLUSH: more than 16 resets in one flush", ops, []
        raise KeyError(kind)

    def audited(self, label, ops, touched) -> Chain:
        if touched is None:
            touched = sorted(self.free | set(self.slot_of.values())) + list(self.extras[:1]) + list(self.extras[-1:])
        slots = []
        for g in touched:
            if g is not None and g not in slots:
                slots.append(g)
        holder = {g: d for d, g in self.slot_of.items()}
        audit = tuple((g, X if g in self.extras else holder.get(g)) for g in slots)
        aid = -1
        if audit:
            aid, self.n_audit = self.n_audit, self.n_audit + 1
            self.n_slot_audits += len(audit)
        return Chain(label, tuple(ops), audit, aid)


def _track_seen(seen: Dict[int, int], op: Op, T: int):
    """frames_seen per slot as the calls leave it (slot arithmetic only)."""
    if op.kind == "reset_stream":
        seen[op.src] = 0
    elif op.kind in ("mig_state", "mig_rec", "mig_engine"):
        seen[op.dst] = min(seen.get(op.src, 0), T)                                         # the ring is re-based to slots 0 .. n-1
        seen[op.src] = 0
    elif op.kind == "attach":
        if op.src is not None:
            seen[op.src] = 0
        seen[op.dst] = op.k
    elif op.kind == "cont":
        seen[op.src] = seen.get(op.src, 0) + op.k


def draw(profile: str, seed: int, ticks: Optional[int] = None, extras: Optional[int] = None) -> Program:
    p = PROFILES[profile]
    ticks = ticks or p.ticks
    dr = _Drawer(p, seed, ticks, p.extras if extras is None else extras)
    rng = dr.rng
    lo = min(p.T + 2, ticks // 2)
    spots = [int(t) for t in rng.permutation(np.arange(lo, max(lo + len(p.combos), ticks - 1)))[:len(p.combos)]]
    forced = dict(zip(spots, p.combos))
    out, n_rows = [], 0
    for t in range(ticks):
        chains = []
        live = dr._live() + [d for d, jt in dr.join_tick.items() if jt == t]
        if p.group:                                    # dialogue d's first leader tick is tick d % 4: phases differ inside a batch from the start
            live = [d for d in live if t >= d % 4]
        dr.members = [d for d in live if rng.random() < 0.8] or [dr._pick(live)]
        for d, jt in dr.join_tick.items():
            if jt == t:
                op = dr.attach(d, dst=dr._pick(dr._free_in(0)))
                chains.append(dr.audited("attach", [op], [op.dst]))
                _track_seen(dr.seen, op, p.T)
        kinds = [forced[t]] if t in forced else []
        if rng.random() < 0.55:
            kinds.append(p.singles[int(rng.integers(len(p.singles)))])
        if rng.random() < 0.2:
            kinds.append(p.singles[int(rng.integers(len(p.singles)))])
        kinds.sort(key=lambda k: k == "FLUSH")         # the flush of > 16 resets comes last: this tick's step has to apply it, no audit
        for kind in kinds:
            if kind == "FLUSH" and t and t % PERIOD == 0:
                chains.append(dr.audited("periodic audit", [], None))
            made = dr.chain(kind, t)
            if made:
                for op in made[1]:
                    _track_seen(dr.seen, op, p.T)
                chains.append(dr.audited(*made))
        if t and t % PERIOD == 0 and "FLUSH" not in kinds:
            chains.append(dr.audited("periodic audit", [], None))
        members = dr.members
        rows = [(d, dr.slot_of[d], dr.pos[d]) for d in members] + [(X, g, dr.xpos) for g in dr.extras]
        rows = [rows[i] for i in rng.permutation(len(rows))]
        for d in members:
            dr.pos[d] += 1
        dr.xpos += 1 if dr.extras else 0
        for d, g, _ in rows:
            dr.seen[g] = dr.seen.get(g, 0) + 1
        routes = ("device", "defer") if p.groups else ("host", "host", "device")
        route = ("step", "wire")[t % 2] if p.group else routes[int(rng.integers(len(routes)))]   # a group: step and step_wire alternate
        step = Step(route, tuple(rows))
        n_rows += len(rows)
        for e in range(p.engines):
            dr.last_step_n[e] = sum(1 for _, g, _ in rows if dr.engine_of(g) == e)
        after = []
        if step.route == "defer":
            made = dr.chain(p.after[int(rng.integers(len(p.after)))], t)
            if made:
                for op in made[1]:
                    _track_seen(dr.seen, op, p.T)
                after.append(dr.audited(*made))
        out.append(Tick(tuple(chains), step, tuple(after)))
    out.append(Tick((dr.audited("final audit", [], None),), None, ()))
    return Program(p, seed, tuple(out), dr.S, dr.extras, dr.start, max(max(dr.pos), dr.xpos) + 1, n_rows, dr.n_slot_audits)


# ---- coverage: conditions on the program, not on the engine ---------------------------------------------------------------------------------
QUEUED_ONLY = ("reset_stream", "reset_carry", "set_stream_class", "set_stream_channel_classes", "maps", "step_defer")   # calls that apply no queue


def _match(seq, pattern) -> bool:
    """``pattern`` (call names; a name without suffix matches both cache variants) occurs in order in ``seq`` of (call, slot): the first two
    on one slot, a third (the import of a migration) wherever the record goes."""
    def is_(name, want):
        return name == want or name.startswith(want + "_")
    for i, (a, s) in enumerate(seq):
        if not is_(a, pattern[0]):
            continue
        for j in range(i + 1, len(seq)):
            b, s2 = seq[j]
            if len(pattern) == 2 and any(c not in QUEUED_ONLY for c, _ in seq[i + 1:j]):
                break                                  # a state call in between has applied the queue: the pair is not what it looks like
            if is_(b, pattern[1]) and (s2 == s or s is None or s2 is None):
                if len(pattern) == 2 or any(is_(c, pattern[2]) for c, _ in seq[j + 1:]):
                    return True
    return False


def coverage(prog: Program) -> dict:
    p, T = prog.profile, prog.profile.T
    counts: Dict[str, int] = {}
    pairs, fills, seen = set(), set(), {}
    steps = 0
    part = {d: 0 for d in range(ACTING)}
    rot_ok = flush_ok = False
    min_rows, empty_steps = 1 << 30, 0
    ks = set()
    slowest = max([p.hz // hz for _, hz, _ in p.group] or [1])   # leader hops per frame of the slowest model
    group = {"reset_mid": 0, "phases_differ": 0, "no_frame_rows": 0}

    def count(op):
        counts[op.kind] = counts.get(op.kind, 0) + 1
        if op.kind == "mig_rec":
            for key in ("mig_rec cache" if op.cache else "mig_rec nocache", "records on device" if op.device else "records on host"):
                counts[key] = counts.get(key, 0) + 1
        if op.kind in ("attach", "cont"):
            ks.add(op.k)
            key = "prefill device" if op.device else "prefill host"
            counts[key] = counts.get(key, 0) + 1

    def walk(chain, prefix=()):
        seq = list(prefix)
        for op in chain.ops:
            count(op)
            seq += events(op)
            if op.kind == "reset_stream" and op.d is not None and seen.get(op.src, 0) % slowest:
                group["reset_mid"] += 1                # the slowest follower holds part of a frame
            _track_seen(seen, op, T)
        for n, pat in PAIRS.items():
            if _match(seq, pat):
                pairs.add(n)
        for g, d in chain.audit:
            if d is not None and d != X:
                fs = seen.get(g, 0)
                fills.add("n<T" if 0 < fs < T else "n==T" if fs == T else "slid" if fs > T else "empty")

    for t, tick in enumerate(prog.ticks):
        for ch in tick.chains:
            walk(ch)
            resets = [op for op in ch.ops if op.kind in ("reset_stream", "reset_carry")]
            if len(resets) == len(ch.ops) >= 17 and tick.step is not None:
                stepped = {g for _, g, _ in tick.step.members}
                mixed = {op.kind for op in resets[:16]} == {"reset_stream", "reset_carry"}
                by_step = ch is tick.chains[-1] and not ch.audit                                  # nothing but the step can apply it
                flush_ok |= by_step and mixed and resets[16].kind == "reset_stream" and resets[16].src in stepped and len({op.src for op in resets}) == len(resets)
        if tick.step is None:
            continue
        steps += 1
        counts["step " + tick.step.route] = counts.get("step " + tick.step.route, 0) + 1
        acting = [d for d, _, _ in tick.step.members if d != X]
        empty_steps += not acting
        min_rows = min(min_rows, len(tick.step.members))
        for d in acting:
            part[d] += 1
        group["phases_differ"] += len({seen.get(g, 0) % slowest for _, g, _ in tick.step.members}) > 1
        for _, g, _ in tick.step.members:
            seen[g] = seen.get(g, 0) + 1
            group["no_frame_rows"] += bool(seen[g] % slowest)
        rots = [(seen[g] % T, seen[g] > T) for _, g, _ in tick.step.members]
        for i, (r, slid) in enumerate(rots):
            near = [rots[j][0] for j in (i - 1, i + 1) if 0 <= j < len(rots)]
            rot_ok |= slid and r % 32 != 0 and bool(near) and all(r != q for q in near)
        for ch in tick.after:
            walk(ch, [("step_defer", None)])
    return {"counts": counts, "pairs": pairs, "fills": fills, "rotation": rot_ok, "flush17": flush_ok, "steps": steps,
            "participation": {d: part[d] / max(steps, 1) for d in part}, "min_rows": min_rows, "empty_steps": empty_steps, "ks": ks, "group": group}


def legal_operations(p: Profile) -> List[str]:
    ops = [k for k in p.singles]
    if "mig_rec" in p.singles:
        ops += ["mig_rec cache", "mig_rec nocache", "records on device", "records on host"]
    if "attach" in p.singles:
        ops += ["prefill device", "prefill host"]
    if p.group:
        return [k for k in p.singles] + (["mig_rec cache", "mig_rec nocache"] if "mig_rec" in p.singles else []) + ["step step", "step wire"]
    ops += ["step device", "step defer"] if p.groups else ["step host", "step device"]
    return ops


def legal_pairs(p: Profile) -> set:
    got = set()
    if "mig_rec" in p.singles:
        got |= {1, 7} | ({4} if "reset_carry" in p.singles else set()) | ({9} if "mig_state" in p.singles else set())
    if "mig_state" in p.singles:
        got |= {2}
    if "attach" in p.singles:
        got |= {3, 8}
    if p.groups:
        got |= {10, 11}
    if p.engines > 1:
        got |= {4}
    got |= {n for n, c in ((12, "P0"), (5, "P5"), (6, "P6")) if c in p.combos}
    return got


def check_coverage(prog: Program) -> dict:
    """The conditions of one committed (profile, seed); returns ``coverage(prog)``."""
    p, cov = prog.profile, coverage(prog)
    what = f"{p.name} seed {prog.seed}"
    for op in legal_operations(p):
        assert cov["counts"].get(op, 0) >= 3, f"{what}: {op} occurs {cov['counts'].get(op, 0)} times, 3 are needed ({cov['counts']})"
    missing = legal_pairs(p) - cov["pairs"]
    assert not missing, f"{what}: the orderings {sorted(missing)} of PAIRS do not occur"
    assert {"n<T", "n==T", "slid"} <= cov["fills"], f"{what}: the audits see the fills {sorted(cov['fills'])} only"
    assert cov["rotation"], f"{what}: no slid stream whose ring rotation is no multiple of 32 and differs from its batch neighbours'"
    if "attach" in p.singles:
        assert cov["ks"] >= {1, p.T - 1, p.T, p.T + 5}, f"{what}: prefills of {sorted(cov['ks'])} frames only"
    if any(hz != p.hz for _, hz, _ in p.group):                                            # slower followers
        g = cov["group"]
        assert g["reset_mid"] >= 3, f"{what}: {g['reset_mid']} resets in mid-accumulation, 3 are needed"
        assert g["phases_differ"] >= 10, f"{what}: only {g['phases_differ']} batches hold streams of different phases"
        assert g["no_frame_rows"] >= 10, f"{what}: only {g['no_frame_rows']} rows without a frame"
    if "FLUSH" in p.combos:
        # every batch >= 64 rows (so that groups=2 splits it) holds because the draw steps every extra stream on every tick; the shortened
        # CPU variant has fewer than 64 extras and is exempt - an edit that makes the extras ragged must keep min_rows >= 64 at full length
        assert cov["flush17"], f"{what}: no tick queues 17 resets, mixed, the 17th a full reset of a stepped stream"
        assert cov["min_rows"] >= 64 or not prog.extras or len(prog.extras) < 64, f"{what}: a batch of {cov['min_rows']} rows runs in one group"
    low = {d: round(v, 2) for d, v in cov["participation"].items() if v < 0.6}
    assert not low, f"{what}: dialogues {low} take part in fewer than 60 % of the steps"
    assert cov["empty_steps"] == 0, f"{what}: {cov['empty_steps']} steps have no acting member"
    return cov


# ---- the truth --------------------------------------------------------------------------------------------------------------------------
def qkv_rows(o, ring):
    """LN(ring) . Wqkv^T of ar_channel layer 0 for ring rows [..., 256] -> [..., 768], in the oracle's precision."""
    import torch
    v = o.v
    with torch.no_grad():
        xn = torch.nn.functional.layer_norm(ring, (256,), v["ar_channel.layers.0.ln_self_attn.weight"], v["ar_channel.layers.0.ln_self_attn.bias"], 1e-5)
        wqkv = torch.cat([v[f"ar_channel.layers.0.mha.{k}.weight"] for k in ("query", "key", "value")])
        return xn @ wqkv.T


def stream_f32(chunk, state, in_hz):
    """``resample.stream_ref`` in float32 arithmetic (what an fp32 resampler in front of the fp32 oracle computes): the fp32 oracle's own
    error E32 then includes the resampler's, as the engine's does."""
    from vap_realtime_amd import resample
    q = resample.geometry(in_hz)
    orig, new, K, d = q["orig"], q["new"], q["K"], q["d"]
    chunk = np.asarray(chunk, dtype=np.float32)
    n = chunk.shape[-1]
    nblk = n // orig
    buf = np.concatenate([state["hist"].astype(np.float32), chunk], axis=-1)
    h = resample.taps(in_hz).astype(np.float32)
    out = np.zeros(chunk.shape[:-1] + (nblk, new), np.float32)
    for kk in range(K):
        seg = buf[..., kk:kk + orig * nblk:orig]
        for p in range(new):
            out[..., p] = out[..., p] + h[p, kk] * seg
    if not state["started"]:
        out[..., :d, :] = 0.0
    state["hist"], state["started"] = buf[..., n:].astype(np.float64), True
    return out.reshape(chunk.shape[:-1] + (nblk * new,))


def carry_bound(in_hz, peak):
    """The resampled carry's distance from float64, as tests/test_resample_gpu.py derives it: K . 2^-24 . max_p sum_k |h[p][k]| . max|x|."""
    from vap_realtime_amd import resample
    h = resample.taps(in_hz)
    return resample.geometry(in_hz)["K"] * 2.0 ** -24 * float(np.abs(h).sum(axis=1).max()) * peak


class _Model:
    """One dialogue: both oracles' states, each behind a framer and, for input at another rate, a streaming resampler (float64 in front of
    the float64 oracle, float32 in front of the fp32 one)."""

    def __init__(self, truth, cls=(0, 0)):
        self.t, self.cls = truth, cls
        self.reset()

    def reset(self, carry_only=False):
        from oracle.vap_oracle import ServerFramer
        self.fr, self.fr32 = ServerFramer(1, self.t.hop), ServerFramer(1, self.t.hop)
        self.restart_input()
        if not carry_only:
            self.s64, self.s32 = self.t.o64.new_state(1), self.t.o32.new_state(1)

    def rates(self):
        return tuple(self.t.prog.profile.classes[c][1] for c in self.cls)

    def restart_input(self):
        from vap_realtime_amd import resample
        self.rs = [None if hz == 16000 else resample.stream_state(hz) for hz in self.rates()]
        self.rs32 = [None if hz == 16000 else resample.stream_state(hz) for hz in self.rates()]

    def set_classes(self, c1, c2):
        """A new class is a new signal: the carry and both channels' resamplers restart, window and LSTM stay."""
        self.cls = (c1, c2)
        self.reset(carry_only=True)

    def _frames(self, new):
        p = self.t.prog.profile
        if not p.decoded:
            frame = self.fr.frame(new[None])
            return frame, frame
        from vap_realtime_amd import pcm, resample
        y64, y32 = [], []
        for ch, c in enumerate(self.cls):
            fmt, hz = p.classes[c]
            x = pcm.decode(fmt, new[ch], np.float64)
            y64.append(x if hz == 16000 else resample.stream_ref(x, self.rs[ch], hz))
            y32.append(x.astype(np.float32) if hz == 16000 else stream_f32(x, self.rs32[ch], hz))
        return self.fr.frame(np.stack(y64)[None]), self.fr32.frame(np.stack(y32)[None])

    def advance(self, new):
        f64, f32 = self._frames(new)
        self.t.o64.advance(f64, self.s64)
        self.t.o32.advance(f32, self.s32)

    def step(self, new):
        f64, f32 = self._frames(new)
        self.t.o32.advance(f32, self.s32)
        out = self.t.o64.step(f64, self.s64)
        out["n"] = len(self.s64.ring)
        return out

    def snapshot(self):
        import torch
        snap = {"carry": self.fr.carry[0].copy(), "n": len(self.s64.ring), "hz": self.rates(), "cls": self.cls}
        if self.t.prog.profile.resampled:                                                  # one rate: both channels' histories have one size
            snap["hist"], snap["started"] = np.stack([r["hist"] for r in self.rs]).astype(np.float32), bool(self.rs[0]["started"])
        for tag, o, s in (("64", self.t.o64, self.s64), ("32", self.t.o32, self.s32)):
            if s.ring:
                ring = torch.stack(s.ring, dim=2)[0]                                       # [2, n, 256] oldest -> newest
                snap["ring" + tag], snap["cache" + tag] = ring.numpy().copy(), qkv_rows(o, ring).numpy().copy()
            z = torch.zeros(1, 2, 256, dtype=o.dtype)
            h, c = (s.h, s.c) if s.h is not None else (z, z)
            snap["h" + tag], snap["c" + tag] = h[0, :, None, :].numpy().copy(), c[0, :, None, :].numpy().copy()
        return snap


class _GroupModel:
    """One dialogue on a trunk group: per model both oracles' states at that model's own rate behind a framer of its own hop, fed R leader
    hops per frame, counted from the dialogue's (re)start.  (A follower equals a stand-alone engine at its rate:
    tests/test_mixed_trunk_gpu.py::test_other_ratios_follower_equals_standalone_engine.)"""
    cls = (0, 0)

    def __init__(self, truth):
        self.t = truth
        self.reset()

    def restart_input(self):
        pass

    def reset(self, carry_only=False):
        from oracle.vap_oracle import ServerFramer
        assert not carry_only
        p = self.t.prog.profile
        self.R = {m: p.hz // hz for m, hz, _ in p.group}
        self.fr = {m: ServerFramer(1, 16000 // hz) for m, hz, _ in p.group}
        self.acc = {m: [] for m, _, _ in p.group}
        self.s64 = {m: self.t.g64[m].new_state(1) for m, _, _ in p.group}
        self.s32 = {m: self.t.g32[m].new_state(1) for m, _, _ in p.group}

    def step(self, new):
        out = {}
        for m, _, _ in self.t.prog.profile.group:
            self.acc[m].append(new)
            if len(self.acc[m]) < self.R[m]:
                out[m] = None                                                              # no frame due: the model collects
                continue
            frame = self.fr[m].frame(np.concatenate(self.acc[m], axis=1)[None])
            self.acc[m] = []
            self.t.g32[m].advance(frame, self.s32[m])
            out[m] = self.t.g64[m].step(frame, self.s64[m])
            out[m]["n"] = len(self.s64[m].ring)
        return out

    def snapshot(self):
        snaps = {}
        for k, (m, _, _) in enumerate(self.t.prog.profile.group):
            one = _Model.__new__(_Model)
            one.t, one.cls = _OneOf(self.t, m), (0, 0)
            one.fr, one.s64, one.s32 = self.fr[m], self.s64[m], self.s32[m]
            snaps[m] = one.snapshot()
        return snaps


class _OneOf:
    """A truth that shows one model of a group as a plain profile's (for ``_Model.snapshot``)."""

    def __init__(self, truth, m):
        self.o64, self.o32 = truth.g64[m], truth.g32[m]
        self.prog = truth.prog._replace(profile=truth.prog.profile._replace(group=()))


class Truth:
    """The float64 (and fp32) model over one program: ``want[(tick, d)]`` the float64 outputs of dialogue d's row of that tick's step,
    ``snap[(audit_id, d)]`` the model of d at that audit."""

    def __init__(self, prog: Program, weights=None):
        import torch
        from oracle.vap_oracle import VapOracle
        from vap_realtime_amd import synth, weights as W
        p = prog.profile
        self.prog, self.hop = prog, p.hop
        self.cpc, self.vap = weights or W.synthetic_weights(p.weight_seed, p.hz, p.mode)
        self.o64 = VapOracle(self.cpc, self.vap, p.hz, p.ctx, mode=p.mode, dtype=torch.float64)
        self.o32 = VapOracle(self.cpc, self.vap, p.hz, p.ctx, mode=p.mode)
        assert self.o64.T == p.T, (self.o64.T, p.T)
        from vap_realtime_amd import pcm
        self.by_class, self.peak = [], []                   # per class: what a client sends, the signal at the class's rate in its format
        for fmt, hz in p.classes:
            a = synth.dialogue_batch([70 + d for d in range(ACTING)], hz // p.hz * prog.frames)
            a = a if fmt == "f32" else pcm.encode(fmt, a)
            self.by_class.append(a)
            self.peak.append([float(np.abs(pcm.decode(fmt, x, np.float64)).max()) for x in a])
        self.want: Dict[tuple, dict] = {}
        self.snap: Dict[tuple, dict] = {}
        torch.set_num_threads(min(4, torch.get_num_threads()))
        if p.group:                                        # one CPC encoder, every model's own heads and downsample at its own rate
            self.g64, self.g32, self.gvap = {}, {}, {}
            for i, (m, hz, T) in enumerate(p.group):
                vap = W.synthetic_weights(p.weight_seed + 100 * (i + 1), hz, m)[1]
                self.gvap[m] = vap
                self.g64[m] = VapOracle(self.cpc, vap, hz, (T + 0.5) / hz, mode=m, dtype=torch.float64)
                self.g32[m] = VapOracle(self.cpc, vap, hz, (T + 0.5) / hz, mode=m)
                assert self.g64[m].T == T
        models = {d: (_GroupModel(self) if p.group else _Model(self)) for d in list(range(ACTING)) + [X]}
        for d, _, c1, c2 in prog.start:
            models[d].cls = (c1, c2)
            models[d].restart_input()
        for t, tick in enumerate(prog.ticks):
            for ch in tick.chains:
                self._chain(ch, models)
            if tick.step is None:
                continue
            for d in dict.fromkeys(d for d, _, _ in tick.step.members):
                pos = next(f for dd, _, f in tick.step.members if dd == d)
                self.want[(t, d)] = models[d].step(self.frames(d, pos, 1, models[d].cls))
            for ch in tick.after:
                self._chain(ch, models)

    def frames(self, d, pos, k, cls=(0, 0)):
        """What the engine is fed for frames pos .. pos+k-1 of dialogue d: [2, k * hop_in], or with a class table the two channels' rows."""
        rows = []
        for ch, c in enumerate(cls):
            hop_in = self.prog.profile.classes[c][1] // self.prog.profile.hz
            rows.append(self.by_class[c][max(d, 0), ch, pos * hop_in:(pos + k) * hop_in])
        return rows if self.prog.profile.table else np.stack(rows)

    def _chain(self, ch: Chain, models):
        for op in ch.ops:
            if op.d is None:
                continue
            m = models[op.d]
            if op.kind == "reset_stream":
                m.reset()
            elif op.kind == "reset_carry":
                m.reset(carry_only=True)
            elif op.kind == "mig_state":
                m.restart_input()                                                          # the call has no place for the resampler history
            elif op.kind in ("set_class", "set_channel_classes"):
                m.set_classes(op.k, op.pos)
            elif op.kind in ("attach", "cont"):
                if op.kind == "attach":
                    m.reset()
                for f in range(op.pos, op.pos + op.k):
                    m.advance(self.frames(op.d, f, 1))
        for _, d in ch.audit:
            if d is not None and (ch.audit_id, d) not in self.snap:
                self.snap[(ch.audit_id, d)] = models[d].snapshot()


# ---- the checker ------------------------------------------------------------------------------------------------------------------------
def _name(d):
    return "free" if d is None else "X (the extra streams')" if d == X else str(d)


def check_slot(s: dict, b: int, snap: Optional[dict], T: int, where: str, figures: dict, peaks=(0.0, 0.0)):
    """One slot's state (``engine.split_state`` views of a record, or the same names from ``get_state`` where export is refused; a field
    the route does not carry is None) against its dialogue's snapshot, or against an empty slot."""
    n_got = int(s["n_frames"][b])
    if snap is None:
        assert n_got == 0, f"{where}: n_frames is {n_got} in a slot that holds no dialogue"
        for field in ("lstm", "carry", "ring", "cache", "resample_hist", "resample_started"):
            if s.get(field) is not None:
                assert not np.asarray(s[field][b]).any(), f"{where}: {field} is not zero in a slot that holds no dialogue"
        return
    if s.get("resample_hist") is not None:                                                 # decoded samples are exact in fp32: the history is too
        started = int(s["resample_started"][b])
        assert started == (3 if snap["started"] else 0), f"{where}: resample_started is {started}, the model's resampler has{'' if snap['started'] else ' not'} started"
        same = s["resample_hist"][b] == snap["hist"]
        assert same.all(), (f"{where}: resample_hist differs from the model's history in {int((~same).sum())} of {same.size} samples "
                            f"(first: channel {int(np.nonzero(~same)[0][0])} sample {int(np.nonzero(~same)[1][0])})")
    n = snap["n"]
    assert n_got == n, f"{where}: n_frames is {n_got}, {n} expected"
    for field in ("ring", "cache"):
        if s.get(field) is None:
            continue
        assert not s[field][b][:, n:].any(), f"{where}: {field} rows beyond the fill ({n}) are not zero in the record"
        if n:
            PC.check_block(field, s[field][b][:, :n], snap[field + "64"], snap[field + "32"], where, lambda t: f"row {t} of {n} (oldest first)", figures)
    if s.get("lstm") is None:                                                              # a follower: LSTM and carry live in its leader
        return
    for i, field in enumerate(("h", "c")):
        got = s["lstm"][b][:, i][:, None, :]
        if not snap[field + "64"].any():
            assert not got.any(), f"{where}: {field} (LSTM state) is not zero after a reset"
        else:
            PC.check_block(field, got, snap[field + "64"], snap[field + "32"], where, lambda t: "(LSTM state)", figures)
    if all(hz == 16000 for hz in snap["hz"]):
        ES.check_carry(s["carry"][b], snap["carry"], what=f"{where}: carry")
        return
    for ch, hz in enumerate(snap["hz"]):                                                   # per channel: its class decides the carry's bar
        got, want = np.asarray(s["carry"][b][ch:ch + 1], np.float32), np.asarray(snap["carry"][ch:ch + 1], np.float32)
        if hz == 16000:                                                                    # nothing is resampled: bit for bit
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), f"{where}: carry channel {ch} differs from the frame's last 320 samples in {int((~same).sum())} samples"
            continue
        bound = carry_bound(hz, peaks[ch])
        err = np.abs(got.astype(np.float64) - want)[0]
        assert err.max() <= bound, (f"{where}: carry channel {ch} sample {int(err.argmax())} is off by {err.max():.3e} > bound {bound:.3e} "
                                    f"(K . 2^-24 . max sum|h| . max|x| at {hz} Hz, max|x| {peaks[ch]:.3e})")
        f = figures.setdefault("carry", {"err/E32": 0.0, "err/bound": 0.0, "E32": 0.0})
        f["err/bound"] = max(f["err/bound"], float(err.max()) / bound)


class Runner:
    """Drives one program on ``ports`` (one per engine: ``EnginePort`` or ``StandIn``) and checks everything against ``truth``."""

    def __init__(self, prog: Program, truth: Truth, ports):
        self.prog, self.truth, self.ports = prog, truth, list(ports)
        assert len(self.ports) == prog.profile.engines
        self.figures: Dict[str, dict] = {}
        self.rows = self.audits = self.checkpoint = 0
        self.worst_out = 0.0
        self.counts: Dict[str, int] = {}
        self.last_e = [None] * len(self.ports)
        self.cls = {d: (0, 0) for d in list(range(ACTING)) + [X]}                          # the classes of every dialogue's two channels, as the program sets them
        for d, g, c1, c2 in prog.start:
            self.cls[d] = (c1, c2)
            if prog.profile.table:
                port, s = self.where(g)
                port.set_stream_channel_classes(s, c1, c2)

    def where(self, g):
        return self.ports[g // self.prog.slots], g % self.prog.slots

    def _mark(self):
        for p in self.ports:
            p.mark = self.checkpoint

    def run(self):
        try:
            for t, tick in enumerate(self.prog.ticks):
                for ch in tick.chains:
                    self._chain(t, ch)
                if tick.step is None:
                    continue
                self._mark()
                pending = self._step_begin(tick.step)
                for ch in tick.after:
                    self._chain(t, ch, counts=False)
                self._step_end(t, tick.step, pending)
                self.checkpoint += 1
        except AssertionError as ex:
            ex.checkpoint = self.checkpoint
            raise
        return {"figures": self.figures, "rows": self.rows, "audits": self.audits, "worst_out": self.worst_out, "counts": self.counts}

    # -- operations
    def _chain(self, t, ch: Chain, counts=True):
        for op in ch.ops:
            self._mark()
            self.counts[op.kind] = self.counts.get(op.kind, 0) + 1
            self._op(t, ch, op)
        if ch.audit:
            self._mark()
            self._audit(t, ch)
            self.checkpoint += counts                                                      # an audit before a deferred step's join is part of that step's check

    def _op(self, t, ch, op: Op):
        tr = self.truth
        if op.kind in ("reset_stream", "reset_carry"):
            port, s = self.where(op.src)
            getattr(port, op.kind)(s)
        elif op.kind == "mig_state":
            port, s = self.where(op.src)
            state = port.get_state(s)
            port.reset_stream(s)
            if op.clean:
                port.reset_stream(self.where(op.dst)[1])
            if self.prog.profile.table:                                                    # the destination's classes first
                port.set_stream_channel_classes(self.where(op.dst)[1], op.k, op.pos)
            port.set_state(self.where(op.dst)[1], state)
        elif op.kind == "set_class":
            port, s = self.where(op.src)
            port.set_stream_class(s, op.k)
            self.cls[op.d] = (op.k, op.k)
        elif op.kind == "set_channel_classes":
            port, s = self.where(op.src)
            port.set_stream_channel_classes(s, op.k, op.pos)
            self.cls[op.d] = (op.k, op.pos)
        elif op.kind in ("mig_rec", "mig_engine"):
            (pa, s), (pb, q) = self.where(op.src), self.where(op.dst)
            rec = pa.export([s], op.cache, op.device)
            pa.reset_stream(s)
            if op.clean:
                pb.reset_stream(q)
            pb.import_([q], rec, op.cache, op.device)
        elif op.kind in ("attach", "cont"):
            if op.kind == "attach" and op.src is not None:
                port, s = self.where(op.src)
                port.reset_stream(s)
            port, s = self.where(op.dst if op.kind == "attach" else op.src)
            port.prefill(np.ascontiguousarray(tr.frames(op.d, op.pos, op.k)[None]), [s], op.device)
        elif op.kind in ("refuse_prefill", "refuse_export", "refuse_import"):
            port, s = self.where(op.src)
            said = port.refused(op.kind[7:], s)                                            # the port's own refusal type (VapxError; the stand-in's Refused), or None
            assert said is not None, f"tick {t} [{ch.label}] slot {s}: {op.kind[7:]} went through, this engine must refuse it"
            assert "refused" in said, f"tick {t} [{ch.label}] slot {s}: {op.kind[7:]} failed with {said!r}, a refusal was expected"
        elif op.kind == "maps":
            self.ports[0].maps(op.pos, op.k, op.seed)
        elif op.kind == "encode_free":
            port, s = self.where(op.src)
            port.encode_free(s, op.seed)
            port.reset_stream(s)
        elif op.kind == "peek":
            got = self.ports[op.src].peek_e(op.k)
            want = self.last_e[op.src]
            assert want is not None and want.shape == got.shape, f"tick {t} {ch.label}: a peek of e for {op.k} rows, the latest step had {None if want is None else len(want)}"
            assert np.array_equal(got, want), f"tick {t} {ch.label}: peek(e) differs from the e columns of the latest step's output rows"
        else:
            raise KeyError(op.kind)

    def _audit(self, t, ch: Chain):
        from vap_realtime_amd import engine
        T = self.prog.profile.T
        for e, port in enumerate(self.ports):
            mine = [(g % self.prog.slots, d) for g, d in ch.audit if g // self.prog.slots == e]
            if not mine:
                continue
            if self.prog.profile.group:                                                    # {model: fields}: records, or get_state where export is refused
                s = port.group_states([g for g, _ in mine])
            elif self.prog.profile.table:                                                  # export is refused: ring, LSTM and carry through get_state
                s = port.states([g for g, _ in mine])
            else:
                s = engine.split_state(port.records([g for g, _ in mine]), T, input_hz=self.prog.profile.input_hz)
            for b, (slot, d) in enumerate(mine):
                where = f"{self.prog.profile.name} seed {self.prog.seed} tick {t} after [{ch.label}] engine {e} slot {slot}, dialogue {_name(d)}"
                snap = None if d is None else self.truth.snap[(ch.audit_id, d)]
                peaks = (0.0, 0.0) if d is None or self.prog.profile.group else tuple(self.truth.peak[c][max(d, 0)] for c in snap["cls"])
                if self.prog.profile.group:
                    for m, _, Tm in self.prog.profile.group:
                        check_slot(s[m], b, None if snap is None else snap[m], Tm, f"{where} model {m}", self.figures, peaks)
                else:
                    check_slot(s, b, snap, T, where, self.figures, peaks)
                self.audits += 1

    # -- the step
    def _step_begin(self, step: Step):
        tr, S = self.truth, self.prog.slots
        pending = []
        for e, port in enumerate(self.ports):
            rows = [(i, d, g % S, pos) for i, (d, g, pos) in enumerate(step.members) if g // S == e]
            if not rows:
                continue
            new = [tr.frames(d, pos, 1, self.cls[d]) for _, d, _, pos in rows]
            if not self.prog.profile.table:
                new = np.ascontiguousarray(np.stack(new))
            port.step_begin(new, np.array([s for _, _, s, _ in rows], np.int32), step.route)
            pending.append((e, port, rows))
        return pending

    def _step_end(self, t, step: Step, pending):
        p = self.prog.profile
        for e, port, rows in pending:
            got = port.step_end()
            if p.group:
                self._group_rows(t, step, e, rows, got)
                continue
            self.last_e[e] = np.array(got["e"][:len(rows)], np.float32)
            for i, (_, d, slot, pos) in enumerate(rows):
                want = self.truth.want[(t, d)]
                where = f"{p.name} seed {self.prog.seed} tick {t} after [step {step.route}] engine {e} slot {slot}, dialogue {_name(d)}"
                n_want = int(want["n"])
                assert int(got["n"][i]) == n_want, f"{where}: n is {int(got['n'][i])}, {n_want} expected"
                err = _compare(p.mode, got, i, want)
                self.worst_out = max(self.worst_out, err)
                assert err <= TOL_OUT, f"{where} (batch row {i}, audio frame {pos}): outputs are off by {err:.3e} > {TOL_OUT}"
                self.rows += 1


def _group_rows(self, t, step, e, rows, got):
    """A trunk group's step: ``got[model]`` = (columns, status [n], every other column zero [n]).  A model with a frame due for the row is
    held against its own oracle; a model without one must give STATUS_NO_FRAME and zeros, on exactly the ticks the dialogue's phase says."""
    from vap_realtime_amd import engine
    p = self.prog.profile
    for i, (_, d, slot, pos) in enumerate(rows):
        for m, _, Tm in p.group:
            cols, status, zero = got[m]
            want = self.truth.want[(t, d)][m]
            where = f"{p.name} seed {self.prog.seed} tick {t} after [step {step.route}] engine {e} slot {slot}, dialogue {_name(d)} model {m}"
            if want is None:
                assert int(status[i]) == engine.STATUS_NO_FRAME, f"{where}: status is {int(status[i])}, no frame is due (STATUS_NO_FRAME expected)"
                assert bool(zero[i]), f"{where}: a row without a frame is not zero"
                continue
            assert int(status[i]) == 0, f"{where}: status is {int(status[i])}, a frame is due"
            assert int(cols["n"][i]) == int(want["n"]), f"{where}: n is {int(cols['n'][i])}, {int(want['n'])} expected"
            err = _compare_group(m, cols, i, want, step.route == "wire")
            self.worst_out = max(self.worst_out, err)
            assert err <= TOL_OUT, f"{where} (batch row {i}, audio frame {pos}): outputs are off by {err:.3e} > {TOL_OUT}"
        self.rows += 1


Runner._group_rows = _group_rows


def _compare_group(mode, cols, i, want, wire):
    """``_compare`` on a full output row; on a wire row the columns the wire publishes (no 256 logits; nod's p_bc rows under their own name)."""
    if not wire:
        return _compare(mode, cols, i, want)
    pairs = [(cols["vad"][i], want["vad"][0])]
    if mode == "vap":
        pairs += [(cols[k][i], want[k][0]) for k in ("p_now", "p_future")]
    elif mode == "bc":
        pairs += [(cols["aux"][i, 1], want["p_bc_react"][0]), (cols["aux"][i, 2], want["p_bc_emo"][0])]
    else:
        pairs += [(cols["aux"][i, 1], want["p_nod_short"][0]), (cols["aux"][i, 2], want["p_nod_long"][0]), (cols["aux"][i, 3], want["p_nod_long_p"][0])]
        n = want["p_bc"].shape[1]
        pairs.append((cols["p_bc_rows"][i, :n], want["p_bc"][0]))
    return max(float(np.abs(np.asarray(a, np.float64).reshape(-1) - np.asarray(b, np.float64).reshape(-1)).max()) for a, b in pairs)


# ---- the engine behind the runner -----------------------------------------------------------------------------------------------------------
class EnginePort:
    """What the runner calls, on a ``vap_realtime_amd.engine.Engine``."""

    def __init__(self, eng):
        import torch
        self.eng, self.torch, self.mark = eng, torch, 0
        self.d_out = torch.zeros(eng.max_batch, 784, device="cuda")
        self._pending = None

    def step_begin(self, new, ids, route):
        from vap_realtime_amd import engine
        torch, n = self.torch, len(ids)
        if route == "host":
            self._pending = ("host", engine.split_outputs(self.eng.step(new, ids)))
            return
        if self.eng.input_classes is not None:                                             # the packed block on the device, ids on the host
            self._keep = (torch.from_numpy(self.eng.pack_input(ids, new)).cuda(),)
            self.eng.step_packed_device(ids, self._keep[0].data_ptr(), self.d_out.data_ptr())
            self._pending = ("device", n)
            return
        self._keep = (torch.from_numpy(np.ascontiguousarray(new)).cuda(), torch.from_numpy(np.ascontiguousarray(ids)).cuda())
        self.eng.step_device(n, self._keep[0].data_ptr(), new.shape[2], self.d_out.data_ptr(), ids_ptr=self._keep[1].data_ptr(), stream=0,
                             defer_join=route == "defer")
        self._pending = ("device", n)

    def step_end(self):
        from vap_realtime_amd import engine
        how, x = self._pending
        self._pending = None
        if how == "host":
            return x
        self.eng.join(0)
        self.torch.cuda.synchronize()
        return engine.split_outputs(self.d_out[:x].cpu().numpy())

    def reset_stream(self, s):
        self.eng.reset_stream(int(s))

    def reset_carry(self, s):
        self.eng.reset_carry(int(s))

    def set_stream_class(self, s, c):
        self.eng.set_stream_class(int(s), int(c))

    def set_stream_channel_classes(self, s, c1, c2):
        self.eng.set_stream_channel_classes(int(s), int(c1), int(c2))

    def refused(self, what, s):
        """The text of the VapxError that ``what`` on slot s raises, None if it goes through."""
        from vap_realtime_amd import engine
        try:
            if what == "prefill":
                self.eng.prefill(np.zeros((1, 2, self.eng.hop), np.float32), [int(s)])
            elif what == "export":
                self.eng.export_streams([int(s)])
            else:
                self.eng.import_streams([int(s)], np.zeros((1, self.eng.state_floats(False)), np.float32))
        except engine.VapxError as ex:
            return str(ex)
        return None

    def states(self, ids):
        """``get_state`` of every slot under the names ``split_state`` gives a record's fields."""
        got = [self.eng.get_state(int(s)) for s in ids]
        return {"n_frames": np.array([g["n_frames"] for g in got]), "ring": np.stack([g["ring"] for g in got]),
                "lstm": np.stack([g["lstm"] for g in got]), "carry": np.stack([g["carry"] for g in got])}

    def get_state(self, s):
        return self.eng.get_state(int(s))

    def set_state(self, s, state):
        self.eng.set_state(int(s), state)

    def export(self, ids, cache, device):
        if not device:
            return self.eng.export_streams(ids, cache=cache)
        torch = self.torch
        rec = torch.empty(len(ids), self.eng.state_floats(cache), device="cuda")
        d_ids = torch.tensor(list(ids), dtype=torch.int32, device="cuda")
        self.eng.export_streams_device(len(ids), rec.data_ptr(), ids_ptr=d_ids.data_ptr(), cache=cache)
        torch.cuda.synchronize()
        return rec

    def import_(self, ids, rec, cache, device):
        if not device:
            self.eng.import_streams(ids, rec, cache=cache)
            return
        torch = self.torch
        d_ids = torch.tensor(list(ids), dtype=torch.int32, device="cuda")
        self.eng.import_streams_device(len(ids), rec.data_ptr(), ids_ptr=d_ids.data_ptr(), cache=cache)
        torch.cuda.synchronize()

    def prefill(self, audio, ids, device):
        if device:
            dev = self.torch.from_numpy(audio).cuda()
            assert self.eng.prefill(dev, ids) == audio.shape[2] // self.eng.hop
            self.torch.cuda.synchronize()
        else:
            assert self.eng.prefill(audio, ids) == audio.shape[2] // self.eng.hop

    def maps(self, n, rows, seed):
        torch = self.torch
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, 2, rows, 256, generator=g).cuda()
        o = torch.full((n, 2, rows, 256), float("nan"), device="cuda")
        attn = torch.full((n, 2, 1, 4, rows, rows), float("nan"), device="cuda")
        self.eng.transformer_maps_device(n, rows, x.data_ptr(), o_ptr=o.data_ptr(), stage=1, attn_ptr=attn.data_ptr())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(attn).all()), "transformer_maps_device left rows unwritten"

    def peek_e(self, n):
        return self.eng.peek("e", (n, 2, 1, 256)).reshape(n, 2, 256)

    def encode_free(self, s, seed):
        torch = self.torch
        g = torch.Generator().manual_seed(seed)
        frames = (0.1 * torch.randn(1, 2, self.eng.L, generator=g)).cuda()
        e = torch.full((1, 2, 256), float("nan"), device="cuda")
        self.eng.encode_audio_device(1, frames.data_ptr(), e.data_ptr(), stream_ids=[int(s)])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(e).all())

    def records(self, ids):
        return self.eng.export_streams(ids, cache=True)


# ---- a stand-in engine backed by an oracle (tests/test_stream_program.py) ------------------------------------------------------------------
FAULTS = ("late_reset", "seventeenth_dropped", "stale_cache", "cache_not_rotated", "set_state_keeps_head", "prefill_from_zero_carry",
          "carry_only_clears_window", "bystander_advances", "history_survives_reset_carry", "history_lost_on_import",
          "carry_survives_class_change", "follower_phase_survives_reset")


class StandIn:
    """The port's methods at slot level on a ``VapOracle`` of either precision, written without the dialogue-level model: per slot a
    physical ring and cache (dictionaries by ring slot), ``seen`` (frames_seen), h, c, the carry, and the list of queued resets with the
    engine's own rules (a full reset subsumes a queued carry-only one, a request already queued is dropped; every state-touching call
    applies the list first, a maps call does not).  ``fault`` seeds one thing the engine could get wrong; ``fault_mark`` is the runner's
    checkpoint count when it first did:

        "late_reset"                a queued reset is applied after an import / set_state / prefill into the same slot
        "seventeenth_dropped"       only the first 16 queued resets of a flush are applied
        "stale_cache"               an import without cache keeps the slot's previous cache rows
        "cache_not_rotated"         after set_state the cache rows stay at the source's rotation
        "set_state_keeps_head"      the next append goes to the previous tenant's frames_seen % T
        "prefill_from_zero_carry"   a prefill continuing a live stream starts from a zero carry
        "carry_only_clears_window"  a carry-only reset also clears the window
        "bystander_advances"        a maps or encode_audio call changes a live slot's LSTM
        "history_survives_reset_carry"  a carry reset leaves the resampler history in place
        "history_lost_on_import"    an import drops the resampler history
        "carry_survives_class_change"  a class change leaves the carry in place
        "follower_phase_survives_reset"  (``GroupStandIn``) a reset leaves a slower follower's collect phase and collected hops in place"""

    def __init__(self, orc, prog: Program, fault: Optional[str] = None):
        import torch
        assert fault is None or fault in FAULTS
        p = prog.profile
        self.o, self.T, self.hop, self.mode, self.fault = orc, p.T, p.hop, p.mode, fault
        n = prog.slots
        self.h = [torch.zeros(2, 256, dtype=orc.dtype) for _ in range(n)]
        self.c = [torch.zeros(2, 256, dtype=orc.dtype) for _ in range(n)]
        self.carry = np.zeros((n, 2, 320), np.float32)
        self.ring = [dict() for _ in range(n)]
        self.qkv = [dict() for _ in range(n)]
        self.seen = [0] * n
        self.head = [0] * n                                                                # frames_seen % T of the slot's latest tenant
        self.append_at: Dict[int, int] = {}
        self.pending: List[int] = []
        self.mark, self.fault_mark = 0, None
        self._out = self._e = None
        self.hz, self.classes, self.table, self.decoded = p.input_hz, p.classes, bool(p.table), p.decoded
        self.cls = [(0, 0)] * n                                                            # every channel's class; they outlive a reset
        self.rs = [self._fresh_input(s) for s in range(n)]

    def _fresh_input(self, s):
        """A fresh resampler per channel of slot s, None where the channel's class is at 16 kHz."""
        from vap_realtime_amd import resample
        return [None if self.classes[c][1] == 16000 else resample.stream_state(self.classes[c][1]) for c in self.cls[s]]

    def _started(self, s):
        return any(r is not None and r["started"] for r in self.rs[s])

    # -- input classes: the class is the host's at once, the restart of carry and history is queued as a carry-only reset
    def set_stream_channel_classes(self, s, c1, c2):
        if not self.table:
            raise PC.Refused("this engine has no input classes")
        self.cls[s] = (c1, c2)
        if self.fault == "carry_survives_class_change":                                    # only the resamplers restart (they have to: another rate)
            if self.carry[s].any():
                self._hit()
            self.rs[s] = self._fresh_input(s)
            return
        self.reset_carry(s)

    def set_stream_class(self, s, c):
        self.set_stream_channel_classes(s, c, c)

    def refused(self, what, s):
        try:
            if what == "prefill":
                self.prefill(np.zeros((1, 2, self.hop), np.float32), [s], False)
            elif what == "export":
                self.export([s], False, False)
            else:
                self.import_([s], None, False, False)
        except PC.Refused as ex:
            return str(ex)
        return None

    def states(self, ids):
        self._flush()
        T = self.T
        out = {"n_frames": np.array([min(self.seen[s], T) for s in ids]), "ring": np.zeros((len(ids), 2, T, 256), np.float32),
               "lstm": np.zeros((len(ids), 2, 2, 256), np.float32), "carry": np.stack([self.carry[s] for s in ids])}
        for b, s in enumerate(ids):
            for t, r in enumerate(self._window(s)):
                out["ring"][b][:, t] = r.numpy()
            out["lstm"][b][:, 0], out["lstm"][b][:, 1] = self.h[s].numpy(), self.c[s].numpy()
        return out

    def _hit(self):
        if self.fault_mark is None:
            self.fault_mark = self.mark

    # -- queued resets
    def reset_stream(self, s):
        for i, q in enumerate(self.pending):
            if q == s:
                return
            if q == -s - 1:
                self.pending[i] = s
                return
        self.pending.append(s)

    def reset_carry(self, s):
        if s in self.pending or -s - 1 in self.pending:
            return
        self.pending.append(-s - 1)

    def _apply(self, q):
        import torch
        s = q if q >= 0 else -q - 1
        self.carry[s] = 0
        if q < 0 and self.fault == "history_survives_reset_carry":
            if self._started(s):
                self._hit()
        else:
            self.rs[s] = self._fresh_input(s)
        if q >= 0 or self.fault == "carry_only_clears_window":
            if q < 0 and self.seen[s]:
                self._hit()
            self.head[s] = self.seen[s] % self.T
            self.seen[s] = 0
            self.append_at.pop(s, None)
        if q >= 0:
            self.h[s], self.c[s] = torch.zeros_like(self.h[s]), torch.zeros_like(self.c[s])

    def _flush(self, late_for=()):
        todo, self.pending = self.pending, []
        if self.fault == "seventeenth_dropped" and len(todo) > 16:
            self._hit()
            todo = todo[:16]
        late = []
        for q in todo:
            s = q if q >= 0 else -q - 1
            if self.fault == "late_reset" and s in late_for:
                self._hit()
                late.append(q)
            else:
                self._apply(q)
        return late

    # -- the window
    def _window(self, s):
        import torch
        fs, n = self.seen[s], min(self.seen[s], self.T)
        zero = torch.zeros(2, 256, dtype=self.o.dtype)
        return [self.ring[s].get((fs - n + t) % self.T, zero) for t in range(n)]

    def _append(self, s, e):
        at = self.seen[s] % self.T
        if s in self.append_at:
            at = self.append_at.pop(s)
            self._hit()
        self.ring[s][at] = e
        self.qkv[s][at] = qkv_rows(self.o, e)
        self.seen[s] += 1

    def _encode(self, s, new, zero_carry=False):
        """One frame of slot s through the encoder: LSTM and carry advance; returns (frame, e [2, 256])."""
        import torch
        from oracle.vap_oracle import OracleState
        pre = np.zeros_like(self.carry[s]) if zero_carry else self.carry[s]
        if self.decoded:                                                                   # per channel: decode, then the streaming resampler in the oracle's precision
            from vap_realtime_amd import pcm, resample
            rows = []
            for ch, c in enumerate(self.cls[s]):
                fmt, hz = self.classes[c]
                x = pcm.decode(fmt, new[ch], np.float64)
                if hz != 16000:
                    x = resample.stream_ref(x, self.rs[s][ch], hz) if self.o.dtype == torch.float64 else stream_f32(x, self.rs[s][ch], hz)
                rows.append(np.asarray(x, np.float32))
            new = np.stack(rows)
        frame = np.concatenate([pre, np.asarray(new, np.float32)], axis=1)
        self.carry[s] = frame[:, -320:]
        st = OracleState(1, self.T, [], self.h[s][None], self.c[s][None])
        with torch.no_grad():
            e = self.o.encode(torch.from_numpy(frame[None]).to(self.o.dtype), st)[0]
        self.h[s], self.c[s] = st.h[0], st.c[0]
        return frame, e

    # -- the step
    def step_begin(self, new, ids, route):
        from oracle.vap_oracle import OracleState
        self._flush()
        rows = []
        for k, s in enumerate(int(v) for v in ids):
            _, e = self._encode(s, new[k])
            self._append(s, e)
            st = OracleState(1, self.T, [r[None] for r in self._window(s)], self.h[s][None], self.c[s][None])
            row = self._row(self._transformer_only(st), min(self.seen[s], self.T))
            row["e"] = e.numpy().astype(np.float32)
            rows.append(row)
        self._out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}

    def _transformer_only(self, st):
        """The oracle's step on a window that is already complete: the newest row is dropped and given again as this frame's ``e``."""
        o = self.o
        ring = list(st.ring)
        enc = o.encode
        try:
            o.encode = lambda audio, state, collect=None: ring[-1]
            st.ring = ring[:-1]
            return o.step(np.zeros((1, 2, o.L), np.float32), st)
        finally:
            o.encode = enc

    def _row(self, out, n):
        row = {"vad": np.asarray(out["vad"][0]), "aux": np.zeros(4), "logits": np.zeros(256), "p_now": np.zeros(2), "p_future": np.zeros(2),
               "n": np.int32(n), "e": np.asarray(out["e"][0], np.float32)}
        if "logits" in out:
            row["logits"], row["p_now"], row["p_future"] = np.asarray(out["logits"][0]), np.asarray(out["p_now"][0]), np.asarray(out["p_future"][0])
        if self.mode == "bc":
            row["aux"][1], row["aux"][2] = out["p_bc_react"][0], out["p_bc_emo"][0]
        elif self.mode == "nod":
            row["aux"][1], row["aux"][2], row["aux"][3] = out["p_nod_short"][0], out["p_nod_long"][0], out["p_nod_long_p"][0]
            row["logits"] = np.zeros(256)
            row["logits"][:out["p_bc"].shape[1]] = out["p_bc"][0]
        return row

    def step_end(self):
        out, self._out = self._out, None
        self._e = out["e"]
        return out

    # -- state calls
    def get_state(self, s):
        self._flush()
        fs, n = self.seen[s], min(self.seen[s], self.T)
        return {"ring": self._window(s), "n": n, "h": self.h[s].clone(), "c": self.c[s].clone(), "carry": self.carry[s].copy(),
                "rot": (fs - n) % self.T}

    def set_state(self, s, state):
        late = self._flush(late_for=(s,))
        n = state["n"]
        self.ring[s] = {t: r for t, r in enumerate(state["ring"])}
        rot = state["rot"] if self.fault == "cache_not_rotated" else 0
        if rot and n:
            self._hit()
        self.qkv[s] = {(t + rot) % self.T: qkv_rows(self.o, r) for t, r in enumerate(state["ring"])}
        self.seen[s] = n
        self.append_at.pop(s, None)
        if self.fault == "set_state_keeps_head" and self.head[s] != n % self.T:
            self.append_at[s] = self.head[s]
        self.h[s], self.c[s], self.carry[s] = state["h"].clone(), state["c"].clone(), state["carry"].copy()
        self.rs[s] = self._fresh_input(s)                                                  # the call has no place for the resampler history
        for q in late:
            self._apply(q)

    def export(self, ids, cache, device):
        if self.table:
            raise PC.Refused("export_streams is refused on an engine with input classes")
        self._flush()
        return self._records(ids, cache)

    def records(self, ids):
        self._flush()
        return self._records(ids, True)

    def _records(self, ids, cache):
        import torch
        from vap_realtime_amd import engine as E
        T = self.T
        rec = np.zeros((len(ids), E.state_record_floats(T, cache, input_hz=self.hz)), np.float32)
        d = E.split_state(rec, T, input_hz=self.hz)
        zero = torch.zeros(2, 768, dtype=self.o.dtype)
        for b, s in enumerate(int(v) for v in ids):
            fs, n = self.seen[s], min(self.seen[s], T)
            d["n_frames"][b] = n
            if self.hz != 16000:
                d["resample_hist"][b], d["resample_started"][b] = np.stack([r["hist"] for r in self.rs[s]]), 3 if self._started(s) else 0
            d["lstm"][b][:, 0], d["lstm"][b][:, 1] = self.h[s].numpy(), self.c[s].numpy()
            d["carry"][b] = self.carry[s]
            for t, r in enumerate(self._window(s)):
                d["ring"][b][:, t] = r.numpy()
                if cache:
                    d["cache"][b][:, t] = self.qkv[s].get((fs - n + t) % T, zero).numpy()
        return rec

    def import_(self, ids, rec, cache, device):
        import torch
        from vap_realtime_amd import engine as E
        if self.table:
            raise PC.Refused("import_streams is refused on an engine with input classes")
        late = self._flush(late_for=tuple(int(v) for v in ids))
        d = E.split_state(np.asarray(rec), self.T, input_hz=self.hz)
        assert (d["cache"] is not None) == bool(cache)
        for b, s in enumerate(int(v) for v in ids):
            n = int(d["n_frames"][b])
            if self.hz != 16000:
                self.rs[s] = [{"hist": d["resample_hist"][b][ch].astype(np.float64), "started": bool(d["resample_started"][b])} for ch in range(2)]
                if self.fault == "history_lost_on_import":
                    if self._started(s):
                        self._hit()
                    self.rs[s] = self._fresh_input(s)
            rows = [torch.from_numpy(d["ring"][b][:, t].copy()).to(self.o.dtype) for t in range(n)]
            self.ring[s] = dict(enumerate(rows))
            if cache:
                self.qkv[s] = {t: torch.from_numpy(d["cache"][b][:, t].copy()).to(self.o.dtype) for t in range(n)}
            elif self.fault == "stale_cache":
                if n:
                    self._hit()
            else:
                self.qkv[s] = {t: qkv_rows(self.o, r) for t, r in enumerate(rows)}
            self.seen[s] = n
            self.append_at.pop(s, None)
            self.h[s] = torch.from_numpy(d["lstm"][b][:, 0].copy()).to(self.o.dtype)
            self.c[s] = torch.from_numpy(d["lstm"][b][:, 1].copy()).to(self.o.dtype)
            self.carry[s] = d["carry"][b]
        for q in late:
            self._apply(q)

    def prefill(self, audio, ids, device):
        if self.decoded:
            raise PC.Refused("prefill is refused on an engine with an input-class table, an input rate or an input format")
        late = self._flush(late_for=tuple(int(v) for v in ids))
        hop = self.hop
        for k, s in enumerate(int(v) for v in ids):
            zero = self.fault == "prefill_from_zero_carry" and self.seen[s] > 0 and self.carry[s].any()
            if zero:
                self._hit()
            for f in range(audio.shape[2] // hop):
                _, e = self._encode(s, audio[k][:, f * hop:(f + 1) * hop], zero_carry=zero and f == 0)
                self._append(s, e)
        for q in late:
            self._apply(q)
        self._e = None

    # -- bystanders
    def _bystander(self):
        if self.fault == "bystander_advances":
            live = [s for s in range(len(self.seen)) if self.seen[s] and -s - 1 not in self.pending and s not in self.pending]
            if live:
                self._hit()
                self.h[live[0]] = self.h[live[0]] * 1.01 + 1e-3

    def maps(self, n, rows, seed):
        self._bystander()

    def encode_free(self, s, seed):
        self._flush()
        self._encode(s, np.random.default_rng(seed).standard_normal((2, self.hop)).astype(np.float32) * 0.1)
        self.carry[s] = 0                                                                  # vapx_encode_audio takes whole frames: no carry
        self._bystander()
        self._e = None

    def peek_e(self, n):
        self._flush()
        return np.array(self._e[:n], np.float32)


# ---- trunk groups ---------------------------------------------------------------------------------------------------------------------------
class GroupPort:
    """What the runner calls, on a ``vap_realtime_amd.engine.TrunkGroup``: ``step`` and ``step_wire``, the leader's reset, group records."""

    def __init__(self, grp):
        self.grp, self.mark, self._out = grp, 0, None

    def step_begin(self, new, ids, route):
        from vap_realtime_amd import engine
        res = self.grp.step(new, ids) if route == "step" else self.grp.step_wire(new, ids)
        self._out = {}
        for m, rows in res.items():
            rows = np.array(rows)
            cols = engine.split_outputs(rows) if route == "step" else engine.split_wire(m, rows)
            self._out[m] = (cols, rows[:, engine.OUT_STATUS].astype(np.int32), ~np.delete(rows, engine.OUT_STATUS, axis=1).any(axis=1))

    def step_end(self):
        out, self._out = self._out, None
        return out

    def reset_stream(self, s):
        self.grp.reset_stream(int(s))

    def export(self, ids, cache, device):
        return self.grp.export_streams(ids, cache)

    def import_(self, ids, rec, cache, device):
        self.grp.import_streams(ids, rec, cache)

    def refused(self, what, s):
        from vap_realtime_amd import engine
        assert what == "export"
        try:
            self.grp.export_streams([int(s)])
        except engine.VapxError as ex:
            return str(ex)
        return None

    def group_states(self, ids):
        """{model: the fields ``split_state`` names}: from records with cache, or from ``get_state`` where a slower follower refuses export."""
        from vap_realtime_amd import engine
        grp, lead = self.grp, self.grp.order[0]
        if all(r == 1 for r in grp.R.values()):
            rec = grp.export_streams(ids, cache=True)
            return {m: engine.split_state(rec[m], grp.T_of[m], follower=m != lead) for m in grp.modes}
        out = {}
        for m in grp.modes:
            got = [grp.engines[m].get_state(int(s)) for s in ids]
            out[m] = {"n_frames": np.array([g["n_frames"] for g in got]), "ring": np.stack([g["ring"] for g in got]),
                      "lstm": np.stack([g["lstm"] for g in got]) if m == lead else None,
                      "carry": np.stack([g["carry"] for g in got]) if m == lead else None}
        return out


class GroupStandIn:
    """``GroupPort``'s methods at slot level: one ``StandIn`` per model on that model's own oracle (window, LSTM, carry at its own rate),
    and on top of them what the group adds: the leader's queue of resets, applied to every model, and per (model, slot) the leader hops
    collected towards the model's next frame.  ``fault``: "follower_phase_survives_reset" or "late_reset"."""

    def __init__(self, oracles: dict, prog: Program, fault: Optional[str] = None):
        p = prog.profile
        self.group, self.fault = p.group, fault
        self.R = {m: p.hz // hz for m, hz, _ in p.group}
        self.inner = {m: StandIn(oracles[m], prog._replace(profile=p._replace(hz=hz, T=T, mode=m, group=())), None) for m, hz, T in p.group}
        self.acc = {m: [[] for _ in range(prog.slots)] for m, _, _ in p.group}
        self.pending: List[int] = []
        self.mark, self.fault_mark, self._out = 0, None, None

    def _hit(self):
        if self.fault_mark is None:
            self.fault_mark = self.mark

    def reset_stream(self, s):
        if s not in self.pending:
            self.pending.append(s)

    def _apply(self, s):
        for m in self.inner:
            self.inner[m]._apply(s)
            if self.fault == "follower_phase_survives_reset" and self.R[m] > 1:
                if self.acc[m][s]:
                    self._hit()
                continue
            self.acc[m][s] = []

    def _flush(self, late_for=()):
        todo, self.pending = self.pending, []
        late = [s for s in todo if self.fault == "late_reset" and s in late_for]
        for s in todo:
            if s in late:
                self._hit()
            else:
                self._apply(s)
        return late

    def step_begin(self, new, ids, route):
        self._flush()
        ids = [int(v) for v in ids]
        n = len(ids)
        self._out = {}
        for m in self.inner:
            due, frames = [], []
            for k, s in enumerate(ids):
                self.acc[m][s].append(np.asarray(new[k], np.float32))
                if len(self.acc[m][s]) >= self.R[m]:
                    due.append(k)
                    frames.append(np.concatenate(self.acc[m][s][-self.R[m]:], axis=1))
                    self.acc[m][s] = []
            status, cols = np.full(n, 2, np.int32), {}
            if due:
                self.inner[m].step_begin(np.stack(frames), [ids[k] for k in due], "host")
                got = self.inner[m].step_end()
                for key, v in got.items():
                    cols[key] = np.zeros((n,) + v.shape[1:], v.dtype)
                    cols[key][due] = v
                cols["p_bc_rows"] = cols["logits"]
                status[due] = 0
            self._out[m] = (cols, status, status != 0)

    def step_end(self):
        out, self._out = self._out, None
        return out

    def export(self, ids, cache, device):
        slow = [m for m in self.inner if self.R[m] > 1]
        if slow:
            raise PC.Refused(f"export_streams is refused on a trunk follower at 1/{self.R[slow[0]]} of its leader's rate")
        self._flush()
        return {m: self.inner[m]._records(ids, cache) for m in self.inner}

    def import_(self, ids, rec, cache, device):
        late = self._flush(late_for=tuple(int(v) for v in ids))
        for m in self.inner:
            self.inner[m].import_(ids, rec[m], cache, False)
            for s in ids:
                self.acc[m][int(s)] = []
        for s in late:
            self._apply(s)

    def refused(self, what, s):
        try:
            self.export([s], False, False)
        except PC.Refused as ex:
            return str(ex)
        return None

    def group_states(self, ids):
        from vap_realtime_amd import engine as E
        self._flush()
        lead, out = self.group[0][0], {}
        for m, _, T in self.group:
            if all(r == 1 for r in self.R.values()):
                d = dict(E.split_state(self.inner[m]._records(ids, True), T))
            else:
                d = self.inner[m].states(ids)
            if m != lead:
                d["lstm"] = d["carry"] = None
            out[m] = d
        return out
