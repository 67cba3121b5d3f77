"""Memory bounds of every device path: the helper of tests/test_memory_bounds.py (CPU) and tests/test_memory_bounds_gpu.py, and the
entry of the child processes the GPU test starts.

    A  SCENARIOS      named runs of every path merged after the first guard-zone test, each under VAPX_GUARD_ZONES=1 (4 KiB canaries
                      round every device allocation of the engine, ``vapx_peek("guard_violations")``).  ``python tests/memory_bounds.py
                      GROUP`` runs one group in this process and prints one JSON line per scenario: name, guard_violations, the launch
                      counts of ``profile_read()`` and the scenario's own proofs.  The environment is read once per process, hence a child.
    B  Guarded        a caller-owned device buffer inside two margins of one NaN bit pattern; ``check_words`` is the checker, on numpy words.
    C  HIGH_SLOTS     engines whose top slots lie beyond 2^31 elements of the layer-0 Q|K|V ring and beyond 2^32 bytes of the context
                      ring: the same record and audio at slot 0 and at the probe slots must give the same bits.

Every kernel (``__global__`` in csrc/*.hip) is claimed by a scenario here, by the first guard-zone test (HYGIENE_KERNELS) or by a test
named in ELSEWHERE; tests/test_memory_bounds.py holds that list against the sources."""
import glob
import json
import os
import re
import sys
import time
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

# ---- B. the checker ---------------------------------------------------------------------------------------------------------------
PATTERN = 0x7FC5A5A5                     # a quiet NaN no arithmetic produces: the pre-fill of margins and payloads
MARGIN_BYTES = 4096                      # 1024 floats on each side


def check_words(words: np.ndarray, payload_words: int, margin_words: int = MARGIN_BYTES // 4, pattern: int = PATTERN,
                defined: bool = False, what: str = "") -> None:
    """``words``: the whole buffer as int32 / uint32 words, ``margin_words`` of ``pattern``, the payload, ``margin_words`` of
    ``pattern``.  Raises AssertionError if a margin word changed, or, with ``defined``, if a payload word still holds the pattern."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1)
    assert w.size == payload_words + 2 * margin_words, (what, w.size, payload_words, margin_words)
    pat = np.uint32(pattern)
    front, back = w[:margin_words], w[margin_words + payload_words:]
    for name, m, base in (("in front of", front, -margin_words), ("behind", back, payload_words)):
        bad = np.nonzero(m != pat)[0]
        if bad.size:
            raise AssertionError(f"{what}: {bad.size} words changed {name} the buffer, the first at payload word {base + int(bad[0])} "
                                 f"(0x{int(m[bad[0]]):08x})")
    if defined:
        left = np.nonzero(w[margin_words:margin_words + payload_words] == pat)[0]
        if left.size:
            raise AssertionError(f"{what}: {left.size} payload words were never written, the first at word {int(left[0])} of {payload_words}")


class Guarded:
    """A device buffer of ``shape`` / ``dtype`` (a torch dtype) inside two 4 KiB margins.  Margins and payload start as ``fill`` words;
    ``t`` is the inner view (16-byte aligned), ``check(defined)`` holds the margins against ``fill``."""

    def __init__(self, shape, dtype=None, fill: int = PATTERN, what: str = ""):
        import torch
        dtype = dtype or torch.float32
        self.what, self.fill = what, fill
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % 4 == 0, "payloads are whole 32-bit words"
        self.whole = torch.empty(self.nbytes + 2 * MARGIN_BYTES, dtype=torch.uint8, device="cuda")
        self.whole.view(torch.int32).fill_(int(np.uint32(fill).view(np.int32)))
        self.t = self.whole[MARGIN_BYTES:MARGIN_BYTES + self.nbytes].view(dtype).reshape(tuple(shape))
        assert self.t.data_ptr() % 16 == 0

    @classmethod
    def of(cls, array: np.ndarray, fill: int = PATTERN, what: str = ""):
        """An input: ``array`` inside margins of ``fill``."""
        import torch
        a = np.ascontiguousarray(array)
        g = cls(a.shape, torch.from_numpy(a[:0].copy()).dtype, fill, what)
        g.t.copy_(torch.from_numpy(a))
        return g

    def ptr(self) -> int:
        return self.t.data_ptr()

    def check(self, defined: bool = False):
        import torch
        torch.cuda.synchronize()
        check_words(self.whole.view(torch.int32).cpu().numpy(), self.nbytes // 4, pattern=self.fill, defined=defined, what=self.what)

    def numpy(self) -> np.ndarray:
        return self.t.cpu().numpy()


# ---- A. scenarios -----------------------------------------------------------------------------------------------------------------
class Scenario(NamedTuple):
    name: str
    group: str
    kernels: Tuple[str, ...]             # the __global__ kernels this scenario is there for
    prof: Tuple[str, ...]                # profile classes that must have been launched
    proofs: Tuple[str, ...]              # names of the proofs the scenario reports as true
    fn: Callable


SCENARIOS: List[Scenario] = []

# What the first guard-zone test steps (tests/test_hygiene_gpu.py::test_no_out_of_bounds_writes_around_any_engine_buffer): plain vap / nod /
# bc engines at T = 50 and 250, fp32, split, groups and the unfused chain
HYGIENE_KERNELS = ("conv0_kernel", "conv_tail_kernel", "lstm_kernel", "ring_append_kernel", "gather_ln_kernel", "attn_block_kernel",
                   "attention_long2_kernel", "attention_long_f16x3_kernel", "attention_proj_f16x3_kernel", "ffn_block_kernel",
                   "ffn_block_f16x3_kernel", "last_block_kernel", "gather_last_ln_kernel", "ln_rows_kernel", "attention_last_kernel",
                   "head_kernel", "gemm_f32_kernel", "window_meta_kernel", "add_kernel", "pbc_rows_kernel")
# kernels without an engine buffer, held by margins in a test of their own
ELSEWHERE = {"resample_whole_kernel": "tests/test_resample_gpu.py::test_whole_signal_kernel_against_float64 (guard floats behind the output)",
             "pcm_decode_kernel": "tests/test_memory_bounds_gpu.py::test_caller_buffers[pcm_decode]"}

CORE = ("conv0", "lstm", "gather_ln", "attention", "ffn_block", "head")
GROUPS = ("input", "classes", "state", "trunk", "windows", "level3")


def scenario(name, group, kernels=(), prof=CORE, proofs=()):
    def deco(fn):
        assert group in GROUPS and name not in [s.name for s in SCENARIOS], name
        SCENARIOS.append(Scenario(name, group, tuple(kernels), tuple(prof), tuple(proofs), fn))
        return fn
    return deco


def kernel_names(csrc: Optional[str] = None) -> List[str]:
    """Every ``__global__`` kernel of csrc/*.hip."""
    csrc = csrc or os.path.join(ROOT, "vap-realtime_amd", "csrc")
    names = set()
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
        with open(path) as f:
            text = f.read()
        names |= set(re.findall(r"__global__\s+(?:__launch_bounds__\s*\([^;{]*?\)\s*)?void\s+(\w+)\s*\(", text))
    return sorted(names)


def claims() -> Dict[str, List[str]]:
    """kernel -> who claims it."""
    out: Dict[str, List[str]] = {}
    for s in SCENARIOS:
        for k in s.kernels:
            out.setdefault(k, []).append(s.name)
    for k in HYGIENE_KERNELS:
        out.setdefault(k, []).append("tests/test_hygiene_gpu.py")
    for k, where in ELSEWHERE.items():
        out.setdefault(k, []).append(where)
    return out


_BLOBS: dict = {}


def blob(hz, mode="vap", seed=3, cpc_hz=None):
    """Synthetic weights; a trunk group's models share the CPC of ``cpc_hz``, the leader's rate."""
    from vap_realtime_amd import weights as W
    key = (hz, mode, seed, cpc_hz)
    if key not in _BLOBS:
        cpc, vap = W.synthetic_weights(seed, hz, mode)
        if cpc_hz is not None:
            cpc = W.synthetic_weights(41, cpc_hz, "vap")[0]
        _BLOBS[key] = W.pack_blob(cpc, vap, mode)
    return _BLOBS[key]


def ctx_sec(T, hz):
    return (T + 0.5) / hz


def noise(rng, shape, amp=0.1):
    return (amp * rng.uniform(-1, 1, shape)).astype(np.float32)


def audio_of(rng, fmt, n, samples):
    """[n, 2, samples] of format ``fmt``."""
    from vap_realtime_amd import pcm
    x = noise(rng, (n, 2, samples))
    return x if fmt == "f32" else pcm.encode(fmt, x)


def batch_ids(S, t):
    """Ragged, reordered, never a multiple of a tile, slots 0 and S - 1 on every tick (S odd, >= 5)."""
    assert S % 2 == 1 and S >= 5
    if t % 3 == 0:
        return np.arange(S, dtype=np.int32)[::-1].copy()
    if t % 3 == 1:
        return np.array([S - 1, 0, S // 2], dtype=np.int32)
    return np.roll(np.arange(S, dtype=np.int32), -2)


class Run:
    """One scenario's bookkeeping: every engine is created, read out (launch counts, canaries) and closed through it."""

    def __init__(self):
        self.launches: Dict[str, int] = {}
        self.violations = 0
        self.proofs: Dict[str, bool] = {}
        self.live: list = []

    def engine(self, *a, env: Optional[dict] = None, **kw):
        from vap_realtime_amd import engine
        env = {k: v for k, v in (env or {}).items() if v}
        saved = {k: os.environ.pop(k, None) for k in env}
        try:
            os.environ.update({k: "1" for k in env})             # debug knobs vapx_create reads once per engine
            e = engine.Engine(*a, **kw)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        return self.adopt(e)

    def adopt(self, e):
        e.profile_enable(range(16))
        self.live.append(e)
        return e

    def group(self, *a, **kw):
        from vap_realtime_amd import engine
        g = engine.TrunkGroup(*a, **kw)
        for m in g.order:
            self.adopt(g.engines[m])
        return g

    def finite(self, out, what=""):
        assert np.isfinite(np.asarray(out)).all(), f"non-finite output {what}"

    def prove(self, name, ok):
        self.proofs[name] = bool(ok) and self.proofs.get(name, True)

    def close(self):
        """Launch counts and canaries of every live engine, then close them, followers before leaders."""
        for e in self.live:
            for k, (_, cnt) in e.profile_read().items():
                self.launches[k] = self.launches.get(k, 0) + int(cnt)
        if self.live:
            v = float(self.live[0].peek("guard_violations", (1,))[0])    # every live allocation of the process
            self.violations = -1 if v < 0 else self.violations + int(v)
        for e in reversed(self.live):
            e.close()
        self.live = []


def drive(run, eng, ticks, fmt="f32", samples=None, seed=0, hooks=None, twin=None):
    """``ticks`` ragged reordered steps of seeded audio.  ``hooks[t](eng)`` runs before tick t.  ``twin``: an engine fed the same
    samples decoded to float32, whose rows must equal ``eng``'s bit for bit (returns whether they did)."""
    from vap_realtime_amd import pcm
    rng = np.random.default_rng(seed)
    samples = samples or eng.hop_in
    same = True
    for t in range(ticks):
        if hooks and t in hooks:
            hooks[t](eng)
            if twin is not None:
                hooks[t](twin)
        ids = batch_ids(eng.max_streams, t)
        a = audio_of(rng, fmt, len(ids), samples)
        out = eng.step(a, ids)
        run.finite(out, f"tick {t}")
        if twin is not None:
            same = same and np.array_equal(out, twin.step(pcm.decode(fmt, a), ids))
    return same


S7, T8 = 7, 8
PARITY = 1e-4                            # the project's parity bar between two routes to the same state (tests/test_state_bulk_gpu.py TOL)


# -- 1. input rate and format ---------------------------------------------------------------------------------------------------------
def _rate_scenario(in_hz, fr, T, **kw):
    def fn(run):
        from vap_realtime_amd import engine
        e = run.engine(blob(fr), fr, ctx_sec(T, fr), max_streams=S7, input_hz=in_hz, **kw)
        hooks = {T // 2 + 1: lambda x: x.reset_stream(S7 - 1), T + 1: lambda x: x.reset_carry(S7 - 1)}
        drive(run, e, T + 4, seed=in_hz + fr, hooks=hooks)
        s = engine.split_state(e.export_streams([0, S7 - 1]), T, input_hz=in_hz)
        run.prove("history_written", s["resample_hist"][0].any() and s["resample_hist"][1].any() and s["resample_started"].tolist() == [3, 3])
    return fn


for _hz in (8000, 32000, 48000):
    for _fr in (20, 50):
        _kw = {"split_f16": True} if (_hz, _fr) == (32000, 20) else {}
        scenario(f"rate_{_hz}_at_{_fr}hz" + ("_split" if _kw else ""), "input", ("input_classes_kernel", "reset_streams_kernel"),
                 proofs=("history_written",))(_rate_scenario(_hz, _fr, T8, **_kw))
scenario("rate_48000_at_5hz", "input", ("input_classes_kernel",), proofs=("history_written",))(_rate_scenario(48000, 5, 4))


def _format_scenario(fmt, full, **kw):
    def fn(run):
        fr = 20
        e = run.engine(blob(fr), fr, ctx_sec(T8, fr), max_streams=S7, input_format=fmt, **kw)
        twin = run.engine(blob(fr), fr, ctx_sec(T8, fr), max_streams=S7, **kw)
        hooks = {5: lambda x: x.reset_stream(S7 - 1), 9: lambda x: x.reset_carry(S7 - 1)}
        same = drive(run, e, T8 + 4, fmt=fmt, samples=e.L if full else e.hop, seed=len(fmt) + full, hooks=hooks, twin=twin)
        run.prove("equals_f32_engine_fed_decoded_samples", same)
    return fn


for _fmt in ("s16", "mulaw", "alaw"):
    for _full in (False, True):
        _kw = {"split_f16": True} if (_fmt, _full) == ("mulaw", False) else {}
        scenario(f"format_{_fmt}_{'full_frame' if _full else 'hop'}" + ("_split" if _kw else ""), "input",
                 ("input_classes_kernel", "reset_streams_kernel"), proofs=("equals_f32_engine_fed_decoded_samples",))(_format_scenario(_fmt, _full, **_kw))


# -- 2. input class tables ------------------------------------------------------------------------------------------------------------
TABLE = (("f32", 16000), ("mulaw", 8000), ("s16", 48000), ("alaw", 32000))


def _class_arrays(rng, eng, ids, fr):
    """Per batch slot: a [2, hop_in] array of the stream's class, or a pair of rows where its channels differ."""
    out = []
    for s in ids:
        c1, c2 = (int(c) for c in eng._cls[int(s)])
        rows = [audio_of(rng, TABLE[c][0], 1, TABLE[c][1] // fr)[0, 0] for c in (c1, c2)]
        out.append(np.stack(rows) if c1 == c2 else (rows[0], rows[1]))
    return out


def _classes_scenario(route, pairs, fr=20, **kw):
    def fn(run):
        import torch
        from vap_realtime_amd import engine

        def program(how):
            e = run.engine(blob(fr), fr, ctx_sec(T8, fr), max_streams=S7, input_classes=TABLE, **kw)
            rng = np.random.default_rng(77 + pairs)
            for s in range(S7):
                if pairs and s % 2:
                    e.set_stream_channel_classes(s, s % 4, (s + 1 + s // 4) % 4)
                else:
                    e.set_stream_class(s, s % 4)
            pin = engine.pinned_empty((S7 * 2 * max(e.input_row_bytes(c) for c in range(4)),), np.uint8)
            outs = []
            for t in range(T8 + 4):
                if t == 5:
                    e.set_stream_class(S7 - 1, 2)
                if t == 8:
                    e.set_stream_channel_classes(S7 - 1, 3, 1)
                ids = batch_ids(S7, t)
                arrays = _class_arrays(rng, e, ids, fr)
                if how == "pageable":
                    out = e.step(arrays, ids).copy()
                elif how == "pinned":
                    out = e.step(e.pack_input(ids, arrays, out=pin), ids).copy()
                else:
                    dev = torch.from_numpy(e.pack_input(ids, arrays).copy()).cuda()
                    d_out = torch.zeros((len(ids), engine.OUT_STRIDE), device="cuda")
                    e.step_packed_device(ids, dev.data_ptr(), d_out.data_ptr())
                    torch.cuda.synchronize()
                    out = d_out.cpu().numpy()
                run.finite(out, f"{how} tick {t}")
                outs.append(out)
            return outs
        got, want = program(route), program("pageable" if route != "pageable" else "pinned")
        run.prove("routes_agree_bit_for_bit", all(np.array_equal(a, b) for a, b in zip(got, want)))
    return fn


for _route in ("pageable", "pinned", "packed_device"):
    for _pairs in (0, 1):
        _kw = {"split_f16": True} if (_route, _pairs) == ("pinned", 1) else {}
        scenario(f"classes_{_route}" + ("_channel_pairs" if _pairs else "") + ("_split" if _kw else ""), "classes",
                 ("input_classes_kernel", "reset_streams_kernel"), proofs=("routes_agree_bit_for_bit",))(_classes_scenario(_route, _pairs, **_kw))


# -- 3. state I/O ---------------------------------------------------------------------------------------------------------------------
STATE_KERNELS = ("state_export_kernel", "state_import_kernel", "state_ln_kernel", "state_cache_scatter_kernel")
PERM_FROM, PERM_TO = (S7 - 1, 0, 3), (0, S7 - 1, 2)


def _state_scenario(route, cache, small_stage=False, in_hz=16000, fr=20, T=T8, **kw):
    def fn(run):
        import torch
        from vap_realtime_amd import engine
        mk = lambda: run.engine(blob(fr), fr, ctx_sec(T, fr), max_streams=S7, input_hz=in_hz, **kw)
        a, b, c = mk(), mk(), mk()
        drive(run, a, T + 4, seed=in_hz + cache)
        fl = a.state_floats(cache)
        if small_stage:
            os.environ["VAPX_STATE_STAGE_FLOATS"] = str(2 * fl)                 # 7 records in four blocks
        try:
            if route == "host":
                rec = a.export_streams(None, cache=cache)
                b.import_streams(None, rec, cache=cache)
                part = a.export_streams(PERM_FROM, cache=cache)
                c.import_streams(PERM_TO, part, cache=cache)
                back, back_part = b.export_streams(None, cache=cache), c.export_streams(PERM_TO, cache=cache)
            else:
                d_rec, d_back = torch.zeros(S7, fl, device="cuda"), torch.zeros(S7, fl, device="cuda")
                d_part, d_back_part = torch.zeros(3, fl, device="cuda"), torch.zeros(3, fl, device="cuda")
                d_from, d_to = (torch.tensor(p, dtype=torch.int32, device="cuda") for p in (PERM_FROM, PERM_TO))
                a.export_streams_device(S7, d_rec.data_ptr(), cache=cache)
                b.import_streams_device(S7, d_rec.data_ptr(), cache=cache)
                a.export_streams_device(3, d_part.data_ptr(), ids_ptr=d_from.data_ptr(), cache=cache)
                c.import_streams_device(3, d_part.data_ptr(), ids_ptr=d_to.data_ptr(), cache=cache)
                b.export_streams_device(S7, d_back.data_ptr(), cache=cache)
                c.export_streams_device(3, d_back_part.data_ptr(), ids_ptr=d_to.data_ptr(), cache=cache)
                torch.cuda.synchronize()
                rec, back, part, back_part = (t.cpu().numpy() for t in (d_rec, d_back, d_part, d_back_part))
                run.prove("device_route_equals_host_route", np.array_equal(rec, a.export_streams(None, cache=cache)))
        finally:
            os.environ.pop("VAPX_STATE_STAGE_FLOATS", None)
        run.finite(rec)
        s = engine.split_state(rec, T, input_hz=in_hz)
        run.prove("records_round_trip", np.array_equal(rec, back) and np.array_equal(part, back_part) and np.array_equal(part, rec[list(PERM_FROM)])
                  and s["n_frames"][[0, S7 - 1]].tolist() == [T, T] and s["n_frames"].all() and s["ring"].any())
        if in_hz != 16000:
            run.prove("history_exported", all(s["resample_hist"][k].any() for k in range(S7)))
        # the next 4 steps of the importing engine are those of the uninterrupted one: bit for bit where the cache travelled; where it was
        # rebuilt (another batch shape of the same GEMMs) to the project's parity bar of 1e-4, as tests/test_state_bulk_gpu.py holds it
        rng = np.random.default_rng(5)
        same = True
        for t in range(4):
            x = noise(rng, (S7, 2, a.hop_in))
            want, got = a.step(x), b.step(x)
            same = same and (np.array_equal(got, want) if cache else bool(np.abs(got - want).max() <= PARITY))
            run.finite(c.step(x[list(PERM_FROM)], PERM_TO))
            run.finite(want)
        run.prove("next_4_steps_match", same)
    return fn


for _route in ("host", "device"):
    for _cache in (False, True):
        scenario(f"state_{_route}" + ("_cache" if _cache else ""), "state", STATE_KERNELS,
                 proofs=("records_round_trip", "next_4_steps_match") + (("device_route_equals_host_route",) if _route == "device" else ()))(
            _state_scenario(_route, _cache))
scenario("state_host_small_staging", "state", STATE_KERNELS, proofs=("records_round_trip", "next_4_steps_match"))(
    _state_scenario("host", False, small_stage=True))
scenario("state_host_cache_small_staging_split", "state", STATE_KERNELS, proofs=("records_round_trip", "next_4_steps_match"))(
    _state_scenario("host", True, small_stage=True, split_f16=True))
for _hz in (8000, 32000, 48000):
    scenario(f"state_rate_{_hz}", "state", STATE_KERNELS, proofs=("records_round_trip", "next_4_steps_match", "history_exported"))(
        _state_scenario("host" if _hz != 32000 else "device", True, in_hz=_hz))
scenario("state_long_window_T70", "state", STATE_KERNELS, proofs=("records_round_trip", "next_4_steps_match"))(
    _state_scenario("host", False, fr=50, T=70))


@scenario("state_get_set_last_slot", "state", STATE_KERNELS, proofs=("state_moves",))
def _get_set(run):
    fr = 20
    a = run.engine(blob(fr), fr, ctx_sec(T8, fr), max_streams=S7)
    b = run.engine(blob(fr), fr, ctx_sec(T8, fr), max_streams=S7)
    drive(run, a, T8 + 4, seed=1)
    st = a.get_state(S7 - 1)
    b.set_state(S7 - 1, st)
    b.set_state(0, a.get_state(0))
    back = b.get_state(S7 - 1)
    ok = back["n_frames"] == st["n_frames"] == T8 and all(np.array_equal(back[k], st[k]) for k in ("ring", "lstm", "carry"))
    x = noise(np.random.default_rng(2), (2, 2, a.hop))
    for _ in range(3):
        want = a.step(x, [S7 - 1, 0])
        ok = ok and bool(np.abs(b.step(x, [S7 - 1, 0]) - want).max() <= PARITY)      # set_state rebuilds the cache
        run.finite(want)
    run.prove("state_moves", ok)


@scenario("state_trunk_group", "state", STATE_KERNELS, proofs=("group_records_round_trip",))
def _state_group(run):
    fr = 20
    blobs = {m: blob(fr, m, seed=40 + i, cpc_hz=fr) for i, m in enumerate(("vap", "bc", "nod"))}
    T_of = {"vap": 8, "bc": 11, "nod": 6}
    mk = lambda: run.group(blobs, fr, {m: ctx_sec(T, fr) for m, T in T_of.items()}, max_streams=S7)
    g, h = mk(), mk()
    rng = np.random.default_rng(3)
    for t in range(15):
        ids = batch_ids(S7, t)
        for rows in g.step(noise(rng, (len(ids), 2, g.hop)), ids).values():
            run.finite(rows)
    ok = True
    for cache in (False, True):
        rec = g.export_streams(PERM_FROM, cache=cache)
        h.import_streams(PERM_TO, rec, cache=cache)
        back = h.export_streams(PERM_TO, cache=cache)
        ok = ok and all(np.array_equal(rec[m], back[m]) and rec[m].any() for m in g.modes)
        x = noise(rng, (3, 2, g.hop))
        want, got = g.step(x, PERM_FROM), h.step(x, PERM_TO)
        ok = ok and all(np.array_equal(want[m], got[m]) if cache else bool(np.abs(want[m] - got[m]).max() <= PARITY) for m in g.modes)
    run.prove("group_records_round_trip", ok)


# -- 4. trunk groups ------------------------------------------------------------------------------------------------------------------
TRUNK_KERNELS = ("trunk_collect_kernel", "out_scatter_kernel", "wire_pack_kernel")


def _trunk_scenario(spec, api, **kw):
    """spec: {mode: (hz, T)}; the fastest leads.  Streams join one leader frame apart (S - 1 first, then 0, then the rest), the batch
    order flips every tick, and the last slot is reset once in the middle of a follower's frame."""
    def fn(run):
        import ctypes as C
        import torch
        from vap_realtime_amd import engine as E
        lead_hz = max(hz for hz, _ in spec.values())
        blobs = {m: blob(hz, m, seed=50 + i, cpc_hz=lead_hz) for i, (m, (hz, _)) in enumerate(spec.items())}
        g = run.group(blobs, {m: hz for m, (hz, _) in spec.items()}, {m: ctx_sec(T, hz) for m, (hz, T) in spec.items()}, max_streams=S7, **kw)
        Rmax = max(g.R.values())
        ticks = max(g.R[m] * (g.T_of[m] + 3) for m in g.modes) + S7
        join = [S7 - 1, 0] + list(range(1, S7 - 1))                              # stream join[k] steps from tick k on
        rng = np.random.default_rng(len(spec) + Rmax)
        seen = {m: set() for m in g.modes}
        for t in range(ticks):
            if t == Rmax + 1 and Rmax > 1:                                       # S - 1 has stepped Rmax + 1 times: one frame out, the next begun
                g.reset_stream(S7 - 1)
            ids = np.array(join[:t + 1], dtype=np.int32)
            ids = ids[::-1].copy() if t % 2 else ids
            if t % 5 == 4 and t >= S7:                                           # ragged: three of the seven
                ids = np.array([S7 - 1, 3, 0], dtype=np.int32)
            x = noise(rng, (len(ids), 2, g.hop))
            if api == "step":
                res = g.step(x, ids)
            elif api == "step_wire":
                res = g.step_wire(x, ids)
            else:
                n, per = len(ids), g.leader.group_wire_floats()
                dx = torch.from_numpy(x).cuda()
                wire = torch.zeros(n * per, device="cuda")               # a wire row's padding lanes are nobody's
                rc = g.leader.lib.vapx_step_group(g.leader._h, n, ids.ctypes.data_as(C.c_void_p), dx.data_ptr(), g.hop, wire.data_ptr(),
                                                  E.AUDIO_DEVICE | E.OUT_DEVICE, None)          # ids on the host: a slower follower needs them
                g.leader._check(rc, "vapx_step_group")
                torch.cuda.synchronize()
                block, res, at = wire.cpu().numpy(), {}, 0
                for m in g.order:
                    wf = g.wire_floats(m)
                    res[m] = block[at:at + n * wf].reshape(n, wf)
                    at += n * wf
            for m in g.modes:
                run.finite(res[m], f"{m} tick {t}")
                seen[m] |= set(res[m][:, E.OUT_STATUS].astype(int).tolist())
                if api != "step":
                    assert res[m].shape == (len(ids), g.wire_floats(m))
        slow = [m for m in g.modes if g.R[m] > 1]
        run.prove("no_frame_rows_and_frames", all(seen[m] == {0, E.STATUS_NO_FRAME} for m in slow) and all(seen[m] == {0} for m in g.modes if m not in slow))
    return fn


THREE = {"vap": (20, 6), "bc": (20, 9), "nod": (10, 5)}
for _api in ("step", "step_wire", "step_group_device"):
    for _split in (False, True):
        scenario(f"trunk_vap_bc_nod_{_api}" + ("_split" if _split else ""), "trunk", TRUNK_KERNELS + (("pbc_rows_kernel",) if _api != "step" else ()),
                 prof=CORE + ("trunk_collect",), proofs=("no_frame_rows_and_frames",))(_trunk_scenario(THREE, _api, split_f16=_split))
scenario("trunk_20_to_5_step_wire", "trunk", TRUNK_KERNELS, prof=CORE + ("trunk_collect",), proofs=("no_frame_rows_and_frames",))(
    _trunk_scenario({"bc": (20, 7), "vap": (5, 4)}, "step_wire"))
scenario("trunk_50_to_10_step", "trunk", TRUNK_KERNELS, prof=CORE + ("trunk_collect",), proofs=("no_frame_rows_and_frames",))(
    _trunk_scenario({"vap": (50, 9), "nod": (10, 4)}, "step"))
scenario("trunk_50_to_10_step_group_device_split", "trunk", TRUNK_KERNELS, prof=CORE + ("trunk_collect",), proofs=("no_frame_rows_and_frames",))(
    _trunk_scenario({"vap": (50, 9), "nod": (10, 4)}, "step_group_device", split_f16=True))


# -- 5. windows and variants ------------------------------------------------------------------------------------------------------------
def _window_scenario(hz, T, label, mode="vap", poison=False, force_xl=False, **kw):
    """The window is filled by ``set_state`` to T - 2 rows (ragged: slot 0 one row less), then stepped 5 ticks: it fills and rotates."""
    def fn(run):
        S = 5
        e = run.engine(blob(hz, mode), hz, ctx_sec(T, hz), max_streams=S, mode=mode,
                       env={"VAPX_POISON_SCRATCH": poison, "VAPX_FORCE_ATTENTION_XL": force_xl}, **kw)
        rng = np.random.default_rng(T)
        for s in range(S):
            n = max(T - 2 - (s == 0), 0)
            if n:
                ring = np.zeros((2, T, 256), np.float32)
                ring[:, :n] = np.tanh(rng.standard_normal((2, n, 256))).astype(np.float32)
                e.set_state(s, {"ring": ring, "n_frames": n, "lstm": noise(rng, (2, 2, 256)), "carry": noise(rng, (2, 320))})
        drive(run, e, 5 if T > 1 else 4, seed=T)
        run.prove("window_full", int(e.get_state(S - 1)["n_frames"]) == T and int(e.get_state(0)["n_frames"]) == T)
    return fn


def _variants(T):
    from test_layer_rows_gpu import base_variants
    v = [(x.label, x.poison, x.force_xl, x.kw) for x in base_variants(T)]
    if T == 65:                          # the long class: what base_variants gives T = 250
        v += [(x.label, x.poison, x.force_xl, x.kw) for x in base_variants(250) if x.label not in [l for l, *_ in v]]
    return v


WINDOW_T = {1: 20, 33: 50, 65: 50, 257: 50, 300: 50}        # T -> frame rate
LONG_KERNELS = ("attention_long2_kernel", "attention_long_f16x3_kernel", "attention_proj_f16x3_kernel", "ffn_block_f16x3_kernel")
for _T, _hz in WINDOW_T.items():
    for _label, _poison, _xl, _kw in _variants(_T):
        _k = ("attn_block_kernel",) if _T <= 64 else ("attention_xl_kernel",) if (_T > 256 or _xl) else LONG_KERNELS
        scenario(f"window_T{_T}_{_label}", "windows", _k, prof=("conv0", "lstm", "attention", "ffn_block", "head"), proofs=("window_full",))(
            _window_scenario(_hz, _T, _label, poison=_poison, force_xl=_xl, **_kw))
# at 5 Hz (K = 20 CPC frames per tick) the conv2-4 tail is the GEMM chain with the ChannelNorm + ReLU epilogue, not conv_tail_kernel
scenario("window_5hz_T6", "windows", ("gemm_f32_kernel", "conv0_kernel"), prof=CORE + ("gemm_cn_relu",), proofs=("window_full",))(
    _window_scenario(5, 6, "5hz"))
scenario("window_5hz_T6_split", "windows", ("gemm_f32_kernel", "conv0_kernel"), prof=CORE + ("gemm_cn_relu",), proofs=("window_full",))(
    _window_scenario(5, 6, "5hz_split", split_f16=True))
scenario("window_nod_T100", "windows", ("pbc_rows_kernel", "add_kernel"), proofs=("window_full",))(_window_scenario(10, 100, "nod", mode="nod"))
scenario("window_nod_T250_split", "windows", ("pbc_rows_kernel", "add_kernel") + LONG_KERNELS, proofs=("window_full",))(
    _window_scenario(50, 250, "nod_split", mode="nod", split_f16=True))       # nod rows hold one p_bc per window row: T <= 256


# -- 6. level-3 calls -----------------------------------------------------------------------------------------------------------------
LEVEL3_ROWS = (1, 33, 65, 250)
HEAD_ROWS = (1, 3, 37, 250)              # no multiple of 4 or 64 (rowdot / rowheads: 4 rows per workgroup)


class Plain:
    """The buffers of a level-3 call without margins (the engine's own canaries are what group 6 checks); Margins (below) is its twin."""

    def __init__(self):
        self.outs = []

    def inp(self, array, what="", ids_top=None):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array)).cuda()

    def out(self, what, shape, defined=True, dtype=None):
        import torch
        t = torch.full(tuple(shape), float("nan"), device="cuda") if dtype is None else torch.zeros(tuple(shape), dtype=dtype, device="cuda")
        self.outs.append((self._name(what), t, defined))
        return t

    def _name(self, what):
        """One call's outputs by name; a second call of the same case gets ``name#k``."""
        taken = [w for w, _, _ in self.outs]
        return what if what not in taken else f"{what}#{sum(w.split('#')[0] == what for w in taken)}"

    def results(self):
        import torch
        torch.cuda.synchronize()
        return {what: t.cpu().numpy() for what, t, _ in self.outs}


class Margins(Plain):
    """Every buffer of a call inside margins.  Inputs' margins hold ``in_fill`` words (the NaN pattern on the first run; zeros, or for
    ids the top stream id, on the second); outputs are pre-filled with the pattern throughout."""

    def __init__(self, in_fill: Optional[int]):
        super().__init__()
        self.in_fill = in_fill
        self.held = []

    def inp(self, array, what="", ids_top=None):
        fill = PATTERN if self.in_fill is None else (ids_top if ids_top is not None else self.in_fill)
        g = Guarded.of(array, fill, what)
        self.held.append(g)
        return g.t

    def out(self, what, shape, defined=True, dtype=None):
        what = self._name(what)
        g = Guarded(shape, dtype, PATTERN, what)
        self.outs.append((what, g, defined))
        return g.t

    def results(self):
        res = {}
        for what, g, defined in self.outs:
            g.check(defined)
            res[what] = g.numpy()
        for g in self.held:
            g.check()                                                            # a call writes to none of its inputs
        return res


def call_transformer(eng, bufs, n, rows, maps, stage=0, seed=0):
    x = bufs.inp(noise(np.random.default_rng(100 * rows + n + seed), (n, 2, rows, 256), 0.7), "x")
    t = {}
    if stage != 2:
        t["o"] = bufs.out("o", (n, 2, rows, 256))
    if stage != 1:
        t["x12"] = bufs.out("x12", (n, 2, rows, 256))
        t["comb"] = bufs.out("comb", (n, rows, 256))
    if maps and stage != 2:
        t["attn"] = bufs.out("attn", (n, 2, 1, 4, rows, rows))
    if maps and stage != 1:
        t["self_attn"] = bufs.out("self_attn", (n, 2, 3, 4, rows, rows))
        t["cross_attn"] = bufs.out("cross_attn", (n, 2, 3, 4, rows, rows))
    p = lambda k: t[k].data_ptr() if k in t else 0
    if maps:
        eng.transformer_maps_device(n, rows, x.data_ptr(), o_ptr=p("o"), x12_ptr=p("x12"), comb_ptr=p("comb"), stage=stage,
                                    attn_ptr=p("attn"), self_attn_ptr=p("self_attn"), cross_attn_ptr=p("cross_attn"))
    else:
        eng.transformer_device(n, rows, x.data_ptr(), o_ptr=p("o"), x12_ptr=p("x12"), comb_ptr=p("comb"), stage=stage)


def call_encode_audio(eng, bufs, n, ids=None, seed=0):
    frames = bufs.inp(noise(np.random.default_rng(n + seed), (n, 2, eng.L)), "frames")
    e = bufs.out("e", (n, 2, 256))
    eng.encode_audio_device(n, frames.data_ptr(), e.data_ptr(), stream_ids=ids)


def call_head(eng, bufs, which, rows, seed=0):
    """which: vap_head / va_classifier / bc_head / nod_head / softmax256 / aggregate."""
    rng = np.random.default_rng(rows + seed)
    lib = eng.lib
    if which == "aggregate":
        p = rng.uniform(0, 1, (rows, 256)).astype(np.float32)
        x = bufs.inp(p / p.sum(1, keepdims=True), "probs")
        y = bufs.out("aggregate", (rows, 2))
        rc = lib.vapx_aggregate(rows, x.data_ptr(), 0, 1, y.data_ptr(), None)
    else:
        x = bufs.inp(noise(rng, (rows, 256), 1.0), "x")
        if which == "vap_head":
            y = bufs.out(which, (rows, 256))
            rc = lib.vapx_vap_head(eng._h, rows, x.data_ptr(), y.data_ptr(), None)
        elif which == "va_classifier":
            y = bufs.out(which, (rows, 1))
            rc = lib.vapx_va_classifier(eng._h, rows, x.data_ptr(), y.data_ptr(), None)
        elif which == "softmax256":
            y = bufs.out(which, (rows, 256))
            rc = lib.vapx_softmax256(rows, x.data_ptr(), y.data_ptr(), None)
        else:
            nout = {("bc", "bc_head"): 3, ("nod", "bc_head"): 1, ("nod", "nod_head"): 4}[(eng.mode, which)]
            y = bufs.out(which, (rows, nout))
            rc = lib.vapx_aux_head(eng._h, 0 if which == "bc_head" else 1, rows, x.data_ptr(), y.data_ptr(), None)
    assert rc == 0, (which, rows, rc, lib.vapx_last_error(eng._h))


def _level3_engine(run_or_none, mode="vap", T=250, hz=50, n=3, **kw):
    from vap_realtime_amd import engine
    args = (blob(hz, mode), hz, ctx_sec(T, hz))
    kw = dict(max_streams=n, mode=mode, **kw)
    return run_or_none.engine(*args, **kw) if run_or_none is not None else engine.Engine(*args, **kw)


def _transformer_scenario(maps, **kw):
    def fn(run):
        e = _level3_engine(run, **kw)
        ok = True
        for rows in LEVEL3_ROWS:
            for stage in (0, 1, 2):
                b = Plain()
                call_transformer(e, b, 3, rows, maps, stage)
                res = b.results()
                for k, v in res.items():
                    run.finite(v, f"{k} rows={rows} stage={stage}")
                if maps:
                    ok = ok and all(np.allclose(res[k].sum(-1), 1.0, atol=1e-3) for k in ("attn", "self_attn", "cross_attn") if k in res)
        if maps:
            run.prove("map_rows_sum_to_one", ok)
    return fn


L3_PROF = ("gather_ln", "attention", "ffn_block")
scenario("level3_transformer_maps", "level3", ("attention_map_kernel", "compact_rows_kernel", "fill_int_kernel", "add_kernel"), prof=L3_PROF,
         proofs=("map_rows_sum_to_one",))(_transformer_scenario(True))
scenario("level3_transformer_maps_split", "level3", ("attention_map_kernel", "compact_rows_kernel", "fill_int_kernel"), prof=L3_PROF,
         proofs=("map_rows_sum_to_one",))(_transformer_scenario(True, split_f16=True))
scenario("level3_transformer", "level3", ("compact_rows_kernel", "fill_int_kernel", "add_kernel"), prof=L3_PROF)(_transformer_scenario(False))
scenario("level3_transformer_split", "level3", ("compact_rows_kernel", "fill_int_kernel"), prof=L3_PROF)(_transformer_scenario(False, split_f16=True))


@scenario("level3_encode_audio", "level3", ("conv0_kernel", "lstm_kernel"), prof=("conv0", "lstm"), proofs=("embeddings_differ_by_tick",))
def _encode(run):
    e = _level3_engine(run, T=8, hz=20, n=S7)
    seen = []
    for t, (n, ids) in enumerate(((S7, None), (3, [S7 - 1, 0, 3]), (S7, list(range(S7))[::-1]))):
        b = Plain()
        call_encode_audio(e, b, n, ids, seed=t)
        res = b.results()["e"]
        run.finite(res)
        seen.append(res[0].copy())
    run.prove("embeddings_differ_by_tick", not np.array_equal(seen[0], seen[2]) and np.abs(seen[0]).max() > 0)


@scenario("level3_heads", "level3", ("rowdot_kernel", "rowheads_kernel", "softmax256_kernel", "aggregate_kernel", "gemm_f32_kernel"), prof=(),
          proofs=("heads_defined",))
def _heads(run):
    engines = {m: _level3_engine(run, mode=m, T=8, hz=20, n=3) for m in ("vap", "bc", "nod")}
    ok = True
    for rows in HEAD_ROWS:
        for m, which in (("vap", "vap_head"), ("vap", "va_classifier"), ("bc", "bc_head"), ("nod", "bc_head"), ("nod", "nod_head"),
                         ("vap", "softmax256"), ("vap", "aggregate")):
            b = Plain()
            call_head(engines[m], b, which, rows)
            res = b.results()[which]
            run.finite(res, f"{which} rows={rows}")
            if which == "softmax256":
                ok = ok and np.allclose(res.sum(-1), 1.0, atol=1e-4)
    run.prove("heads_defined", ok)


# ---- C. high slots ----------------------------------------------------------------------------------------------------------------
class HighRow(NamedTuple):
    name: str
    hz: int
    T: int
    max_streams: int
    probes: Tuple[int, ...]
    split: bool


def _high(name, hz, T, S, probes):
    return [HighRow(f"high_{name}_fp32", hz, T, S, probes, False), HighRow(f"high_{name}_split", hz, T, S, probes, True)]


HIGH_SLOTS: List[HighRow] = (_high("xl_T512", 50, 512, 5632, (0, 2730, 2731, 5461, 5631))[:1]      # split runs the same kernel there
                             + _high("long_T250", 50, 250, 11264, (0, 5592, 5593, 11185, 11263))
                             + _high("short_T50", 20, 50, 56320, (0, 27962, 27963, 55925, 56319)))
HIGH_TRUNK = ("high_trunk_T250", 5632)   # passes 2^31 elements of ring_qkv, not 2^32


def alias_slots(T: int, slot: int) -> List[int]:
    """The slots in which an offset of ``slot`` would land if it were truncated to 32 bits: elements and bytes of the Q|K|V ring
    ([S][2][T][768]) and of the context ring ([S][2][T][256]).  Empty while every offset fits."""
    out = set()
    for width in (768, 256):
        per = 2 * T * width
        for unit in (1, 4):
            off = slot * per * unit
            if off >= 1 << 31:           # beyond a signed 32-bit offset: as unsigned it wraps from 2^32 on, as signed it is negative
                wrapped = off & 0xFFFFFFFF
                if wrapped != off:
                    out.add(wrapped // (per * unit))
    return sorted(out)


def probe_plan(row: "HighRow") -> Tuple[List[int], List[int]]:
    """(probes, aliases).  An alias is never itself a probe: where a probe of the table truncates onto one (the first slot beyond 2^31
    elements lands on slot 0), the table's probe stays, for the bit identity, and its neighbour one slot up, whose aliases are free,
    joins it for the alias check."""
    probes = list(row.probes)
    for p in row.probes:
        q = p
        while set(alias_slots(row.T, q)) & (set(probes) | {q}):
            q += 1
            assert q < row.max_streams - 1, (row.name, p)
        if q != p:
            probes.append(q)
    probes = sorted(set(probes))
    aliases = sorted({a for p in probes for a in alias_slots(row.T, p)} - set(probes))
    return probes, aliases


def high_record(eng, T, seed=9):
    """One stream's record built on the host: T - 1 seeded window rows, a seeded LSTM state and carry, no cache."""
    from vap_realtime_amd import engine
    rec = eng.export_streams([0], cache=False).copy()                            # a fresh slot: the header of this engine
    s = engine.split_state(rec, T)
    rng = np.random.default_rng(seed)
    s["n_frames"][:] = T - 1
    s["ring"][0, :, :T - 1] = np.tanh(rng.standard_normal((2, T - 1, 256))).astype(np.float32)
    s["lstm"][0] = noise(rng, (2, 2, 256), 0.3)
    s["carry"][0] = noise(rng, (2, 320))
    return rec


def run_high(row: HighRow) -> dict:
    import torch
    from vap_realtime_amd import engine
    t0 = time.time()
    free0 = torch.cuda.mem_get_info()[0]
    T, S = row.T, row.max_streams
    eng = engine.Engine(blob(row.hz), row.hz, ctx_sec(T, row.hz), max_streams=S, max_batch=2, split_f16=row.split)   # a refusal is a failure
    used = free0 - torch.cuda.mem_get_info()[0]
    selftest = float(eng.peek("guard_selftest", (1,))[0])
    rec = high_record(eng, T)
    audio = noise(np.random.default_rng(4), (3, 1, 2, eng.hop))
    probes, aliases = probe_plan(row)
    assert aliases and not set(aliases) & set(probes), (aliases, probes)
    assert probes[0] == 0 and probes[-1] == S - 1
    proofs = {}

    def fresh(ids):
        r = eng.export_streams(ids, cache=True)
        s = engine.split_state(r, T)
        return not s["n_frames"].any() and not r[:, engine.STATE_HEADER_FLOATS:].any()

    def probe_all():
        rows, recs, states = {}, {}, {}
        for p in probes:
            eng.reset_stream(p)
            eng.import_streams([p], rec, cache=False)                            # the batched rebuild writes the slot's Q|K|V rows
            rows[p] = np.stack([eng.step(audio[t], [p])[0].copy() for t in range(3)])
            assert np.isfinite(rows[p]).all(), p
            recs[p] = eng.export_streams([p], cache=True).copy()
            states[p] = eng.get_state(p)
        ok = all(np.array_equal(rows[p].view(np.uint32), rows[0].view(np.uint32)) for p in probes)
        ok_rec = all(np.array_equal(recs[p].view(np.uint32), recs[0].view(np.uint32)) for p in probes)
        ok_get = all(states[p]["n_frames"] == T and all(np.array_equal(states[p][k], states[0][k]) for k in ("ring", "lstm", "carry")) for p in probes)
        return ok, ok_rec, ok_get, rows, recs

    proofs["aliases_fresh_before"] = fresh(aliases)
    ok, ok_rec, ok_get, rows, recs = probe_all()
    proofs["rows_bit_identical_to_slot_0"] = ok
    proofs["records_bit_identical_to_slot_0"] = ok_rec
    proofs["get_state_identical_to_slot_0"] = ok_get
    proofs["window_rotated"] = bool(engine.split_state(recs[0], T)["n_frames"][0] == T and rows[0][:, engine.OUT_NVALID].tolist() == [T, T, T])
    proofs["aliases_fresh_after"] = fresh(aliases)
    # a cached record of one probe into another (state_import_kernel with the cache at high slots), both stepped on
    ok = True
    for src, dst in ((probes[-1], probes[1]), (probes[2], probes[-2]), (probes[-2], 0)):
        eng.import_streams([dst], recs[src], cache=True)
        eng.import_streams([src], recs[src], cache=True)
        a, b = eng.step(audio[0], [src])[0].copy(), eng.step(audio[0], [dst])[0].copy()
        ok = ok and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.isfinite(a).all()
    proofs["cached_import_between_probes"] = ok
    # beyond the issue's alias check (an export shows nothing of a slot without frames): the aliases hold a full cached window of their
    # own while the probes run again, and keep every bit of it
    full = recs[0].copy()
    eng.import_streams(aliases, np.repeat(full, len(aliases), axis=0), cache=True)
    before = eng.export_streams(aliases, cache=True).copy()
    ok2 = probe_all()[:3]
    proofs["second_pass_identical"] = all(ok2)
    proofs["full_aliases_keep_their_bits"] = np.array_equal(before.view(np.uint32), eng.export_streams(aliases, cache=True).view(np.uint32))
    v = float(eng.peek("guard_violations", (1,))[0])
    eng.close()
    proofs = {k: bool(ok) for k, ok in proofs.items()}
    return {"name": row.name, "guard_selftest": selftest, "guard_violations": int(v), "proofs": proofs, "device_bytes": int(used),
            "probes": probes, "aliases": aliases, "seconds": round(time.time() - t0, 2)}


def run_high_trunk() -> dict:
    import torch
    from vap_realtime_amd import engine
    t0 = time.time()
    name, S = HIGH_TRUNK
    T = 250
    free0 = torch.cuda.mem_get_info()[0]
    blobs = {"vap": blob(20, "vap", 60, cpc_hz=20), "nod": blob(10, "nod", 61, cpc_hz=20)}
    g = engine.TrunkGroup(blobs, {"vap": 20, "nod": 10}, {"vap": ctx_sec(T, 20), "nod": ctx_sec(T, 10)}, max_streams=S, max_batch=2)
    used = free0 - torch.cuda.mem_get_info()[0]
    selftest = float(g.leader.peek("guard_selftest", (1,))[0])
    audio = noise(np.random.default_rng(6), (4, 1, 2, g.hop))
    got = {}
    for sid in (S - 1, 0):
        got[sid] = [g.step(audio[t], [sid]) for t in range(4)]
    same = all(np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32)) for a, b in zip(got[S - 1], got[0]) for m in g.modes)
    status = [int(r["nod"][0, engine.OUT_STATUS]) for r in got[S - 1]]
    finite = all(np.isfinite(r[m]).all() for r in got[S - 1] for m in g.modes)
    v = float(g.leader.peek("guard_violations", (1,))[0])
    g.close()
    return {"name": name, "guard_selftest": selftest, "guard_violations": int(v), "device_bytes": int(used),
            "proofs": {"vap_and_nod_rows_bit_equal": same and finite, "nod_frames_every_second_tick": status == [2, 0, 2, 0]},
            "seconds": round(time.time() - t0, 2)}


# ---- the child ------------------------------------------------------------------------------------------------------------------------
def run_group(group: str) -> int:
    from vap_realtime_amd import engine
    probe = engine.Engine(blob(20), 20, ctx_sec(4, 20), max_streams=1)
    st = float(probe.peek("guard_selftest", (1,))[0])
    after = float(probe.peek("guard_violations", (1,))[0])
    probe.close()
    print(json.dumps({"name": "guard_selftest", "group": group, "guard_selftest": st, "guard_violations": after}), flush=True)
    for s in SCENARIOS:
        if s.group != group:
            continue
        run, t0, err, stop = Run(), time.time(), None, False
        try:
            s.fn(run)
        except AssertionError as e:                                              # a check of the scenario: reported, the device is fine
            err = f"AssertionError: {e}"[:600]
        except Exception as e:                                                   # noqa: BLE001 - an error code of the library or worse:
            err, stop = f"{type(e).__name__}: {e}"[:600], True                   # nothing more is started on the device
        if not stop:
            run.close()
        print(json.dumps({"name": s.name, "group": group, "guard_violations": run.violations, "launches": run.launches,
                          "proofs": run.proofs, "error": err, "seconds": round(time.time() - t0, 2)}), flush=True)
        if stop:
            return 3
    return 0


def main(argv: Sequence[str]) -> int:
    if len(argv) != 1:
        print(f"usage: memory_bounds.py GROUP   ({', '.join(GROUPS)}, a high-slot row or {HIGH_TRUNK[0]})", file=sys.stderr)
        return 2
    what = argv[0]
    if what in GROUPS:
        return run_group(what)
    if what == HIGH_TRUNK[0]:
        print(json.dumps(run_high_trunk()), flush=True)
        return 0
    for row in HIGH_SLOTS:
        if row.name == what:
            print(json.dumps(run_high(row)), flush=True)
            return 0
    print(f"unknown group {what!r}", file=sys.stderr)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
