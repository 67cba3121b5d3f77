"""Every newer device path held to its buffers (tests/memory_bounds.py has the scenarios, the checker and the child's entry).

A. Engine-owned buffers under VAPX_GUARD_ZONES=1, one child process per group, one JSON line per scenario: ``guard_selftest`` says 1
   (the counter can count), every scenario's ``guard_violations`` is 0, its claimed profile classes were launched, its proofs are true.
     input    rate_{8000,32000,48000}_at_{20,50}hz (32 kHz at 20 Hz split), rate_48000_at_5hz, format_{s16,mulaw,alaw}_{hop,full_frame}
              (mulaw hop split); reset_stream and reset_carry of the last slot in mid-run
     classes  classes_{pageable,pinned,packed_device}[_channel_pairs]: the four-class table f32@16k, mulaw@8k, s16@48k, alaw@32k,
              set_stream_class and set_stream_channel_classes on the last slot in mid-run; every route against another, bit for bit
     state    state_{host,device}[_cache], state_host_small_staging, state_host_cache_small_staging_split, state_rate_{8000,32000,48000}
              (cache; the next 4 steps bit-identical), state_long_window_T70, state_get_set_last_slot, state_trunk_group
     trunk    trunk_vap_bc_nod_{step,step_wire,step_group_device}[_split] (20, 20, 10 Hz, windows 6, 9, 5), trunk_20_to_5_step_wire,
              trunk_50_to_10_step, trunk_50_to_10_step_group_device_split; streams join one leader frame apart, a reset in mid-frame
     windows  window_T{1,33,65,257,300}_<variant of test_layer_rows_gpu.base_variants; T = 65 also the long-window variants of T = 250>,
              window_5hz_T6[_split], window_nod_T100, window_nod_T250_split; filled by set_state, then 5 ticks
     level3   level3_transformer_maps[_split], level3_transformer[_split] (rows 1, 33, 65, 250, stages 0, 1, 2), level3_encode_audio,
              level3_heads (rows 1, 3, 37, 250)
B. Caller-owned buffers: every output inside two 4 KiB margins of one NaN pattern, every device input inside margins that hold NaNs on
   the first run and zeros (ids: the top stream id) on the second; the margins stay, the two runs agree bit for bit, promised rows are
   fully written.
C. High slots, one child per engine: T = 512 x 5 632 slots (fp32), T = 250 x 11 264 and T = 50 x 56 320 (fp32 and split), and a vap + nod
   trunk group at T = 250 x 5 632; slot 0 against the slots round 2^31 and 2^32 elements of the Q|K|V ring and the last slot.

If a child ends abnormally (a signal, an abort, a timeout), that test fails and every later test of this module fails at once without
starting another GPU process.

Measured on an MI355X, MEASURED below: the wall time of every child from start to exit (2.5 .. 4.9 s, of which about 2.3 s are the
interpreter and its imports), its slowest scenario (0.71 s, trunk_vap_bc_nod_step, the first of its child: every other scenario is
below 0.3 s, most below 0.1 s; a high-slot child spends 0.5 .. 1.2 s between create and close) and the device memory of each high-slot
engine (23.4 .. 24.0 GB; the trunk group's two models together 23.5 GB).  The whole module: 84 tests in 41 s, the 72 caller-buffer cases
below 0.7 s each.  The children's timeouts are three times the measured times, rounded up to a multiple of 10 s."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import memory_bounds as mb

pytestmark = pytest.mark.gpu

# child -> (wall seconds measured on an MI355X, slowest scenario and its seconds, device GB of the engine for the high-slot rows)
MEASURED = {
    "input": (3.3, "rate_8000_at_50hz", 0.21, None), "classes": (3.1, "classes_packed_device", 0.08, None),
    "state": (4.0, "state_trunk_group", 0.64, None), "trunk": (4.9, "trunk_vap_bc_nod_step", 0.71, None),
    "windows": (3.6, "window_T33_fp32", 0.20, None), "level3": (3.3, "level3_transformer_maps", 0.28, None),
    "high_xl_T512_fp32": (3.3, "", 1.16, 23.95), "high_long_T250_fp32": (2.8, "", 0.92, 23.40), "high_long_T250_split": (2.5, "", 0.53, 23.40),
    "high_short_T50_fp32": (2.7, "", 0.52, 23.69), "high_short_T50_split": (2.5, "", 0.52, 23.69), "high_trunk_T250": (2.8, "", 0.62, 23.52),
}
ABNORMAL = {"by": None}                  # the child that faulted: nothing more is started on the GPU from this module


def _timeout(what):
    return int(-(-3 * MEASURED[what][0] // 10) * 10)


def _child(what):
    """Run ``python tests/memory_bounds.py what`` with guard zones on; returns its JSON lines."""
    if ABNORMAL["by"]:
        pytest.fail(f"not started: the child {ABNORMAL['by']!r} of this module ended abnormally before")
    env = dict(os.environ, VAPX_GUARD_ZONES="1")
    cmd = [sys.executable, os.path.join(mb.HERE, "memory_bounds.py"), what]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=_timeout(what), env=env, cwd=mb.ROOT)
    except subprocess.TimeoutExpired as e:
        ABNORMAL["by"] = what
        pytest.fail(f"child {what!r} did not end within {_timeout(what)} s; its output so far:\n{str(e.stdout or '')[-3000:]}")
    print(r.stdout)
    if r.returncode != 0:               # a signal (< 0), an abort (134), a segmentation fault (139), or the child's own "stop" (3)
        ABNORMAL["by"] = what
        pytest.fail(f"child {what!r} ended abnormally (return code {r.returncode}):\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


# ---- A ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", mb.GROUPS)
def test_engine_buffers_under_guard_zones(group):
    lines = _child(group)
    by_name = {d["name"]: d for d in lines}
    st = by_name.pop("guard_selftest")
    assert st["guard_selftest"] == 1, f"the canary counter saw {st['guard_selftest']} changed bytes where exactly one was changed (-1: zones off)"
    assert st["guard_violations"] == 0, "the self-test's allocation is gone, and so is its canary"
    want = [s for s in mb.SCENARIOS if s.group == group]
    assert list(by_name) == [s.name for s in want]
    problems = []
    for s in want:
        d = by_name[s.name]
        if d["error"]:
            problems.append(f"{s.name}: {d['error']}")
        if d["guard_violations"] < 0:
            problems.append(f"{s.name}: guard zones were not on")
        if d["guard_violations"] > 0:
            problems.append(f"{s.name}: {d['guard_violations']} canary bytes changed")
        idle = [c for c in s.prof if d["launches"].get(c, 0) < 1]
        if idle:
            problems.append(f"{s.name}: claimed profile classes never launched: {idle} (launched: {d['launches']})")
        for p in s.proofs:
            if d["proofs"].get(p) is not True:
                problems.append(f"{s.name}: proof {p!r} is {d['proofs'].get(p)}")
    assert not problems, "\n".join(problems)


# ---- C ------------------------------------------------------------------------------------------------------------------------------
def _check_high(d):
    assert d["guard_selftest"] == 1
    bad = [k for k, ok in d["proofs"].items() if ok is not True]
    assert not bad, f"{d['name']}: {bad} (probes {d.get('probes')}, aliases {d.get('aliases')})"
    assert d["guard_violations"] == 0, d


@pytest.mark.parametrize("row", mb.HIGH_SLOTS, ids=[r.name for r in mb.HIGH_SLOTS])
def test_high_slots(row):
    (d,) = _child(row.name)
    assert set(d["proofs"]) == {"aliases_fresh_before", "rows_bit_identical_to_slot_0", "records_bit_identical_to_slot_0",
                                "get_state_identical_to_slot_0", "window_rotated", "aliases_fresh_after", "cached_import_between_probes",
                                "second_pass_identical", "full_aliases_keep_their_bits"}
    assert d["device_bytes"] > row.max_streams * 2 * row.T * 1024 * 4           # both rings were really allocated
    _check_high(d)


def test_high_slots_trunk_group():
    (d,) = _child(mb.HIGH_TRUNK[0])
    assert set(d["proofs"]) == {"vap_and_nod_rows_bit_equal", "nod_frames_every_second_tick"}
    _check_high(d)


# ---- B ------------------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 3, 37)
S37 = 37


def _engine(**kw):
    from vap_realtime_amd import engine
    fr = kw.pop("fr", 20)
    T = kw.pop("T", mb.T8)
    mode = kw.pop("mode", "vap")
    return engine.Engine(mb.blob(fr, mode), fr, mb.ctx_sec(T, fr), mode=mode, **kw)


def _ids(n):
    """n distinct stream ids of a 37-slot engine, reordered, the last slot first."""
    return np.array(([S37 - 1, 0, 17] + list(range(1, 17)) + list(range(18, S37 - 1)))[:n] if n < S37 else list(range(S37))[::-1], dtype=np.int32)


def _warm(eng, ticks=2, seed=1):
    rng = np.random.default_rng(seed)
    for _ in range(ticks):
        eng.step(mb.noise(rng, (eng.max_streams, 2, eng.hop_in)))


def case_step_device(b, n):
    e = _engine(max_streams=S37)
    _warm(e)
    x = b.inp(mb.noise(np.random.default_rng(n), (n, 2, e.hop)), "audio")
    ids = b.inp(_ids(n), "ids", ids_top=S37 - 1)
    out = b.out("out", (n, 784), defined=False)
    e.step_device(n, x.data_ptr(), e.hop, out.data_ptr(), ids_ptr=ids.data_ptr())
    return [e]


def case_step_follow_device(b, n):
    from vap_realtime_amd import engine
    blobs = {m: mb.blob(20, m, seed=40 + i, cpc_hz=20) for i, m in enumerate(("vap", "bc", "nod"))}
    g = engine.TrunkGroup(blobs, 20, {"vap": mb.ctx_sec(8, 20), "bc": mb.ctx_sec(11, 20), "nod": mb.ctx_sec(6, 20)}, max_streams=S37)
    x = b.inp(mb.noise(np.random.default_rng(n), (n, 2, g.hop)), "audio")
    ids = b.inp(_ids(n), "ids", ids_top=S37 - 1)
    outs = {m: b.out(f"out_{m}", (n, 784), defined=False) for m in g.order}
    g.step_device(n, x.data_ptr(), g.hop, {m: t.data_ptr() for m, t in outs.items()}, ids_ptr=ids.data_ptr())
    return [g]


def case_step_group_device(b, n):
    from vap_realtime_amd import engine
    blobs = {"vap": mb.blob(20, "vap", 50, cpc_hz=20), "nod": mb.blob(10, "nod", 51, cpc_hz=20)}
    g = engine.TrunkGroup(blobs, {"vap": 20, "nod": 10}, {"vap": mb.ctx_sec(6, 20), "nod": mb.ctx_sec(5, 10)}, max_streams=S37)
    ids = _ids(n)
    rng = np.random.default_rng(n)
    g.step(mb.noise(rng, (n, 2, g.hop)), ids)                                    # the next tick is one with nod frames
    x = b.inp(mb.noise(rng, (n, 2, g.hop)), "audio")
    wire = b.out("wire", (n * g.leader.group_wire_floats(),), defined=False)
    rc = g.leader.lib.vapx_step_group(g.leader._h, n, ids.ctypes.data_as(C.c_void_p), x.data_ptr(), g.hop, wire.data_ptr(),
                                      engine.AUDIO_DEVICE | engine.OUT_DEVICE, None)
    g.leader._check(rc, "vapx_step_group")
    return [g]


def case_step_packed_device(b, n):
    e = _engine(max_streams=S37, input_classes=mb.TABLE)
    for s in range(S37):
        if s % 3 == 2:
            e.set_stream_channel_classes(s, s % 4, (s + 1) % 4)
        else:
            e.set_stream_class(s, s % 4)
    ids = _ids(n)
    rng = np.random.default_rng(n)
    block = b.inp(np.array(e.pack_input(ids, mb._class_arrays(rng, e, ids, 20))), "packed block")
    out = b.out("out", (n, 784), defined=False)
    e.step_packed_device(ids, block.data_ptr(), out.data_ptr())
    return [e]


def _case_export(cache):
    def case(b, n):
        e = _engine(max_streams=S37, input_hz=32000)                             # the record with the padded history
        _warm(e, 3)
        ids = b.inp(_ids(n), "ids", ids_top=S37 - 1)
        rec = b.out("records", (n, e.state_floats(cache)))
        e.export_streams_device(n, rec.data_ptr(), ids_ptr=ids.data_ptr(), cache=cache)
        return [e]
    return case


def case_import_device(b, n):
    """Reads: the records and the ids of import_streams_device inside margins; what arrives is exported again."""
    src = _engine(max_streams=S37)
    _warm(src, 3)
    e = _engine(max_streams=S37)
    ids_np = _ids(n)
    rec = b.inp(src.export_streams(ids_np, cache=True), "records")
    ids = b.inp(ids_np, "ids", ids_top=S37 - 1)
    back = b.out("records back", (n, e.state_floats(True)))
    e.import_streams_device(n, rec.data_ptr(), ids_ptr=ids.data_ptr(), cache=True)
    e.export_streams_device(n, back.data_ptr(), ids_ptr=ids.data_ptr(), cache=True)
    return [src, e]


_L3 = {}


def _l3(mode="vap", **kw):
    key = (mode, tuple(sorted(kw.items())))
    if key not in _L3:
        _L3[key] = mb._level3_engine(None, mode=mode, **kw)
    return _L3[key]


def _case_transformer(maps, split=False):
    def case(b, rows):
        mb.call_transformer(_l3(split_f16=split), b, 3, rows, maps, stage=0)
        if rows in (33, 250):                                                    # the stages' own output sets
            for stage in (1, 2):
                mb.call_transformer(_l3(split_f16=split), b, 3, rows, maps, stage=stage)
        return []
    return case


def case_encode_audio(b, n):
    e = _engine(max_streams=S37)
    mb.call_encode_audio(e, b, n, _ids(n))
    return [e]


def _case_head(mode, which):
    def case(b, rows):
        mb.call_head(_l3(mode, T=8, hz=20), b, which, rows)
        return []
    return case


def case_pcm_decode(b, rows):
    from vap_realtime_amd import engine, pcm
    lib = engine.load_library()
    for fmt in ("s16", "mulaw", "alaw"):
        n = rows * 16 + (4 if fmt == "s16" else 8)                               # whole words, no multiple of the 256-thread block's span
        raw = b.inp(pcm.encode(fmt, mb.noise(np.random.default_rng(rows), (n,), 0.9)), f"{fmt} samples")
        dst = b.out(f"decoded {fmt}", (n,))
        assert lib.vapx_pcm_decode(pcm.FORMATS[fmt], n, raw.data_ptr(), dst.data_ptr(), None) == 0
    return []


GEMM_SHAPES = ((0, 768, 256, 333), (1, 768, 256, 257), (2, 256, 768, 100), (3, 256, 256, 515), (4, 256, 1024, 31), (5, 256, 1280, 70))


def case_gemm(b, shape):
    from vap_realtime_amd import engine
    epi, N, K, M = shape
    lib = engine.load_library()
    rng = np.random.default_rng(epi * 7 + M)
    A, W = b.inp(mb.noise(rng, (M, K), 1.0), "A"), b.inp(mb.noise(rng, (N, K), K ** -0.5), "W")
    bias, gamma, beta = (b.inp(mb.noise(rng, (N,), 0.3) + add, name) for add, name in ((0, "bias"), (1, "gamma"), (0, "beta")))
    resid = b.inp(mb.noise(rng, (M, N), 1.0), "resid")
    Cm = b.out("C", (M, N))
    C2 = b.out("C2" if epi == 3 else "C2 (unused)", (M, N), defined=epi == 3)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.vapx_gemm(None, M, N, K, p(A), p(W), p(Cm), epi, p(bias) if epi in (0, 4, 5) else None, p(gamma), p(beta), p(resid), p(C2), 0)
    assert rc == 0, lib.vapx_last_error(None)
    return []


CALLER_CASES = (
    [(f"step_device-n{n}", case_step_device, n) for n in BATCHES]
    + [(f"step_follow_device-n{n}", case_step_follow_device, n) for n in BATCHES]
    + [(f"step_group_device-n{n}", case_step_group_device, n) for n in BATCHES]
    + [(f"step_packed_device-n{n}", case_step_packed_device, n) for n in BATCHES]
    + [(f"export_streams_device{'_cache' if c else ''}-n{n}", _case_export(c), n) for c in (False, True) for n in BATCHES]
    + [(f"import_streams_device-n{n}", case_import_device, n) for n in BATCHES]
    + [(f"transformer_maps_device-rows{r}", _case_transformer(True), r) for r in mb.LEVEL3_ROWS]
    + [(f"transformer_device-rows{r}", _case_transformer(False), r) for r in mb.LEVEL3_ROWS]
    + [("transformer_maps_device_split-rows65", _case_transformer(True, True), 65), ("transformer_device_split-rows250", _case_transformer(False, True), 250)]
    + [(f"encode_audio_device-n{n}", case_encode_audio, n) for n in BATCHES]
    + [(f"{which}_{mode}-rows{r}", _case_head(mode, which), r) for mode, which in (("vap", "vap_head"), ("vap", "va_classifier"), ("bc", "bc_head"),
                                                                                   ("nod", "bc_head"), ("nod", "nod_head"), ("vap", "softmax256"),
                                                                                   ("vap", "aggregate")) for r in mb.HEAD_ROWS]
    + [(f"pcm_decode-rows{r}", case_pcm_decode, r) for r in (1, 3, 37, 250)]
    + [(f"gemm-epi{s[0]}", case_gemm, s) for s in GEMM_SHAPES])


@pytest.mark.parametrize("case,arg", [(c, a) for _, c, a in CALLER_CASES], ids=[name for name, _, _ in CALLER_CASES])
def test_caller_buffers(case, arg):
    if ABNORMAL["by"]:
        pytest.fail(f"not started: the child {ABNORMAL['by']!r} of this module ended abnormally before")
    results = []
    for in_fill in (None, 0):                                                   # input margins: NaNs, then zeros / the top stream id
        b = mb.Margins(in_fill)
        held = case(b, arg)
        results.append(b.results())                                             # synchronises; margins and promised rows are checked here
        for e in held:
            e.close()
    first, second = results
    assert list(first) == list(second) and first
    for what in first:
        same = first[what].view(np.uint32) == second[what].view(np.uint32)
        assert same.all(), (f"{what}: {int((~same).sum())} words differ between input margins of NaNs and of zeros: the call read outside "
                            f"its inputs (first at flat index {int(np.argmax(~same.reshape(-1)))})")
        written = first[what].view(np.uint32) != np.uint32(mb.PATTERN)
        if what.endswith("(unused)"):
            assert not written.any(), f"{what}: {int(written.sum())} words written to an output this call does not have"
        else:
            assert written.any(), f"{what}: the call wrote nothing"


def teardown_module(module):
    for e in _L3.values():
        e.close()
    _L3.clear()
