"""Bulk stream-state export / import (vapx_export_streams / vapx_import_streams, include/vapx.h) on the GPU: the gather against the
per-stream vapx_get_state, the round trip as pure data movement, the continuation of migrated streams against their uninterrupted
twins, launch counts, stream ordering, trunk groups, refusals and the snapshot file.

No reference and no golden: expected values come from an uninterrupted twin engine or from get_state.  The population is the smallest
that takes every branch of the gather: seven streams in shuffled, non-contiguous slots of an 11-slot engine whose max_batch = 3 (so the
cache rebuild of an import runs in three chunks), with window fills 0, 3, T-1, T (just full), T+7 and 2T+1 (ring rotated) and one stream
reset part-way.  T = 50 is the short-window dispatch class, T = 70 the long-window one (T > 64)."""
import os

import numpy as np
import pytest

from golden_util import Case

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the bar tests/test_engine_gpu.py::test_state_roundtrip_and_reset sets for a migrated stream
SLOTS = [9, 2, 6, 0, 10, 4, 7]           # source slots of the seven streams (max_streams = 11)
SLOTS_B = [3, 15, 0, 8, 12, 1, 6]        # their slots in the target engine (max_streams = 16)
CTX = {1: 0.05, 50: 2.5, 70: 3.5}
_CACHE = {}


def _case(name="vap20"):
    if name not in _CACHE:
        from vap_realtime_amd import weights as W
        c = Case(name)
        _CACHE[name] = (c, W.pack_blob(c.cpc_sd, c.vap_sd, c.mode))
    return _CACHE[name]


def _audio(T):
    """[7, 2, hop * (2T + 12)] seeded dialogue audio, stream k of the population on row k."""
    key = ("audio", T)
    if key not in _CACHE:
        from vap_realtime_amd import synth
        _CACHE[key] = synth.dialogue_batch(list(range(40, 47)), 800 * (2 * T + 12))
    return _CACHE[key]


def _engine(T, max_streams=11, max_batch=3, **kw):
    from vap_realtime_amd import engine
    c, blob = _case()
    return engine.Engine(blob, c.frame_hz, CTX[T], max_streams=max_streams, max_batch=max_batch, mode=c.mode, **kw)


def _fills(T):
    F = 2 * T + 1
    return F, [0, 3, T - 1, T, T + 7, 2 * T + 1, F - (T + 5)]      # the last stream is reset before tick T + 5


def _tick(eng, T, f, members, slots):
    """One tick for the population's members (indices into the seven), in sub-batches of three; returns {member: output row}."""
    a = _audio(T)
    rows = {}
    for i in range(0, len(members), 3):
        part = members[i:i + 3]
        out = eng.step(a[part, :, f * 800:(f + 1) * 800], [slots[k] for k in part])
        for k, row in zip(part, out):
            rows[k] = row.copy()
    return rows


def _populate(T, **kw):
    eng = _engine(T, **kw)
    F, fills = _fills(T)
    for f in range(F):
        if f == T + 5:
            eng.reset_stream(SLOTS[6])
        members = [k for k in range(7) if k == 6 or f >= F - fills[k]]
        _tick(eng, T, f, members, SLOTS)
    return eng, F, fills


@pytest.mark.parametrize("T", [50, 70])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_export_agrees_with_get_state(split, T):
    from vap_realtime_amd import engine
    eng, F, fills = _populate(T, split_f16=split)
    assert eng.state_floats() == 8 + 1024 + 640 + 2 * T * 256 and eng.state_floats(True) == eng.state_floats() + 2 * T * 768
    for cache in (False, True):
        rec = eng.export_streams(SLOTS, cache=cache)
        assert rec.shape == (7, eng.state_floats(cache))
        s = engine.split_state(rec, T)
        assert s["magic"].tolist() == [engine.STATE_MAGIC] * 7 and s["ctx_frames"].tolist() == [T] * 7 and s["frame_hz"].tolist() == [20] * 7
        bits = engine.STATE_HAS_LSTM | ((engine.STATE_HAS_CACHE | (engine.STATE_CACHE_SPLIT if split else 0)) if cache else 0)
        assert s["bits"].tolist() == [bits] * 7 and s["mode"].tolist() == [0] * 7
        assert not rec[:, 6:8].view(np.int32).any()
        assert s["n_frames"].tolist() == [min(x, T) for x in fills]
        for k, sid in enumerate(SLOTS):
            st = eng.get_state(sid)
            n = st["n_frames"]
            assert n == s["n_frames"][k]
            np.testing.assert_array_equal(s["ring"][k][:, :n], st["ring"][:, :n], err_msg=f"stream {k} ring")
            assert not s["ring"][k][:, n:].any(), f"stream {k}: rows beyond n_frames are not zero"
            np.testing.assert_array_equal(s["lstm"][k], st["lstm"])
            np.testing.assert_array_equal(s["carry"][k], st["carry"])
            if cache:
                assert not s["cache"][k][:, n:].any()
                assert n == 0 or s["cache"][k][:, :n].any()
    # a pinned destination (DMA target itself) and a pageable one hold the same bytes
    pinned = engine.pinned_empty((7, eng.state_floats(True)))
    np.testing.assert_array_equal(eng.export_streams(SLOTS, cache=True, out=pinned), rec)
    eng.close()


@pytest.mark.parametrize("T", [50, 70])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_round_trip_is_data_movement_and_the_continuation_matches(split, T):
    """Export with cache -> import into other slots of a larger engine -> export again: bit-equal, cache rows included.  Then both
    engines run 5 more ticks (the full windows slide): a stream that carried its cache continues BIT-identically — the same kernels
    consume the same values in the same launch shapes — which is stronger than the 1e-5 bar and what vapx.h promises."""
    from vap_realtime_amd.engine import split_outputs
    a, F, _ = _populate(T, split_f16=split)
    b = _engine(T, max_streams=16, split_f16=split)
    rec = a.export_streams(SLOTS, cache=True)
    b.import_streams(SLOTS_B, rec)
    np.testing.assert_array_equal(b.export_streams(SLOTS_B, cache=True), rec)
    worst = 0.0
    for f in range(F, F + 5):
        ra, rb = _tick(a, T, f, list(range(7)), SLOTS), _tick(b, T, f, list(range(7)), SLOTS_B)
        for k in range(7):
            oa, ob = split_outputs(ra[k][None]), split_outputs(rb[k][None])
            for key in ("p_now", "p_future", "vad", "logits", "e"):
                worst = max(worst, float(np.abs(oa[key] - ob[key]).max()))
                np.testing.assert_allclose(ob[key], oa[key], rtol=0, atol=TOL, err_msg=f"tick {f} stream {k} {key}")
            np.testing.assert_array_equal(rb[k], ra[k], err_msg=f"tick {f} stream {k}: not bit-identical")
    print(f"continuation with cache, T={T} split={split}: worst |diff| = {worst:.3e}")
    np.testing.assert_array_equal(b.export_streams(SLOTS_B, cache=True), a.export_streams(SLOTS, cache=True))
    a.close(); b.close()


def test_host_records_in_several_staging_blocks(monkeypatch):
    """Host records travel through a bounded device block (pageable memory additionally through a pinned one).  With the block shrunk to
    two or three records the seven streams take the multi-block path in every direction: the bytes must equal the single-kernel device
    export."""
    import torch
    from vap_realtime_amd import engine
    T = 50
    a, _, _ = _populate(T)
    b = _engine(T, max_streams=16)
    d_ids = torch.tensor(SLOTS, dtype=torch.int32, device="cuda")
    for cache in (True, False):
        fl = a.state_floats(cache)
        d_rec = torch.zeros(7, fl, device="cuda")
        a.export_streams_device(7, d_rec.data_ptr(), ids_ptr=d_ids.data_ptr(), cache=cache)
        torch.cuda.synchronize()
        want = d_rec.cpu().numpy()
        monkeypatch.setenv("VAPX_STATE_STAGE_FLOATS", str(fl * (3 if cache else 2)))
        np.testing.assert_array_equal(a.export_streams(SLOTS, cache=cache), want)                       # pageable, 3 / 4 blocks
        pinned = engine.pinned_empty((7, fl))
        np.testing.assert_array_equal(a.export_streams(SLOTS, cache=cache, out=pinned), want)           # page-locked
        b.import_streams(SLOTS_B, want)                                                                 # pageable source
        np.testing.assert_array_equal(b.export_streams(SLOTS_B, cache=cache), want)
        for sid in SLOTS_B:
            b.reset_stream(sid)
        assert not engine.split_state(b.export_streams(SLOTS_B), T)["n_frames"].any()
        b.import_streams(SLOTS_B, pinned)                                                               # page-locked source
        monkeypatch.delenv("VAPX_STATE_STAGE_FLOATS")
        np.testing.assert_array_equal(b.export_streams(SLOTS_B, cache=cache), want)                     # one block
    a.close(); b.close()


def test_cache_import_launches_nothing_and_the_rebuild_is_batched():
    T = 50
    a, _, _ = _populate(T)
    b = _engine(T)
    rec_c, rec = a.export_streams(SLOTS, cache=True), a.export_streams(SLOTS)
    b.profile_enable((0, 10))
    b.import_streams([1, 5, 8], rec_c[:3])
    assert b.profile_read() == {}, "an import with VAPX_STATE_CACHE must launch no LayerNorm gather and no GEMM"
    b.import_streams([1, 5], rec[:2])
    two = {k: v[1] for k, v in b.profile_read().items()}
    b.import_streams([1, 5, 8], rec[:3])
    three = {k: v[1] for k, v in b.profile_read().items()}
    assert two == three == {"gemm_store": 1, "gather_ln": 1}          # one chunk: the count does not grow with the streams in it
    b.import_streams(SLOTS, rec)                                     # seven streams, max_batch = 3: three chunks
    assert {k: v[1] for k, v in b.profile_read().items()} == {"gemm_store": 3, "gather_ln": 3}
    b.profile_enable(())
    a.close(); b.close()


@pytest.mark.parametrize("T", [50, 70])
def test_import_without_cache_equals_the_per_stream_path(T):
    from vap_realtime_amd.engine import split_outputs
    a, F, _ = _populate(T)
    x, y = _engine(T), _engine(T)
    x.import_streams(SLOTS, a.export_streams(SLOTS))
    for sid in SLOTS:
        y.set_state(sid, a.get_state(sid))
    for sid in SLOTS:
        sx, sy = x.get_state(sid), y.get_state(sid)
        n = sx["n_frames"]
        assert n == sy["n_frames"] == a.get_state(sid)["n_frames"]
        np.testing.assert_array_equal(sx["ring"][:, :n], sy["ring"][:, :n])
        np.testing.assert_array_equal(sx["lstm"], sy["lstm"])
        np.testing.assert_array_equal(sx["carry"], sy["carry"])
    for f in range(F, F + 3):
        rx, ry = _tick(x, T, f, list(range(7)), SLOTS), _tick(y, T, f, list(range(7)), SLOTS)
        for k in range(7):
            ox, oy = split_outputs(rx[k][None]), split_outputs(ry[k][None])
            for key in ("p_now", "p_future", "vad", "logits", "e"):
                np.testing.assert_allclose(ox[key], oy[key], rtol=0, atol=TOL, err_msg=f"tick {f} stream {k} {key}")
    a.close(); x.close(); y.close()


@pytest.mark.parametrize("T", [50, 70])
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_set_state_is_the_one_record_import(split, T):
    """vapx_set_state moves a stream through the kernels of the bulk import and rebuilds its cache with the import's helper: one record
    per vapx_import_streams call has the GEMM shape (M = 2T) of a vapx_set_state, so the two engines end up BIT-equal - ring, LSTM, carry,
    n_frames and every cache row of the export - and stay so for three more ticks."""
    a, F, _ = _populate(T, split_f16=split)
    x, y = _engine(T, split_f16=split), _engine(T, split_f16=split)
    rec = a.export_streams(SLOTS)
    for k, sid in enumerate(SLOTS):
        x.import_streams([sid], rec[k:k + 1])
        y.set_state(sid, a.get_state(sid))
    np.testing.assert_array_equal(y.export_streams(SLOTS, cache=True), x.export_streams(SLOTS, cache=True))
    for f in range(F, F + 3):
        rx, ry = _tick(x, T, f, list(range(7)), SLOTS), _tick(y, T, f, list(range(7)), SLOTS)
        for k in range(7):
            np.testing.assert_array_equal(ry[k], rx[k], err_msg=f"tick {f} stream {k}: not bit-identical")
    a.close(); x.close(); y.close()


@pytest.mark.parametrize("T", [1, 50])
def test_partial_set_state_touches_only_what_it_names(T):
    """vapx_set_state with the ring alone, the LSTM alone, the carry alone and the ring with n_frames = 0, on every stream of the
    population in turn: after each call the export (with cache) of ALL seven streams is held against the export before it - what the call
    did not name is bit-equal, n_frames and cache rows included, what it named is what was given."""
    from vap_realtime_amd import engine
    eng, _, fills = _populate(T)
    rng = np.random.default_rng(T)
    want = eng.export_streams(SLOTS, cache=True).copy()
    w = engine.split_state(want, T)                                   # views into `want`

    def held(what):
        np.testing.assert_array_equal(eng.export_streams(SLOTS, cache=True), want, err_msg=what)

    for k, sid in enumerate(SLOTS):
        lstm = rng.standard_normal((2, 2, 256)).astype(np.float32)
        eng.set_state(sid, {"lstm": lstm, "n_frames": T})             # n_frames without a ring says nothing
        w["lstm"][k] = lstm
        held(f"stream {k}: lstm alone")
        carry = rng.standard_normal((2, 320)).astype(np.float32)
        eng.set_state(sid, {"carry": carry})
        w["carry"][k] = carry
        held(f"stream {k}: carry alone")
        n = [T, max(T - 3, 1), 1][k % 3]
        ring = rng.standard_normal((2, T, 256)).astype(np.float32)
        eng.set_state(sid, {"ring": ring, "n_frames": n})
        got = engine.split_state(eng.export_streams(SLOTS, cache=True), T)
        assert got["n_frames"][k] == n
        np.testing.assert_array_equal(got["ring"][k][:, :n], ring[:, :n])
        assert not got["ring"][k][:, n:].any() and not got["cache"][k][:, n:].any()
        assert np.isfinite(got["cache"][k]).all() and all(got["cache"][k][c, t].any() for c in range(2) for t in range(n))
        w["n_frames"][k], w["ring"][k], w["cache"][k] = n, got["ring"][k], got["cache"][k]      # the named sections move on ...
        held(f"stream {k}: ring alone")                                                         # ... and nothing else has
        eng.set_state(sid, {"ring": ring, "n_frames": 0})
        w["n_frames"][k], w["ring"][k], w["cache"][k] = 0, 0, 0
        held(f"stream {k}: ring with n_frames = 0")
    eng.close()


def test_refused_follower_read_writes_nothing():
    """vapx_get_state on a same-rate follower with a non-NULL lstm is refused before anything is written: the caller's ring and n_frames
    keep the pattern they held (argument checks before anything)."""
    import ctypes as C
    c, g = _trunk_group()
    for f in range(3):
        g.step_wire(c.new_samples(f), [3, 1])
    fol = g.engines["nod"]
    assert fol.get_state(3)["n_frames"] == 3
    ring = np.full((2, c.T, 256), np.nan, np.float32)
    ring.view(np.uint32)[:] = 0x7FC0BEEF
    lstm, n = np.zeros((2, 2, 256), np.float32), C.c_int32(-77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((ptr(lstm), None), (None, ptr(np.zeros((2, 320), np.float32))), (ptr(lstm), ptr(np.zeros((2, 320), np.float32)))):
        rc = fol.lib.vapx_get_state(fol._h, 3, ptr(ring), C.byref(n), *args)
        assert rc == -1 and "lives in the trunk leader" in fol.lib.vapx_last_error(fol._h).decode()
        assert n.value == -77 and (ring.view(np.uint32) == 0x7FC0BEEF).all() and not lstm.any()
    assert fol.lib.vapx_get_state(fol._h, 3, ptr(ring), C.byref(n), None, None) == 0 and n.value == 3
    assert np.isfinite(ring[:, :3]).all() and (ring.view(np.uint32)[:, 3:] == 0x7FC0BEEF).all()      # rows beyond n_frames stay the caller's
    g.close()


def test_records_without_cache_move_between_the_precision_paths():
    """fp32 engine -> split engine without cache is accepted and continues within the project's parity bar of the split path (1e-4,
    tests/test_split_precision_gpu.py); the same records WITH cache are refused (covered in test_refusals_leave_the_engine_untouched)."""
    from vap_realtime_amd.engine import split_outputs
    T = 50
    a, F, _ = _populate(T)
    b = _engine(T, split_f16=True)
    b.import_streams(SLOTS, a.export_streams(SLOTS))
    ra, rb = _tick(a, T, F, list(range(7)), SLOTS), _tick(b, T, F, list(range(7)), SLOTS)
    for k in range(7):
        for key in ("p_now", "p_future", "vad", "logits"):
            np.testing.assert_allclose(split_outputs(rb[k][None])[key], split_outputs(ra[k][None])[key], rtol=0, atol=1e-4)
    a.close(); b.close()


def test_export_is_ordered_on_the_stream_like_a_step():
    """Two overlap groups stepped device-resident with VAPX_DEFER_JOIN and no synchronisation, then an export to a device buffer on the
    same stream, ONE synchronisation: the records show that step's state.  A reset queued before an export shows up in it."""
    import torch
    from vap_realtime_amd import engine, synth
    c, blob = _case()
    S, F_, T = 64, 3, 50
    eng = engine.Engine(blob, 20, 2.5, max_streams=S, groups=2)
    audio = synth.noise_batch(S, 800 * F_, seed=11)
    d_audio = [torch.from_numpy(np.ascontiguousarray(audio[:, :, f * 800:(f + 1) * 800])).cuda() for f in range(F_)]
    d_out = torch.zeros(S, engine.OUT_STRIDE, device="cuda")
    fl = eng.state_floats()
    d_rec, d_rec2 = torch.zeros(S, fl, device="cuda"), torch.zeros(S, fl, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for f in range(F_):
        eng.step_device(S, d_audio[f].data_ptr(), 800, d_out.data_ptr(), stream=side.cuda_stream, defer_join=True)
    eng.export_streams_device(S, d_rec.data_ptr(), stream=side.cuda_stream)
    eng.reset_stream(5)
    eng.export_streams_device(S, d_rec2.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    s = engine.split_state(d_rec.cpu().numpy(), T)
    assert s["n_frames"].tolist() == [F_] * S
    np.testing.assert_array_equal(s["carry"], audio[:, :, -320:])
    assert all(s["lstm"][k].any() and s["ring"][k][:, :F_].any() for k in range(S))
    s2 = engine.split_state(d_rec2.cpu().numpy(), T)
    assert s2["n_frames"].tolist() == [0 if k == 5 else F_ for k in range(S)]
    assert not s2["lstm"][5].any() and not s2["carry"][5].any() and not s2["ring"][5].any()
    keep = [k for k in range(S) if k != 5]
    np.testing.assert_array_equal(d_rec2.cpu().numpy()[keep], d_rec.cpu().numpy()[keep])
    # device ids + device records back into another engine, still without a host synchronisation in between
    other = engine.Engine(blob, 20, 2.5, max_streams=S)
    d_ids = torch.arange(S - 1, -1, -1, dtype=torch.int32, device="cuda")
    d_back = torch.zeros(S, fl, device="cuda")
    with torch.cuda.stream(side):
        other.import_streams_device(S, d_rec.data_ptr(), ids_ptr=d_ids.data_ptr(), stream=side.cuda_stream)
        other.export_streams_device(S, d_back.data_ptr(), ids_ptr=d_ids.data_ptr(), stream=side.cuda_stream)
    side.synchronize()
    np.testing.assert_array_equal(d_back.cpu().numpy(), d_rec.cpu().numpy())
    eng.close(); other.close()


def _trunk_group(max_streams=4):
    from vap_realtime_amd import engine, weights as W
    for m in ("bc", "nod"):
        if ("trunk", m) not in _CACHE:
            c = Case(f"trunk_{m}20")
            _CACHE[("trunk", m)] = (c, W.pack_blob(c.cpc_sd, c.vap_sd, m))
    c = _CACHE[("trunk", "bc")][0]
    blobs = {m: _CACHE[("trunk", m)][1] for m in ("bc", "nod")}
    return c, engine.TrunkGroup(blobs, c.frame_hz, c.ctx_sec, max_streams=max_streams)


def test_trunk_group_moves_as_a_whole():
    from vap_realtime_amd import engine
    c, a = _trunk_group()
    _, b = _trunk_group()
    T, ids, ids_b = c.T, [3, 1], [0, 2]
    assert T == 50
    for f in range(c.n_frames):                       # 54 frames: the window is full and has slid four times
        a.step_wire(c.new_samples(f), ids)
    rec = a.export_streams(ids, cache=True)
    assert list(rec) == ["bc", "nod"]
    lead, fol = engine.split_state(rec["bc"], T), engine.split_state(rec["nod"], T, follower=True)
    assert rec["nod"].shape[1] == a.engines["nod"].state_floats(True) == rec["bc"].shape[1] - 1664
    assert fol["lstm"] is None and fol["carry"] is None and not (fol["bits"] & engine.STATE_HAS_LSTM).any()
    assert (lead["bits"] & engine.STATE_HAS_LSTM).all() and lead["mode"].tolist() == [1, 1] and fol["mode"].tolist() == [2, 2]
    assert lead["n_frames"].tolist() == fol["n_frames"].tolist() == [T, T]
    # a leader record offered to a follower is refused, and the reverse; nothing changes
    before = b.export_streams(None, cache=True)
    nocache = a.export_streams(ids)
    with pytest.raises(engine.VapxError, match="record length"):
        b.engines["nod"].import_streams(ids_b, nocache["bc"])
    lib = b.leader.lib
    i32 = np.asarray(ids_b, np.int32)
    for eng_, blk, word in ((b.engines["nod"], nocache["bc"], "follower"), (b.leader, nocache["nod"], "follower's record")):
        pad = np.zeros((2, max(nocache["bc"].shape[1], nocache["nod"].shape[1])), np.float32)      # room for the longer stride
        pad[:, :blk.shape[1]] = blk
        rc = lib.vapx_import_streams(eng_._h, 2, i32.ctypes.data, pad.ctypes.data, 0, None)
        assert rc == -1 and "content bits" in lib.vapx_last_error(eng_._h).decode() and word in lib.vapx_last_error(eng_._h).decode()
    after = b.export_streams(None, cache=True)
    for m in before:
        np.testing.assert_array_equal(after[m], before[m])
    b.import_streams(ids_b, rec)
    extra = np.ascontiguousarray(c.audio[:, :, :800 * 4])
    for f in range(4):
        x = extra[:, :, f * 800:(f + 1) * 800]
        wa, wb = a.step_wire(x, ids), b.step_wire(x, ids_b)
        for m in wa:
            np.testing.assert_allclose(wb[m], wa[m], rtol=0, atol=TOL, err_msg=f"{m} tick {f}")
    # and the plain leader / follower steps go on as well
    x = extra[:, :, :800]
    sa, sb = a.step(x, ids), b.step(x, ids_b)
    for m in sa:
        np.testing.assert_allclose(sb[m][:, :272], sa[m][:, :272], rtol=0, atol=TOL)
    a.close(); b.close()


def test_refusals_leave_the_engine_untouched():
    from vap_realtime_amd import engine
    T = 50
    a, F, _ = _populate(T)
    sp = _engine(T, split_f16=True)
    rec, rec_c = a.export_streams(SLOTS), a.export_streams(SLOTS, cache=True)
    before = a.export_streams(None, cache=True)

    def bad(word, value):
        r = rec.copy()
        r[4, :8].view(np.int32)[word] = value          # record 4 of 7
        return r

    cases = [
        ("ctx_frames", -1, r"record 4: ctx_frames 51", lambda: a.import_streams(SLOTS, bad(1, 51))),
        ("frame_hz", -1, r"record 4: frame_hz 10", lambda: a.import_streams(SLOTS, bad(2, 10))),
        ("magic", -1, r"record 4: magic", lambda: a.import_streams(SLOTS, bad(0, 0x12345678))),
        ("n_frames", -4, rf"record 4: n_frames {T + 1} outside", lambda: a.import_streams(SLOTS, bad(4, T + 1))),
        ("duplicate id", -1, r"stream id 6 appears twice", lambda: a.import_streams([9, 2, 6, 0, 10, 6, 7], rec)),
        ("id out of range", -4, r"stream id 11 out of range", lambda: a.import_streams([9, 2, 6, 0, 11, 4, 7], rec)),
        ("n > max_streams", -4, r"n=12 outside \[1,11\]", lambda: a.import_streams(list(range(12)), np.concatenate([rec, rec[:5]]))),
        ("n > max_streams (export)", -4, r"n=12 outside \[1,11\]", lambda: a.export_streams(list(range(12)))),
    ]
    for name, code, pattern, call in cases:
        with pytest.raises(engine.VapxError, match=pattern) as ei:
            call()
        assert f"({code})" in str(ei.value), (name, str(ei.value))
        np.testing.assert_array_equal(a.export_streams(None, cache=True), before, err_msg=name)
    # a cache made on the fp32 path is refused by a split-precision engine (and the reverse), whose streams stay as they were
    sp_before = sp.export_streams(None, cache=True)
    with pytest.raises(engine.VapxError, match=r"record 0: content bits.*fp32 path.*split-precision path") as ei:
        sp.import_streams(SLOTS, rec_c)
    assert "(-1)" in str(ei.value)
    np.testing.assert_array_equal(sp.export_streams(None, cache=True), sp_before)
    with pytest.raises(engine.VapxError, match=r"content bits.*split-precision path.*fp32 path"):
        a.import_streams(SLOTS, sp.export_streams(SLOTS, cache=True))
    np.testing.assert_array_equal(a.export_streams(None, cache=True), before)
    # both engines still step
    _tick(a, T, F, list(range(7)), SLOTS)
    _tick(sp, T, 0, list(range(7)), SLOTS)
    a.close(); sp.close()


def test_snapshot_file_round_trip_and_refusals(tmp_path):
    import json
    import struct
    from vap_realtime_amd import snapshot
    from vap_realtime_amd.engine import VapxError
    T = 50
    a, F, _ = _populate(T)
    b = _engine(T)
    path = str(tmp_path / "state.vapx")
    hdr = snapshot.save(path, a)
    assert hdr["ids"] == list(range(11)) and hdr["cache"] and hdr["ctx_frames"] == T and hdr["modes"] == ["vap"]
    assert sorted(os.listdir(tmp_path)) == ["state.vapx"]
    empty = b.export_streams(None, cache=True)
    # a truncated file and one whose header names another window are refused before any stream changes
    blob = open(path, "rb").read()
    cut = str(tmp_path / "cut.vapx")
    open(cut, "wb").write(blob[:len(blob) - 4096])
    with pytest.raises(VapxError, match="truncated"):
        snapshot.load(cut, b)
    (jl,) = struct.unpack("<I", blob[8:12])
    h2 = json.loads(blob[12:12 + jl])
    h2["ctx_frames"] = 51
    js = json.dumps(h2, separators=(",", ":")).encode()
    assert len(js) == jl
    other = str(tmp_path / "other.vapx")
    open(other, "wb").write(blob[:12] + js + blob[12 + jl:])
    with pytest.raises(VapxError, match="ctx_frames"):
        snapshot.load(other, b)
    np.testing.assert_array_equal(b.export_streams(None, cache=True), empty)
    assert snapshot.load(path, b) == list(range(11))
    np.testing.assert_array_equal(b.export_streams(None, cache=True), a.export_streams(None, cache=True))
    for f in range(F, F + 5):
        ra, rb = _tick(a, T, f, list(range(7)), SLOTS), _tick(b, T, f, list(range(7)), SLOTS)
        for k in range(7):
            np.testing.assert_array_equal(rb[k], ra[k], err_msg=f"tick {f} stream {k}")
    a.close(); b.close()


def _serve(tmp, *state_args):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.Popen([sys.executable, "-u", "-m", "vap_realtime_amd.serve", "--synthetic-weights", "3", "--streams", "2", "--precision", "fp32",
                             "--port_num_in", "0", "--port_num_out", "0", "--stats_sec", "0", *state_args],
                            cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _dialogue(proc, frames, audio):
    """Connect two dialogues to a serve process, feed ``frames`` of ``audio`` [2,2,*] and return every result, [frame][stream] dicts."""
    import re
    import socket
    import struct
    import time
    from vap_realtime_amd import wire
    seen, line, t0 = [], "", time.time()
    while "input :" not in line and time.time() - t0 < 180:
        line = proc.stdout.readline()
        seen.append(line)
        assert line or proc.poll() is None, "serve exited early: " + "".join(seen)
    pin, pout = (int(x) for x in re.search(r"input :(\d+), output :(\d+)", line).groups())
    ins, outs = [], []
    for lst, port in ((ins, pin), (outs, pout)):
        for _ in range(2):                       # one by one: arrival order = dialogue slot
            lst.append(socket.create_connection(("127.0.0.1", port)))
            time.sleep(0.1)
    res = []
    for f in frames:
        new = audio[:, :, f * 800:(f + 1) * 800].astype(np.float64)
        for s in range(2):
            ins[s].sendall(wire.encode_input(new[s, 0], new[s, 1]))
        row = []
        for s in range(2):
            outs[s].settimeout(30)
            buf = b""
            while len(buf) < 4:
                buf += outs[s].recv(4 - len(buf))
            (ln,) = struct.unpack("<I", buf)
            payload = b""
            while len(payload) < ln:
                payload += outs[s].recv(ln - len(payload))
            row.append(wire.decode_result(payload, "vap"))
        res.append(row)
    for s in ins + outs:
        s.close()
    return "".join(seen), res


def _stop(proc):
    import signal
    import subprocess
    proc.send_signal(signal.SIGTERM)
    try:
        out, _ = proc.communicate(timeout=60)
    except subprocess.TimeoutExpired:
        proc.kill()
        out, _ = proc.communicate()
    return out


def test_serve_restart_keeps_the_dialogues(tmp_path):
    """``serve --save_state`` on SIGTERM, then ``serve --load_state``: the restarted service answers the next frame as an engine that was
    never stopped does (a new connection re-zeroes the carry, vap_main.py:368-369, in both), and not as a cold one.  (The refusal of a
    snapshot that does not fit is covered without a GPU: tests/test_state_file.py.)"""
    from vap_realtime_amd import engine, snapshot, synth, weights as W
    path = str(tmp_path / "state.vapx")
    audio = synth.dialogue_batch([0, 1], 800 * 8).astype(np.float32)
    proc = _serve(tmp_path, "--save_state", path, "--load_state", path)
    try:
        banner, first = _dialogue(proc, range(6), audio)
        assert "cold start" in banner                                  # no file yet: a warning, and the service came up
    finally:
        out = _stop(proc)
    assert proc.returncode == 0 and "state of 2 dialogue slot(s) saved" in out, out
    hdr, _ = snapshot.read_header(path)
    assert hdr["ids"] == [0, 1] and hdr["cache"] and hdr["modes"] == ["vap"] and sorted(os.listdir(tmp_path)) == ["state.vapx"]
    # the twin that never stopped
    cpc, vap = W.synthetic_weights(3, 20, "vap")
    twin = engine.Engine(W.pack_blob(cpc, vap), 20, 2.5, max_streams=2)
    for f in range(6):
        o = engine.split_outputs(twin.step(audio[:, :, f * 800:(f + 1) * 800]))
    np.testing.assert_allclose([r["p_now"] for r in first[5]], o["p_now"], rtol=0, atol=TOL)
    twin.reset_carry(0); twin.reset_carry(1)
    want = engine.split_outputs(twin.step(audio[:, :, 6 * 800:7 * 800]))
    cold = engine.Engine(W.pack_blob(cpc, vap), 20, 2.5, max_streams=2)
    cold_o = engine.split_outputs(cold.step(audio[:, :, 6 * 800:7 * 800]))
    twin.close(); cold.close()
    proc = _serve(tmp_path, "--load_state", path)
    try:
        banner, second = _dialogue(proc, [6], audio)
        assert "state of 2 dialogue slot(s) loaded" in banner
    finally:
        _stop(proc)
    assert proc.returncode == 0
    for k in ("p_now", "p_future", "vad"):
        got = np.array([r[k] for r in second[0]])
        np.testing.assert_allclose(got, want[k], rtol=0, atol=TOL, err_msg=k)
    assert np.abs(np.array([r["p_now"] for r in second[0]]) - cold_o["p_now"]).max() > 100 * TOL      # a cold start answers differently
