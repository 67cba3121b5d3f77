"""Snapshot files and the state-record arithmetic without a GPU: header write / parse / validate on synthetic records, the record sizes
against the layout documented in include/vapx.h, and serve's --load_state / --save_state handling over stub engines."""
import json
import os
import re
import struct

import numpy as np
import pytest

from vap_realtime_amd import engine, serve, snapshot
from vap_realtime_amd.engine import VapxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_records(n, T, cache=False, follower=False, hz=20, split=False, mode=0, seed=0):
    """Synthetic records in the layout of vapx.h: random payload, n_frames = k mod (T + 1), zero rows beyond it."""
    fl = engine.state_record_floats(T, cache, follower)
    rng = np.random.default_rng(seed)
    rec = rng.standard_normal((n, fl)).astype(np.float32)
    hdr = rec[:, :8].view(np.int32)
    bits = (0 if follower else engine.STATE_HAS_LSTM) | ((engine.STATE_HAS_CACHE | (engine.STATE_CACHE_SPLIT if split else 0)) if cache else 0)
    for k in range(n):
        hdr[k] = [engine.STATE_MAGIC, T, hz, bits, k % (T + 1), mode, 0, 0]
    s = engine.split_state(rec, T, follower)
    for k in range(n):
        s["ring"][k][:, k % (T + 1):] = 0
        if cache:
            s["cache"][k][:, k % (T + 1):] = 0
    return rec


class StubEngine:
    """What snapshot / serve touch of an Engine."""

    def __init__(self, T=50, hz=20, mode="vap", max_streams=6, split_f16=False, follower=False):
        self.T, self.frame_hz, self.mode, self.max_streams, self.split_f16, self.follower = T, hz, mode, max_streams, split_f16, follower
        self.imported = []

    def export_streams(self, ids=None, cache=False):
        ids = list(range(self.max_streams)) if ids is None else list(ids)
        return make_records(len(ids), self.T, cache, self.follower, self.frame_hz, self.split_f16, engine.MODE[self.mode], seed=len(ids))

    def import_streams(self, ids, records, cache=None):
        self.imported.append((list(ids), np.array(records), cache))


class StubGroup:
    def __init__(self, modes=("bc", "nod"), **kw):
        self.modes = list(modes)
        self.engines = {m: StubEngine(mode=m, follower=i > 0, **kw) for i, m in enumerate(self.modes)}


def test_record_sizes_follow_the_layout_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "vapx.h")).read()
    # the layout as the header states it: 8 header words, lstm [2][2][256] + carry [2][320] = 1664, ring [2][T][256], cache [2][T][768]
    assert "lstm    [2 ch][2 (h, c)][256] and carry [2][320] (1664 floats)" in hdr
    assert "ring    [2][T][256]" in hdr and "[2][T][768]" in hdr and "header  8 x int32 (32 bytes" in hdr
    defs = {k: int(v, 0) for k, v in re.findall(r"#define (VAPX_STATE_[A-Z_]+) (\w+)", hdr)}
    assert defs == {"VAPX_STATE_CACHE": engine.STATE_CACHE, "VAPX_STATE_MAGIC": engine.STATE_MAGIC, "VAPX_STATE_HAS_LSTM": engine.STATE_HAS_LSTM,
                    "VAPX_STATE_HAS_CACHE": engine.STATE_HAS_CACHE, "VAPX_STATE_CACHE_SPLIT": engine.STATE_CACHE_SPLIT,
                    "VAPX_STATE_HEADER_FLOATS": engine.STATE_HEADER_FLOATS}
    assert struct.pack("<I", engine.STATE_MAGIC) == b"VPS1"
    for T in (1, 50, 70, 250, 512):
        lead, fol = engine.state_record_floats(T), engine.state_record_floats(T, follower=True)
        assert lead == 8 + 2 * 2 * 256 + 2 * 320 + 2 * T * 256 and fol == 8 + 2 * T * 256
        assert engine.state_record_floats(T, True) == lead + 2 * T * 768 and engine.state_record_floats(T, True, True) == fol + 2 * T * 768
        assert all(x % 4 == 0 for x in (lead, fol, lead + 2 * T * 768))              # records stay 16-byte aligned
    # the C side computes the same (no device needed: a null handle answers 0, the sizes themselves are asserted on the GPU)
    assert engine.load_library().vapx_state_floats(None, 0) == 0


def test_split_state_names_the_fields():
    T = 7
    for follower in (False, True):
        for cache in (False, True):
            rec = make_records(5, T, cache, follower, split=True, mode=2)
            s = engine.split_state(rec, T, follower)
            assert s["n_frames"].tolist() == [0, 1, 2, 3, 4] and s["mode"].tolist() == [2] * 5 and s["ctx_frames"].tolist() == [T] * 5
            assert (s["lstm"] is None) == follower and (s["carry"] is None) == follower and (s["cache"] is None) == (not cache)
            assert s["ring"].shape == (5, 2, T, 256) and not s["ring"][2][:, 2:].any() and s["ring"][2][:, :2].all()
            if not follower:
                assert s["lstm"].shape == (5, 2, 2, 256) and s["carry"].shape == (5, 2, 320)
                np.testing.assert_array_equal(s["carry"][3].reshape(-1), rec[3, 8 + 1024:8 + 1664])
            if cache:
                np.testing.assert_array_equal(s["cache"][4].reshape(-1), rec[4, -2 * T * 768:])
    with pytest.raises(VapxError, match="fits no layout"):
        engine.split_state(np.zeros((1, 100), np.float32), T)


def test_snapshot_write_parse_validate(tmp_path):
    a = StubEngine()
    path = str(tmp_path / "s.vapx")
    hdr = snapshot.save(path, a, ids=[4, 1, 3])
    assert hdr == {"version": 1, "frame_hz": 20, "ctx_frames": 50, "modes": ["vap"], "split_f16": False, "cache": True, "ids": [4, 1, 3],
                   "record_floats": [engine.state_record_floats(50, True)]}
    assert os.listdir(tmp_path) == ["s.vapx"]                                     # the temporary name is gone
    got, off = snapshot.read_header(path)
    assert got == hdr and off % 16 == 0 and os.path.getsize(path) == off + 4 * 3 * hdr["record_floats"][0]
    b = StubEngine()
    assert snapshot.load(path, b) == [4, 1, 3]
    (ids, recs, cache), = b.imported
    assert ids == [4, 1, 3] and cache is True
    np.testing.assert_array_equal(recs, a.export_streams([4, 1, 3], True))
    c = StubEngine()
    assert snapshot.load(path, c, ids=[0, 5, 2]) == [0, 5, 2] and c.imported[0][0] == [0, 5, 2]      # a move into other slots

    def refused(pattern, target=None, ids=None, file=path):
        t = target or StubEngine()
        with pytest.raises(VapxError, match=pattern):
            snapshot.load(file, t, ids)
        assert t.imported == []

    refused("ctx_frames", StubEngine(T=70))
    refused("frame_hz", StubEngine(hz=10))
    refused("modes", StubEngine(mode="bc"))
    refused("split_f16", StubEngine(split_f16=True))
    refused("ids", StubEngine(max_streams=4))                                     # slot 4 does not exist there
    refused("ids", ids=[1, 1, 2])
    refused("3 records", ids=[1, 2])
    blob = open(path, "rb").read()

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p

    refused("truncated", file=variant("cut", blob[:-8]))
    refused("too long", file=variant("long", blob + b"\0" * 16))
    refused("truncated inside the header", file=variant("head", blob[:20]))
    refused("magic", file=variant("magic", b"NOTASNAP" + blob[8:]))
    (jl,) = struct.unpack("<I", blob[8:12])
    h2 = dict(hdr, version=2)
    js = json.dumps(h2, separators=(",", ":")).encode()
    assert len(js) == jl
    refused("version 2", file=variant("v2", blob[:12] + js + blob[12 + jl:]))
    h3 = {k: v for k, v in hdr.items() if k != "cache"}
    js = json.dumps(h3, separators=(",", ":")).encode()
    refused("lacks the field cache", file=variant("nofield", blob[:8] + struct.pack("<I", len(js)) + js))
    # a record header that does not fit is found before anything is imported, in a follower block as well
    bad = bytearray(blob)
    struct.pack_into("<i", bad, off + 4 * hdr["record_floats"][0] + 4 * 4, 51)     # record 1: n_frames = T + 1
    refused(r"record 1: n_frames 51", file=variant("nframes", bytes(bad)))
    # without cache the precision path does not matter
    p2 = str(tmp_path / "nocache.vapx")
    assert snapshot.save(p2, a, ids=[0], cache=False)["cache"] is False
    d = StubEngine(split_f16=True)
    snapshot.load(p2, d)
    assert d.imported[0][2] is False and d.imported[0][1].shape == (1, engine.state_record_floats(50))


def test_snapshot_travels_in_bounded_pieces(tmp_path, monkeypatch):
    """Save and load move at most CHUNK_BYTES of records per engine call; the file is the same as in one piece."""
    a = StubEngine()
    whole, pieces = str(tmp_path / "whole"), str(tmp_path / "pieces")
    snapshot.save(whole, a)
    monkeypatch.setattr(snapshot, "CHUNK_BYTES", 4 * engine.state_record_floats(50, True) * 2 + 100)       # two records per piece
    calls = []
    orig = a.export_streams
    # StubEngine's payload is seeded by the number of ids: serve the pieces from one whole export instead
    full = orig(None, True)
    monkeypatch.setattr(a, "export_streams", lambda ids=None, cache=False: (calls.append(list(ids)), full[list(ids)])[1])
    snapshot.save(pieces, a)
    assert calls == [[0, 1], [2, 3], [4, 5]]
    monkeypatch.setattr(a, "export_streams", orig)
    assert open(pieces, "rb").read() == open(whole, "rb").read()
    b = StubEngine()
    assert snapshot.load(pieces, b, ids=[5, 4, 3, 2, 1, 0]) == [5, 4, 3, 2, 1, 0]
    assert [i for i, _, _ in b.imported] == [[5, 4], [3, 2], [1, 0]]
    np.testing.assert_array_equal(np.concatenate([r for _, r, _ in b.imported]), full)
    with pytest.raises(VapxError, match="does not continue block"):
        snapshot.write_file(str(tmp_path / "bad"), snapshot.read_header(whole)[0], [full[:, :-1]])
    with pytest.raises(VapxError, match="incomplete"):
        snapshot.write_file(str(tmp_path / "bad"), snapshot.read_header(whole)[0], [full[:4]])
    assert not os.path.exists(str(tmp_path / "bad")) and sorted(os.listdir(tmp_path)) == ["pieces", "whole"]


def test_snapshot_rename_is_atomic(tmp_path, monkeypatch):
    a = StubEngine()
    path = str(tmp_path / "s.vapx")
    snapshot.save(path, a, ids=[0])
    old = open(path, "rb").read()
    seen = {}

    def failing_replace(src, dst):
        seen["tmp"] = src
        assert os.path.exists(src) and open(dst, "rb").read() == old             # the old file is whole until the rename
        raise OSError("disk full")

    monkeypatch.setattr(os, "replace", failing_replace)
    with pytest.raises(OSError):
        snapshot.save(path, a, ids=[0, 1])
    monkeypatch.undo()
    assert seen["tmp"].startswith(path + ".tmp.") and not os.path.exists(seen["tmp"]) and open(path, "rb").read() == old


def test_group_snapshot_refuses_before_touching_the_leader(tmp_path):
    g = StubGroup()
    path = str(tmp_path / "g.vapx")
    hdr = snapshot.save(path, g, ids=[2, 0])
    assert hdr["modes"] == ["bc", "nod"] and hdr["record_floats"] == [engine.state_record_floats(50, True), engine.state_record_floats(50, True, True)]
    g2 = StubGroup()
    snapshot.load(path, g2)
    assert [e.imported[0][0] for e in g2.engines.values()] == [[2, 0], [2, 0]]
    assert g2.engines["nod"].imported[0][1].shape[1] == hdr["record_floats"][1]
    with pytest.raises(VapxError, match="modes"):
        snapshot.load(path, StubGroup(modes=("nod", "bc")))
    with pytest.raises(VapxError, match="modes"):
        snapshot.load(path, StubEngine(mode="bc"))
    _, off = snapshot.read_header(path)
    bad = bytearray(open(path, "rb").read())
    struct.pack_into("<i", bad, off + 4 * 2 * hdr["record_floats"][0] + 3 * 4, engine.STATE_HAS_LSTM)   # follower record 0 claims an LSTM
    open(path, "wb").write(bytes(bad))
    g3 = StubGroup()
    with pytest.raises(VapxError, match="nod record 0: content bits"):
        snapshot.load(path, g3)
    assert all(e.imported == [] for e in g3.engines.values())


def test_serve_state_arguments(tmp_path, capsys):
    assert serve.state_path(None, 0, 1) is None
    assert serve.state_path("/x/state", 0, 1) == "/x/state"
    assert [serve.state_path("/x/state", r, 3) for r in range(3)] == ["/x/state.0", "/x/state.1", "/x/state.2"]
    assert serve.state_path("/x/state", 0, 1, worker=True) == "/x/state.0"        # a worker process names its rank even when alone
    a = StubEngine()
    missing = str(tmp_path / "nothing.vapx")
    assert serve.load_state(missing, a, "GPU 0: ") is False and a.imported == []     # cold start ...
    err = capsys.readouterr().err
    assert "WARNING" in err and "cold start" in err and missing in err              # ... with a warning
    assert serve.load_state(None, a) is False
    path = str(tmp_path / "state.vapx")
    assert serve.save_state(path, a) is True and serve.save_state(None, a) is False
    b = StubEngine()
    assert serve.load_state(path, b) is True and b.imported[0][0] == list(range(6))
    c = StubEngine(T=70)
    with pytest.raises(VapxError, match="ctx_frames"):                              # a mismatching file is refused, nothing imported
        serve.load_state(path, c)
    assert c.imported == []
    assert serve.save_state(str(tmp_path / "no" / "such" / "dir" / "s"), a) is False   # reported, the shutdown goes on
    assert "failed" in capsys.readouterr().err


def test_serve_parses_the_state_flags_and_refuses_a_mismatch_at_start_up(tmp_path, monkeypatch, capsys):
    """main() with the engine and front-end replaced by stubs: --load_state happens after the engine is built and before the front-end
    opens, a mismatching file ends start-up with exit code 1 and no front-end, --save_state writes after the front-end closed."""
    from vap_realtime_amd import ingest
    order, made = [], {"engines": [], "shards": []}

    class Eng(StubEngine):
        def __init__(self, blob, hz, ctx, max_streams=1, **kw):
            super().__init__(T=int(ctx * hz), hz=hz, mode=kw.get("mode", "vap"), max_streams=max_streams, split_f16=kw.get("split_f16", False))
            order.append("engine")
            made["engines"].append(self)

        def import_streams(self, ids, records, cache=None):
            order.append("import")
            super().import_streams(ids, records, cache)

        def export_streams(self, ids=None, cache=False):
            order.append("export")
            return super().export_streams(ids, cache)

        def close(self):
            order.append("engine closed")

    class Srv:
        port_in, port_out = 1, 2

        def __init__(self, eng, **kw):
            order.append("front-end open")
            made["reset_on_connect"], made["keep_state"] = kw["reset_on_connect"], kw["keep_state"]
            made["shards"].append(self)

        def close(self):
            order.append("front-end closed")

    monkeypatch.setattr(engine, "Engine", Eng)
    monkeypatch.setattr(ingest, "NativeServer", Srv)
    monkeypatch.setattr(serve, "load_blob", lambda args: (None, "vap"))
    monkeypatch.setattr(serve.signal, "signal", lambda *a: None)
    monkeypatch.setattr(serve.time, "sleep", lambda s: (_ for _ in ()).throw(KeyboardInterrupt))
    good, out = str(tmp_path / "good"), str(tmp_path / "out")
    snapshot.save(good, StubEngine(max_streams=3))
    base = ["--synthetic-weights", "0", "--streams", "3", "--precision", "fp32", "--worker-procs", "off", "--stats_sec", "0"]
    # the service loop is left through the stubbed sleep; teardown is what it runs after a SIGTERM / SIGINT
    with pytest.raises(KeyboardInterrupt):
        serve.main(base + ["--load_state", good, "--save_state", out])
    assert order == ["engine", "import", "front-end open"]
    assert made["reset_on_connect"] is False and made["keep_state"] is True      # loaded state must survive the open and the (re)connects
    order.clear()
    serve.teardown(made["engines"], made["shards"], None, out)
    assert order == ["front-end closed", "export", "engine closed"] and os.path.exists(out)
    assert snapshot.read_header(out)[0]["ids"] == [0, 1, 2]
    # a snapshot of another window: refused, exit code 1, the front-end never opens
    order.clear()
    rc = serve.main(base + ["--context_len_sec", "3.5", "--load_state", good])
    assert rc == 1 and "front-end open" not in order and "import" not in order
    assert "ctx_frames" in capsys.readouterr().err
    # a missing file: warning, cold start, the service comes up
    order.clear()
    with pytest.raises(KeyboardInterrupt):
        serve.main(base + ["--load_state", str(tmp_path / "absent")])
    assert order[:2] == ["engine", "front-end open"] and "cold start" in capsys.readouterr().err
    assert made["reset_on_connect"] is True and made["keep_state"] is False      # a cold engine keeps today's behaviour
