"""Snapshot files of stream state: what ``serve --save_state`` writes on shutdown and ``--load_state`` reads at start-up, and what a
GPU-to-GPU move carries (INTEGRATION.md "Snapshots and migration").

A file is the state records of ``Engine.export_streams`` (include/vapx.h "Bulk state export / import") behind a small header::

    8 bytes   b"VAPXSNP1"
    4 bytes   length of the JSON header, little-endian u32
    JSON      {"version", "frame_hz", "ctx_frames", "modes" (attach order, the first leads), "split_f16" (the precision path the
               records' Q|K|V cache was made on), "cache", "ids" (stream slots, one record each), "record_floats" (per mode),
               and "input_hz" ONLY when the engine takes audio at another rate than 16000 (a file without the key is a 16 kHz file)}
    padding   zero bytes up to a multiple of 16
    records   per mode in ``modes`` order: float32 [len(ids)][record_floats[mode]], little-endian

It is written to a temporary name next to the target and renamed, so a reader never sees half a file.  ``load`` validates the header
and every record header against the target BEFORE any stream is touched and raises ``VapxError`` naming the field; header parsing and
validation need no GPU (``read_header`` / ``validate`` / ``check_records`` take plain descriptions).  Records travel in pieces of at
most ``CHUNK_BYTES`` in both directions (the file is mapped, not read), so a 4096-stream engine with 2 MB records needs no 8 GB of host
memory to be saved or loaded.
"""
from __future__ import annotations

import json
import os
import struct
from typing import Optional, Sequence

import numpy as np

from .engine import (STATE_CACHE_SPLIT, STATE_HAS_CACHE, STATE_HAS_LSTM, STATE_HAS_RESAMPLE, STATE_HEADER_FLOATS, STATE_MAGIC, VapxError,
                     state_record_floats)

FILE_MAGIC = b"VAPXSNP1"
VERSION = 1
CHUNK_BYTES = 256 << 20
_FIELDS = ("version", "frame_hz", "ctx_frames", "modes", "split_f16", "cache", "ids", "record_floats")


def describe(target) -> dict:
    """What a snapshot must match: of an ``Engine`` or a ``TrunkGroup`` (anything with these attributes: the CPU tests pass stubs)."""
    if hasattr(target, "engines"):
        lead = target.engines[target.modes[0]]
        modes = list(target.modes)
    else:
        lead, modes = target, [target.mode]
    desc = {"frame_hz": int(lead.frame_hz), "ctx_frames": int(lead.T), "modes": modes, "split_f16": bool(getattr(lead, "split_f16", False)),
            "max_streams": int(lead.max_streams)}
    if int(getattr(lead, "input_hz", 16000)) != 16000:       # the leader owns the audio; 16 kHz descriptions stay as they were
        desc["input_hz"] = int(lead.input_hz)
    return desc


def make_header(desc: dict, ids: Sequence[int], cache: bool) -> dict:
    T, in_hz = desc["ctx_frames"], int(desc.get("input_hz", 16000))
    hdr = {"version": VERSION, "frame_hz": desc["frame_hz"], "ctx_frames": T, "modes": list(desc["modes"]),
           "split_f16": bool(desc["split_f16"]), "cache": bool(cache), "ids": [int(i) for i in ids],
           "record_floats": [state_record_floats(T, cache, follower=k > 0, input_hz=in_hz) for k in range(len(desc["modes"]))]}
    if in_hz != 16000:
        hdr["input_hz"] = in_hz
    return hdr


def _data_offset(json_len: int) -> int:
    return (len(FILE_MAGIC) + 4 + json_len + 15) // 16 * 16


def write_file(path: str, header: dict, pieces):
    """Header + the record blocks, written to ``path + ".tmp.<pid>"`` and renamed over ``path``.  ``pieces``: an iterable of float32
    arrays [rows, record_floats[mode]] that, in order, make up one block of ``len(ids)`` records per mode."""
    js = json.dumps(header, separators=(",", ":")).encode()
    tmp = f"{path}.tmp.{os.getpid()}"
    n, sizes = len(header["ids"]), [int(x) for x in header["record_floats"]]
    mode, rows = 0, 0
    try:
        with open(tmp, "wb") as f:
            f.write(FILE_MAGIC + struct.pack("<I", len(js)) + js)
            f.write(b"\0" * (_data_offset(len(js)) - f.tell()))
            for blk in pieces:
                blk = np.ascontiguousarray(blk, dtype="<f4")
                if mode < len(sizes) and rows == n:
                    mode, rows = mode + 1, 0
                if mode >= len(sizes) or blk.ndim != 2 or blk.shape[1] != sizes[mode] or rows + blk.shape[0] > n:
                    raise VapxError(f"snapshot piece of shape {blk.shape} does not continue block {mode} ({rows} of {n} records of "
                                    f"{sizes[mode] if mode < len(sizes) else '-'} floats written)")
                f.write(memoryview(blk).cast("B"))
                rows += blk.shape[0]
            if n and (mode != len(sizes) - 1 or rows != n):
                raise VapxError(f"snapshot incomplete: block {mode} has {rows} of {n} records")
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def read_header(path: str):
    """(header dict, offset of the records).  Raises ``VapxError`` for a file that is not a snapshot, has an unknown version, lacks a
    field, or is shorter (or longer) than its header says."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(len(FILE_MAGIC) + 4)
        if len(head) < len(FILE_MAGIC) + 4 or head[:len(FILE_MAGIC)] != FILE_MAGIC:
            raise VapxError(f"{path}: not a vapx snapshot (magic)")
        (jl,) = struct.unpack("<I", head[len(FILE_MAGIC):])
        js = f.read(jl)
    if len(js) != jl:
        raise VapxError(f"{path}: truncated inside the header")
    try:
        hdr = json.loads(js.decode())
    except (ValueError, UnicodeDecodeError) as e:
        raise VapxError(f"{path}: unreadable header: {e}") from None
    if not isinstance(hdr, dict) or hdr.get("version") != VERSION:
        raise VapxError(f"{path}: snapshot version {hdr.get('version') if isinstance(hdr, dict) else None}, this build reads version {VERSION}")
    for k in _FIELDS:
        if k not in hdr:
            raise VapxError(f"{path}: header lacks the field {k}")
    if len(hdr["record_floats"]) != len(hdr["modes"]):
        raise VapxError(f"{path}: record_floats names {len(hdr['record_floats'])} sizes for {len(hdr['modes'])} modes")
    off = _data_offset(jl)
    want = off + 4 * len(hdr["ids"]) * sum(int(x) for x in hdr["record_floats"])
    if size != want:
        raise VapxError(f"{path}: {size} bytes, the header describes {want}: the file is {'truncated' if size < want else 'too long'}")
    return hdr, off


def validate(hdr: dict, desc: dict, ids: Optional[Sequence[int]] = None) -> list:
    """Check a snapshot header against a target description (``describe``); returns the stream slots to load into (``ids`` or the
    file's).  Raises ``VapxError`` naming the field that does not fit."""
    for k in ("frame_hz", "ctx_frames"):
        if int(hdr[k]) != int(desc[k]):
            raise VapxError(f"snapshot {k} = {hdr[k]}, the engine has {k} = {desc[k]}")
    if int(hdr.get("input_hz", 16000)) != int(desc.get("input_hz", 16000)):
        raise VapxError(f"snapshot input_hz = {hdr.get('input_hz', 16000)}, the engine has input_hz = {desc.get('input_hz', 16000)}: the "
                        f"records of an engine with an input rate carry its resampler history")
    if list(hdr["modes"]) != list(desc["modes"]):
        raise VapxError(f"snapshot modes = {hdr['modes']}, the engine serves modes = {desc['modes']} (same models, same attach order)")
    if hdr["cache"] and bool(hdr["split_f16"]) != bool(desc["split_f16"]):
        raise VapxError(f"snapshot split_f16 = {bool(hdr['split_f16'])} with a Q|K|V cache, the engine runs split_f16 = {bool(desc['split_f16'])}: "
                        f"cached values differ between the precision paths (save with cache=False to move between them)")
    T = int(desc["ctx_frames"])
    for k, fl in enumerate(hdr["record_floats"]):
        want = state_record_floats(T, bool(hdr["cache"]), follower=k > 0, input_hz=int(desc.get("input_hz", 16000)))
        if int(fl) != want:
            raise VapxError(f"snapshot record_floats[{k}] = {fl}, a {'follower' if k else 'leader'} record of this engine has {want}")
    use = [int(i) for i in (hdr["ids"] if ids is None else ids)]
    if len(use) != len(hdr["ids"]):
        raise VapxError(f"{len(use)} ids for the snapshot's {len(hdr['ids'])} records")
    if len(set(use)) != len(use) or any(i < 0 or i >= desc["max_streams"] for i in use):
        raise VapxError(f"snapshot ids: {len(use)} slots, distinct and inside [0, {desc['max_streams']}) needed")
    return use


def check_records(records: np.ndarray, desc: dict, cache: bool, follower: bool, what: str = "record"):
    """The per-record header checks of vapx_import_streams, on the host and without an engine — so that a group load can refuse a bad
    follower block before its leader was touched."""
    hdr = np.ascontiguousarray(records[:, :STATE_HEADER_FLOATS]).view(np.int32)
    in_hz = int(desc.get("input_hz", 16000))
    in_hz = 0 if follower or in_hz == 16000 else in_hz       # header word [6]: 0 at 16 kHz and in a follower's records
    bits = ((0 if follower else STATE_HAS_LSTM) | (STATE_HAS_CACHE if cache else 0) | (STATE_CACHE_SPLIT if cache and desc["split_f16"] else 0)
            | (STATE_HAS_RESAMPLE if in_hz else 0))
    T = int(desc["ctx_frames"])
    for k, h in enumerate(hdr):
        for name, got, want in (("magic", int(h[0]), STATE_MAGIC), ("ctx_frames", int(h[1]), T), ("frame_hz", int(h[2]), int(desc["frame_hz"])),
                                ("input_hz", int(h[6]), in_hz), ("content bits", int(h[3]), bits)):
            if got != want:
                raise VapxError(f"{what} {k}: {name} {got:#x} does not match {want:#x}" if name in ("magic", "content bits")
                                else f"{what} {k}: {name} {got} differs from the engine's {want}")
        if not 0 <= int(h[4]) <= T:
            raise VapxError(f"{what} {k}: n_frames {int(h[4])} outside [0,{T}]")


def _engines(target):
    return [target.engines[m] for m in target.modes] if hasattr(target, "engines") else [target]


def _chunks(n: int, record_floats: int):
    step = max(1, CHUNK_BYTES // (4 * max(1, int(record_floats))))
    return [(k0, min(n, k0 + step)) for k0 in range(0, n, step)]


def save(path: str, target, ids: Optional[Sequence[int]] = None, cache: bool = True) -> dict:
    """Export streams ``ids`` (None: every slot) of an ``Engine`` or a whole ``TrunkGroup`` into ``path``; returns the header.  Nobody may
    step the engines meanwhile: the records are exported in pieces."""
    desc = describe(target)
    ids = list(range(desc["max_streams"])) if ids is None else [int(i) for i in ids]
    hdr = make_header(desc, ids, cache)

    def pieces():
        for e, fl in zip(_engines(target), hdr["record_floats"]):
            for k0, k1 in _chunks(len(ids), fl):
                yield e.export_streams(ids[k0:k1], cache)

    write_file(path, hdr, pieces())
    return hdr


def load(path: str, target, ids: Optional[Sequence[int]] = None) -> list:
    """Import the streams of ``path`` into ``target`` (into slots ``ids``: None = the slots they were saved from); returns the slots.
    Nothing is imported unless the file header and every record header fit the target."""
    desc = describe(target)
    hdr, off = read_header(path)
    use = validate(hdr, desc, ids)
    n, cache = len(use), bool(hdr["cache"])
    if not n:
        return use
    blocks = []
    for k, fl in enumerate(hdr["record_floats"]):
        blk = np.memmap(path, dtype="<f4", mode="r", offset=off, shape=(n, int(fl)))
        off += 4 * n * int(fl)
        check_records(blk, desc, cache, follower=k > 0, what=f"{hdr['modes'][k]} record")
        blocks.append(blk)
    for e, blk in zip(_engines(target), blocks):
        for k0, k1 in _chunks(n, blk.shape[1]):
            e.import_streams(use[k0:k1], np.ascontiguousarray(blk[k0:k1], dtype=np.float32), cache)
    return use
