"""ctypes binding of libvapx.so (include/vapx.h) — the only way Python reaches the HIP path.

There is deliberately NO fallback: if the shared library is missing, was built for another
architecture, or no gfx950 device is visible, construction raises.  PyTorch is used only as the
owner of device buffers / HIP streams whose raw pointers are handed to the C ABI.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvapx.so")

OUT_STRIDE = 784
OUT_P_NOW, OUT_P_FUTURE, OUT_VAD, OUT_AUX, OUT_NVALID, OUT_LOGITS, OUT_E = 0, 2, 4, 6, 10, 16, 272
OUT_VAD_LOGIT = 11
OUT_STATUS = 13
STATUS_NO_FRAME = 2     # a slower trunk follower had no frame due for this stream on this leader tick (vapx.h VAPX_STATUS_NO_FRAME)
E_NUMERIC = -6
ABI_VERSION = 2
AUDIO_DEVICE, OUT_DEVICE, IDS_DEVICE = 1, 2, 4
# bulk state records (vapx.h "Bulk state export / import")
STATE_CACHE = 16
STATE_MAGIC = 0x31535056
STATE_HAS_LSTM, STATE_HAS_CACHE, STATE_CACHE_SPLIT = 1, 2, 4
STATE_HAS_RESAMPLE = 8   # the record carries a resampler history (an engine with an input rate), header word [6] = input_hz
STATE_HEADER_FLOATS = 8
STATE_LSTM_FLOATS, STATE_CARRY_FLOATS = 2 * 2 * 256, 2 * 320
MODE = {"vap": 0, "bc": 1, "nod": 2}

MAX_INPUT_CLASSES = 16
PROF_CLASSES = {0: "gemm_store", 1: "gemm_gelu", 2: "gemm_resid", 3: "gemm_resid_ln", 4: "gemm_cn_relu",
                5: "conv_tail", 6: "ffn_block", 7: "last_row", 8: "conv0", 9: "lstm", 10: "gather_ln", 11: "attention", 12: "head",
                13: "gemm_bias_ln_gelu", 14: "ffn_proj", 15: "trunk_collect"}


class VapxError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device_id", C.c_int32), ("frame_hz", C.c_int32),
                ("ctx_frames", C.c_int32), ("max_streams", C.c_int32), ("max_batch", C.c_int32),
                ("mode", C.c_int32), ("flags", C.c_int32)]


class _InputClass(C.Structure):
    _fields_ = [("input_hz", C.c_int32), ("format", C.c_int32)]


def _prototypes() -> dict:
    """Every export of include/vapx.h: ``name -> (restype, argtypes)`` or ``(restype, argtypes, True)`` for one that an older build
    may lack (``load_library`` then leaves it undeclared)."""
    P, vp, i32, i64, sz, dbl, text = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_size_t, C.c_double, C.c_char_p
    f32p = i32p = vp                     # device or host blocks, passed as raw addresses
    step = [vp, i32, i32p, f32p, i32, f32p, i32, vp]
    state_io = [vp, i32, i32p, f32p, i32, vp]
    rows = [vp, i64, f32p, f32p, vp]
    return {
        "vapx_abi_version": (i32, []),
        "vapx_blob_floats": (sz, [i32]),
        "vapx_create": (i32, [P(_Config), f32p, sz, P(vp)]),
        "vapx_destroy": (None, [vp]),
        "vapx_last_error": (text, [vp]),
        "vapx_get_config": (i32, [vp, P(_Config)]),
        "vapx_step": (i32, step),
        "vapx_join": (i32, [vp, vp]),
        "vapx_bad_slots": (i32, [vp, i32p, i32]),
        "vapx_attach_trunk": (i32, [vp, vp]),
        "vapx_wire_floats": (i32, [i32, i32]),
        "vapx_group_wire_floats": (sz, [vp]),
        "vapx_step_group": (i32, step),
        "vapx_group_bad": (i32, [vp, i32p, i32p, i32]),
        "vapx_reset_stream": (i32, [vp, i32]),
        "vapx_reset_carry": (i32, [vp, i32]),
        "vapx_get_state": (i32, [vp, i32, f32p, P(i32), f32p, f32p]),
        "vapx_set_state": (i32, [vp, i32, f32p, i32, f32p, f32p]),
        "vapx_state_floats": (sz, [vp, i32]),
        "vapx_export_streams": (i32, state_io),
        "vapx_import_streams": (i32, state_io),
        "vapx_prefill": (i32, [vp, i32, i32p, f32p, i32, i32, vp], True),
        "vapx_set_input_rate": (i32, [vp, i32]),
        "vapx_get_input_rate": (i32, [vp]),
        "vapx_resample": (i32, [i32, i64, i64, f32p, f32p, vp]),
        "vapx_set_input_format": (i32, [vp, i32]),
        "vapx_get_input_format": (i32, [vp]),
        "vapx_pcm_decode": (i32, [i32, i64, vp, f32p, vp]),
        "vapx_set_input_classes": (i32, [vp, i32, vp]),
        "vapx_get_input_classes": (i32, [vp, vp, i32]),
        "vapx_set_stream_class": (i32, [vp, i32, i32]),
        "vapx_get_stream_class": (i32, [vp, i32]),
        "vapx_input_slot_bytes": (i64, [vp, i32]),
        "vapx_set_stream_channel_classes": (i32, [vp, i32, i32, i32]),
        "vapx_get_stream_channel_classes": (i32, [vp, i32, vp]),
        "vapx_input_row_bytes": (i64, [vp, i32]),
        "vapx_encode_audio": (i32, [vp, i32, i32p, f32p, f32p, vp]),
        "vapx_transformer": (i32, [vp, i32, i32, f32p, f32p, f32p, f32p, i32, vp]),
        "vapx_transformer_maps": (i32, [vp, i32, i32, f32p, f32p, f32p, f32p, i32, f32p, f32p, f32p, vp]),
        "vapx_peek": (i64, [vp, text, f32p, sz]),
        "vapx_profile_enable": (i32, [vp, C.c_uint32]),
        "vapx_profile_read": (i32, [vp, P(dbl), P(i64), i32]),
        "vapx_host_alloc": (vp, [sz]),
        "vapx_host_free": (None, [vp]),
        "vapx_vap_head": (i32, rows),
        "vapx_va_classifier": (i32, rows),
        "vapx_aux_head": (i32, [vp, i32, i64, f32p, f32p, vp]),
        "vapx_softmax256": (i32, [i64, f32p, f32p, vp]),
        "vapx_aggregate": (i32, [i64, f32p, i32, i32, f32p, vp]),
        "vapx_gemm": (i32, [vp, i32, i32, i32, f32p, f32p, f32p, i32, f32p, f32p, f32p, f32p, f32p, i32]),
        "vapx_gemm_tile_rows": (i32, [i32, i32, i32, i32], True),
        "vapx_ingest_open": (i32, [vp, vp, P(vp)]),
        "vapx_ingest_open_fn": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, P(vp)]),
        "vapx_ingest_open_group": (i32, [vp, P(vp), i32, vp, P(i32), P(vp)]),
        "vapx_ingest_open_group_fn": (i32, [vp, vp, vp, i32, i32, i32, i32, P(i32), i32, vp, P(i32), P(vp)]),
        "vapx_ingest_open_group_fn2": (i32, [vp, vp, vp, i32, i32, P(i32), P(i32), P(i32), i32, vp, P(i32), P(vp)]),
        "vapx_ingest_last_open_error": (text, []),
        "vapx_ingest_ports": (i32, [vp, P(i32), P(i32)]),
        "vapx_ingest_group_ports": (i32, [vp, P(i32), P(i32), i32]),
        "vapx_ingest_class_ports": (i32, [vp, vp, i32]),
        "vapx_ingest_pair_ports": (i32, [vp, vp, i32]),
        "vapx_ingest_stream_class": (i32, [vp, i32]),
        "vapx_ingest_stream_channel_classes": (i32, [vp, i32, vp]),
        "vapx_ingest_attach_link": (i32, [vp, i32]),
        "vapx_ingest_stats_read": (i32, [vp, vp, i32]),
        "vapx_ingest_late_read": (i32, [vp, vp, vp]),
        "vapx_ingest_close": (None, [vp]),
        "vapx_frontdoor_open": (i32, [vp, i32, i32, i32, i32, P(vp)]),
        "vapx_frontdoor_open_links": (i32, [P(i32), i32, i32, i32, i32, P(vp)]),
        "vapx_frontdoor_ports": (i32, [vp, P(i32), P(i32)]),
        "vapx_frontdoor_counts": (i32, [vp, P(i64), P(i64), P(i64)]),
        "vapx_frontdoor_close": (None, [vp]),
        "vapx_wire_decode_input": (i64, [vp, sz, dbl, vp, vp, vp, vp]),
        "vapx_wire_encode_result": (i64, [i32, dbl, vp, vp, i32, vp, vp, sz]),
    }


PROTOTYPES = _prototypes()
EXPORTS = tuple(PROTOTYPES)


def input_class_table(classes) -> list:
    """``[(format, rate), ...]`` as ``[(format name, rate in Hz)]``: formats by name or id ("f32" / "s16" / "mulaw" / "alaw", vapx.h VAPX_PCM_*),
    rates 8000 / 16000 / 32000 / 48000; 1 .. 16 entries, no two equal (the rules of ``vapx_set_input_classes``)."""
    from . import pcm
    tab = [(pcm.format_name(f), int(hz)) for f, hz in classes]
    if not 1 <= len(tab) <= MAX_INPUT_CLASSES:
        raise ValueError(f"{len(tab)} input classes: the table holds 1 .. {MAX_INPUT_CLASSES}")
    for f, hz in tab:
        if hz not in (8000, 16000, 32000, 48000):
            raise ValueError(f"input rate {hz} Hz: supported are 8000, 16000, 32000 and 48000")
    if len(set(tab)) != len(tab):
        raise ValueError("two equal input classes")
    return tab


def input_slot_shape(cls, frame_hz: int):
    """``(dtype, [2, hop_in])`` of one batch slot of class ``cls = (format, rate)``."""
    from . import pcm
    f, hz = cls
    return pcm.DTYPES[pcm.format_name(f)], (2, int(hz) // frame_hz)


def input_slot_bytes(cls, frame_hz: int) -> int:
    """Bytes of one batch slot of class ``cls``: 2 * hop_in * bytes per sample, a multiple of 16 (vapx.h, vapx_input_slot_bytes)."""
    dt, (two, hop_in) = input_slot_shape(cls, frame_hz)
    return two * hop_in * dt.itemsize


def aligned_bytes(n: int, align: int = 16) -> np.ndarray:
    """A uint8 array of n bytes whose first byte sits on a multiple of ``align``."""
    raw = np.empty(n + align, np.uint8)
    at = (-raw.ctypes.data) % align
    return raw[at:at + n]


def input_row_bytes(cls, frame_hz: int) -> int:
    """Bytes of one channel's row of class ``cls``: hop_in * bytes per sample, a multiple of 16 (vapx.h, vapx_input_row_bytes)."""
    return input_slot_bytes(cls, frame_hz) // 2


def _slot_pair(c):
    """A batch slot's classes as ``(c1, c2)``: a class index means both channels."""
    if isinstance(c, (tuple, list, np.ndarray)):
        if len(c) != 2:
            raise ValueError(f"a batch slot's classes are one index or a pair (c1, c2), not {c!r}")
        return int(c[0]), int(c[1])
    return int(c), int(c)


def pack_input_classes(classes, frame_hz: int, slot_classes: Sequence, arrays, out: Optional[np.ndarray] = None) -> np.ndarray:
    """The packed audio block of one step on an engine with input classes (vapx.h "Input classes", LAYOUT).  ``slot_classes[k]`` is a class
    index c_k, and ``arrays[k]`` [2, hop_in(c_k)] samples of format(c_k); or a pair (c1, c2), the classes of the stream's two channels, and
    ``arrays[k]`` a pair of 1-D arrays: hop_in(c1) samples of format(c1), then hop_in(c2) of format(c2) (a class index takes such a pair
    too).  Slot k starts at the sum of the earlier slots' bytes, channel 1's row first; a pair (c, c) is the block of the index c byte for
    byte.  The dtype of every array is checked as ``Engine.step`` checks a uniform engine's: float arrays of any width are cast for "f32",
    a raw format takes its own dtype only.  Returns a 16-byte aligned uint8 block (``out``, e.g. a view of a ``pinned_empty`` block, if
    given)."""
    tab = input_class_table(classes)
    if len(slot_classes) != len(arrays):
        raise ValueError(f"{len(arrays)} arrays for {len(slot_classes)} batch slots")
    pairs = [_slot_pair(c) for c in slot_classes]
    total = int(sum(input_row_bytes(tab[c], frame_hz) for p in pairs for c in p))
    if out is None:
        out = aligned_bytes(total)
    block = out.reshape(-1).view(np.uint8)[:total]
    if block.size != total or block.ctypes.data % 16:
        raise ValueError("the packed block must hold every slot and start on a 16-byte boundary")
    at = 0
    for k, (pair, a) in enumerate(zip(pairs, arrays)):
        if hasattr(a, "detach") and hasattr(a, "numpy"):
            a = a.detach().cpu().numpy()
        planar = isinstance(a, (tuple, list))
        if planar and len(a) != 2:
            raise ValueError(f"batch slot {k}: a pair of per-channel arrays has two entries, not {len(a)}")
        if not planar:
            if pair[0] != pair[1]:
                raise TypeError(f"batch slot {k}: channel classes {pair} take a pair of 1-D arrays, one per channel")
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[0] != 2:
                dt, shape = input_slot_shape(tab[pair[0]], frame_hz)
                raise ValueError(f"batch slot {k}: class {pair[0]} ({tab[pair[0]][0]} at {tab[pair[0]][1]} Hz) takes {list(shape)} samples, not {list(a.shape)}")
        for ch, c in enumerate(pair):
            dt, (_, hop_in) = input_slot_shape(tab[c], frame_hz)
            r = a[ch]
            if hasattr(r, "detach") and hasattr(r, "numpy"):
                r = r.detach().cpu().numpy()
            r = np.asarray(r)
            if tab[c][0] == "f32":
                r = np.ascontiguousarray(r, dtype=np.float32)
            elif r.dtype != dt:
                raise TypeError(f"batch slot {k}: class {c} ({tab[c][0]} at {tab[c][1]} Hz) takes {dt.name} samples, not {r.dtype.name}")
            if r.shape != (hop_in,):
                shape = [hop_in] if planar else [2, hop_in]
                raise ValueError(f"batch slot {k}: class {c} ({tab[c][0]} at {tab[c][1]} Hz) takes {shape} samples, not {list(r.shape if planar else a.shape)}")
            nb = hop_in * dt.itemsize
            block[at:at + nb] = np.ascontiguousarray(r).view(np.uint8)
            at += nb
    return block


_lib = None


def load_library(path: Optional[str] = None):
    """dlopen libvapx.so and declare prototypes.  Import torch first when it is going to be used in
    the same process so both share one HIP runtime (same SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("VAPX_LIBRARY") or LIB_PATH     # VAPX_LIBRARY: the debug build with phase stamps (make trace)
    if not os.path.exists(p):
        raise VapxError(f"{p} not found — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"(or `make -C vap-realtime_amd/csrc`). There is no CPU fallback.")
    try:
        import torch  # noqa: F401  (loads torch's bundled libamdhip64 first when torch is installed)
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (restype, argtypes, *optional) in PROTOTYPES.items():
        if optional and not hasattr(lib, name):   # an older build named by VAPX_LIBRARY for an A/B run (tools/ab_lib.sh); build() checks EXPORTS
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


def _np_ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _PinnedOwner:
    """Frees a vapx_host_alloc block when the last numpy view of it is collected."""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        try:
            self.lib.vapx_host_free(self.ptr)
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float32) -> np.ndarray:
    """numpy array in page-locked host memory (vapx_host_alloc): ``Engine.step`` DMAs straight from / into such arrays
    instead of staging through the engine's own pinned buffers."""
    lib = load_library()
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    ptr = lib.vapx_host_alloc(max(nbytes, 1))
    if not ptr:
        raise VapxError(f"vapx_host_alloc({nbytes}) failed")
    owner = _PinnedOwner(lib, ptr)
    buf = (C.c_char * max(nbytes, 1)).from_address(ptr)
    buf._owner = owner                                   # the ctypes buffer is the numpy base: keeps the block alive
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


class Engine:
    """One engine = one GPU: device weights + state of ``max_streams`` dialogue streams.

    Mirrors ``VAPRealTime(vap_model, cpc_model, device, frame_rate, context_len_sec)``
    (rvap/vap_main/vap_main.py:192-247) with the weights given as a packed blob
    (``weights.pack_blob``)."""

    def __init__(self, blob: np.ndarray, frame_hz: int = 20, context_len_sec: float = 2.5,
                 max_streams: int = 1, max_batch: Optional[int] = None, mode: str = "vap", device_id: int = 0,
                 groups: int = 0, full_last_layer: bool = False, unfused_conv: bool = False,
                 materialize_x0: bool = False, unfused_last_row: bool = False, split_f16: bool = False,
                 unfused_proj: bool = False, split_qkv_in_ffn: bool = False, input_hz: int = 16000,
                 input_format: str = "f32", input_classes=None):
        from . import pcm
        self.input_classes = None                           # [(format name, rate)]: every stream has a class of its own (vapx.h "Input classes")
        if input_classes is not None:
            if int(input_hz) != 16000 or pcm.format_name(input_format) != "f32":
                raise ValueError("input_classes replaces input_hz / input_format: give the table alone")
            self.input_classes = input_class_table(input_classes)
        self.lib = load_library()
        self.input_format = pcm.format_name(input_format)   # sample format of the audio ``step`` takes (vapx.h, vapx_set_input_format)
        self.frame_hz = frame_hz
        self.T = int(context_len_sec * frame_hz)           # vap_main.py:221
        self.hop = 16000 // frame_hz
        self.L = self.hop + 320                             # vap_main.py:230
        self.input_hz = int(input_hz)                       # sample rate of the audio ``step`` takes (vapx.h, vapx_set_input_rate)
        self.hop_in = self.input_hz // frame_hz             # samples per channel and tick at that rate (== hop at 16 kHz)
        self.max_streams = max_streams
        self.max_batch = max_batch or max_streams
        self.mode = mode
        self.device_id = device_id
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        flags = ((groups & 0xF) | (16 if full_last_layer else 0) | (32 if unfused_conv else 0)
                 | (64 if materialize_x0 else 0) | (256 if unfused_last_row else 0) | (512 if split_f16 else 0) | (1024 if unfused_proj else 0)
                 | (2048 if split_qkv_in_ffn else 0))
        self.split_f16 = bool(split_f16)
        cfg = _Config(C.sizeof(_Config), device_id, frame_hz, self.T, max_streams, self.max_batch, MODE[mode], flags)
        h = C.c_void_p()
        rc = self.lib.vapx_create(C.byref(cfg), _np_ptr(blob), blob.size, C.byref(h))
        if rc != 0:
            raise VapxError(f"vapx_create failed ({rc}): {self.lib.vapx_last_error(None).decode()}")
        self._h = h
        if self.input_hz != 16000:
            rc = self.lib.vapx_set_input_rate(h, self.input_hz)
            if rc != 0:
                msg = self.lib.vapx_last_error(h).decode()
                self.close()
                raise VapxError(f"vapx_set_input_rate failed ({rc}): {msg}")
        if self.input_format != "f32":
            rc = self.lib.vapx_set_input_format(h, pcm.FORMATS[self.input_format])
            if rc != 0:
                msg = self.lib.vapx_last_error(h).decode()
                self.close()
                raise VapxError(f"vapx_set_input_format failed ({rc}): {msg}")
        if self.input_classes is not None:
            tab = (_InputClass * len(self.input_classes))(*[_InputClass(hz, pcm.FORMATS[f]) for f, hz in self.input_classes])
            rc = self.lib.vapx_set_input_classes(h, len(self.input_classes), C.cast(tab, C.c_void_p))
            if rc != 0:
                msg = self.lib.vapx_last_error(h).decode()
                self.close()
                raise VapxError(f"vapx_set_input_classes failed ({rc}): {msg}")
            self._mirror_input_classes()

    # -- input classes ---------------------------------------------------------------------------
    def _mirror_input_classes(self):
        """The host's copy of every (stream, channel)'s class and every class's row size: a step sizes its packed block without a library
        call per slot."""
        self._cls = np.zeros((self.max_streams, 2), np.int64)
        self._row_bytes = np.array([input_row_bytes(c, self.frame_hz) for c in self.input_classes], np.int64)

    def set_stream_class(self, sid: int, cls: int):
        """Move stream ``sid`` to input class ``cls``: queued like ``reset_carry``; the next step zeroes the stream's carry and resampler
        history first (a new class is a new signal) and keeps its LSTM and context window."""
        self._check(self.lib.vapx_set_stream_class(self._h, sid, cls), "vapx_set_stream_class")
        self._cls[sid] = cls

    def stream_class(self, sid: int) -> int:
        return self._check(self.lib.vapx_get_stream_class(self._h, sid), "vapx_get_stream_class")

    def set_stream_channel_classes(self, sid: int, c1: int, c2: int):
        """Give the two channels of stream ``sid`` the input classes ``c1`` and ``c2`` (a dialogue whose legs arrive in different codecs):
        the rules of ``set_stream_class``, and the carry and the history of both channels restart."""
        self._check(self.lib.vapx_set_stream_channel_classes(self._h, sid, c1, c2), "vapx_set_stream_channel_classes")
        self._cls[sid] = (c1, c2)

    def stream_channel_classes(self, sid: int) -> tuple:
        out = (C.c_int32 * 2)()
        self._check(self.lib.vapx_get_stream_channel_classes(self._h, sid, out), "vapx_get_stream_channel_classes")
        return int(out[0]), int(out[1])

    def refresh_stream_classes(self):
        """Re-read every channel's class from the library: after somebody else moved streams (a ``NativeServer`` does for every connection)."""
        for s in range(self.max_streams):
            self._cls[s] = self.stream_channel_classes(s)

    def input_slot_bytes(self, cls: int) -> int:
        return int(self.lib.vapx_input_slot_bytes(self._h, cls))

    def input_row_bytes(self, cls: int) -> int:
        return int(self.lib.vapx_input_row_bytes(self._h, cls))

    def pack_input(self, stream_ids: Optional[Sequence[int]], arrays, out: Optional[np.ndarray] = None) -> np.ndarray:
        """The packed block ``step`` takes for these streams in this batch order (``stream_ids`` None = 0 .. n-1): array k is
        [2, hop_in] samples in the class of ``stream_ids[k]``, or a pair of 1-D arrays in its two channels' classes
        (``pack_input_classes``)."""
        if self.input_classes is None:
            raise VapxError("this engine has no input classes")
        ids = np.arange(len(arrays)) if stream_ids is None else np.asarray(stream_ids, dtype=np.int64)
        slot_classes = [int(c1) if c1 == c2 else (int(c1), int(c2)) for c1, c2 in self._cls[ids]]
        return pack_input_classes(self.input_classes, self.frame_hz, slot_classes, arrays, out)

    def _packed_audio(self, audio, stream_ids):
        """``(block, n)`` of a step on an engine with input classes: ``audio`` is a list of per-slot arrays (packed here) or one packed
        uint8 block, whose size must be what the streams' classes add up to."""
        if isinstance(audio, np.ndarray) and audio.dtype == np.uint8 and audio.ndim == 1:
            if stream_ids is None:
                raise ValueError("a packed block needs stream_ids: its slots are sized by their streams' classes")
            need = int(self._row_bytes[self._cls[np.asarray(stream_ids, dtype=np.int64)]].sum())
            if audio.size != need:
                raise ValueError(f"the packed block has {audio.size} bytes, the classes of these {len(stream_ids)} streams add up to {need}")
            if not audio.flags.c_contiguous or audio.ctypes.data % 16:
                aligned = aligned_bytes(audio.size)
                aligned[:] = audio
                audio = aligned
            return audio, len(stream_ids)
        return self.pack_input(stream_ids, audio), len(audio)

    # -- lifecycle -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.vapx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc < 0:
            raise VapxError(f"{what} failed ({rc}): {self.lib.vapx_last_error(self._h).decode()}")
        return rc

    # -- the step --------------------------------------------------------------------------------
    def _host_audio(self, audio):
        """The audio block of a host-path step as a contiguous array of the engine's input format: float32 for "f32" (anything numeric is
        cast, as ever); for a raw format the samples themselves, int16 ("s16") or uint8 ("mulaw" / "alaw") arrays or CPU tensors."""
        if hasattr(audio, "detach") and hasattr(audio, "numpy"):      # a torch tensor
            audio = audio.detach().cpu().numpy()
        if self.input_format == "f32":
            return np.ascontiguousarray(audio, dtype=np.float32)
        from . import pcm
        want = pcm.DTYPES[self.input_format]
        audio = np.asarray(audio)
        if audio.dtype != want:
            raise TypeError(f"an engine with input_format={self.input_format!r} takes {want.name} samples, not {audio.dtype.name}")
        return np.ascontiguousarray(audio)

    def pcm_decode(self, fmt, samples):
        """``vapx_pcm_decode``: a CUDA tensor of raw samples (int16 for "s16", uint8 for "mulaw" / "alaw"; numpy arrays are uploaded) ->
        a float32 CUDA tensor of the same shape, decoded by the kernel the engine's step uses."""
        import torch
        from . import pcm
        name = pcm.format_name(fmt)
        if name == "f32":
            raise ValueError("pcm_decode takes s16, mulaw or alaw samples")
        want = pcm.DTYPES[name]
        if not isinstance(samples, torch.Tensor):
            samples = np.asarray(samples)
            if samples.dtype != want:
                raise TypeError(f"{name} samples are {want.name}, not {samples.dtype.name}")
            samples = torch.from_numpy(np.ascontiguousarray(samples))
        if samples.dtype != (torch.int16 if name == "s16" else torch.uint8):
            raise TypeError(f"{name} samples are {want.name}, not {samples.dtype}")
        src = samples.to(f"cuda:{self.device_id}").contiguous()
        dst = torch.empty(src.shape, dtype=torch.float32, device=src.device)
        if src.numel():
            rc = self.lib.vapx_pcm_decode(pcm.FORMATS[name], src.numel(), src.data_ptr(), dst.data_ptr(),
                                          torch.cuda.current_stream(src.device).cuda_stream or None)
            if rc != 0:
                raise VapxError(f"vapx_pcm_decode failed ({rc})")
        return dst

    def step(self, audio: np.ndarray, stream_ids: Optional[Sequence[int]] = None, out: Optional[np.ndarray] = None,
             on_numeric: str = "raise") -> np.ndarray:
        """Host path.  audio: float [n,2,hop] (new samples; engine keeps the carry) or [n,2,hop+320]
        (complete frames as ``process_vap`` receives them); with ``input_hz`` other than 16000: [n,2,hop_in] and nothing else; with an
        ``input_format`` other than "f32": the same shapes as int16 ("s16") or uint8 ("mulaw" / "alaw") samples, any other dtype is refused.  Returns float32 [n, OUT_STRIDE] (``out`` if given, e.g. a
        ``pinned_empty`` block).  A stream with non-finite results (VAPX_E_NUMERIC) raises by default; with
        ``on_numeric="status"`` the block is returned — every other row is valid, the bad rows have column OUT_STATUS = 1
        and ``bad_slots()`` lists them."""
        if self.input_classes is not None:   # a list of per-slot arrays, [2, hop_in] each in its stream's class, or one packed uint8 block
            audio, n = self._packed_audio(audio, stream_ids)
            spc = 0
        else:
            audio = self._host_audio(audio)
            n, two, spc = audio.shape
            assert two == 2
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        if ids is not None:
            assert ids.shape == (n,)
        if out is None:
            out = np.empty((n, OUT_STRIDE), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= n * OUT_STRIDE
        rc = self.lib.vapx_step(self._h, n, _np_ptr(ids), _np_ptr(audio), spc, _np_ptr(out), 0, None)
        if not (rc == E_NUMERIC and on_numeric == "status"):
            self._check(rc, "vapx_step")
        return out.reshape(-1, OUT_STRIDE)[:n]

    # -- attach to a call in progress ------------------------------------------------------------------
    def _prefill_shape(self, shape, dtype_ok: bool, n_ids: Optional[int]) -> tuple:
        """(n, frames) of a prefill block of ``shape``; raises before any library call."""
        if not dtype_ok:
            raise TypeError("prefill takes float32 samples (16 kHz new samples as the step takes them)")
        if len(shape) != 3 or shape[1] != 2:
            raise ValueError(f"prefill audio must be [n, 2, frames * hop], got shape {tuple(shape)}")
        n, _, samples = (int(x) for x in shape)
        if n < 1 or samples < self.hop or samples % self.hop:
            raise ValueError(f"prefill audio {tuple(shape)}: n >= 1 and a whole number (>= 1) of {self.hop}-sample frames per channel are needed")
        if n_ids is not None and n_ids != n:
            raise ValueError(f"{n_ids} stream ids for {n} audio rows")
        return n, samples // self.hop

    def prefill(self, audio, stream_ids: Optional[Sequence[int]] = None):
        """Attach to a call in progress (vapx.h, vapx_prefill): ``audio`` float32 [n, 2, frames * hop], the streams' buffered 16 kHz
        history, as a numpy array (host: page-locked ``pinned_empty`` blocks are copied from directly, others staged in bounded blocks)
        or a torch CUDA tensor (read where it lies, enqueued on the current torch stream, no synchronisation).  Afterwards the streams'
        LSTM, carry, context window and layer-0 Q|K|V cache are what ``frames`` calls of ``step`` would have left; no output rows are
        made and no transformer layer runs.  ``stream_ids``: as in ``step`` (None: slots 0 .. n-1).  Returns the number of frames."""
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32).reshape(-1)
        n_ids = None if ids is None else int(ids.size)
        if hasattr(audio, "data_ptr") and hasattr(audio, "is_cuda"):          # a torch tensor
            import torch
            n, frames = self._prefill_shape(tuple(audio.shape), audio.dtype == torch.float32, n_ids)
            if audio.is_cuda:
                if not audio.is_contiguous():
                    raise ValueError("a device prefill block must be contiguous")
                stream = torch.cuda.current_stream(audio.device).cuda_stream or None
                self._check(self.lib.vapx_prefill(self._h, n, _np_ptr(ids), audio.data_ptr(), frames, AUDIO_DEVICE, stream), "vapx_prefill")
                return frames
            audio = audio.detach().numpy()
        audio = np.asarray(audio)
        n, frames = self._prefill_shape(audio.shape, audio.dtype == np.float32, n_ids)
        audio = np.ascontiguousarray(audio)
        if audio.ctypes.data % 16:                                            # the block must be 16-byte aligned (vapx.h)
            block = aligned_bytes(audio.nbytes).view(np.float32).reshape(audio.shape)
            block[...] = audio
            audio = block
        self._check(self.lib.vapx_prefill(self._h, n, _np_ptr(ids), _np_ptr(audio), frames, 0, None), "vapx_prefill")
        return frames

    def prefill_device(self, n: int, audio_ptr: int, frames: int, ids_ptr: int = 0, stream: int = 0):
        """Device twin of ``prefill``: raw device pointers, enqueued on ``stream``, no synchronisation."""
        flags = AUDIO_DEVICE | (IDS_DEVICE if ids_ptr else 0)
        self._check(self.lib.vapx_prefill(self._h, n, ids_ptr or None, audio_ptr, frames, flags, stream or None), "vapx_prefill")

    def bad_slots(self) -> list:
        """Batch slots of the latest host-path step whose results were not finite."""
        n = self.lib.vapx_bad_slots(self._h, None, 0)
        if n <= 0:
            return []
        buf = np.empty(n, np.int32)
        self.lib.vapx_bad_slots(self._h, _np_ptr(buf), n)
        return buf.tolist()

    def attach_trunk(self, leader: "Engine"):
        """Make this engine a follower of ``leader``: it shares the leader's CPC CNN + LSTM (vapx.h, vapx_attach_trunk)."""
        self._check(self.lib.vapx_attach_trunk(self._h, leader._h), "vapx_attach_trunk")
        self._leader = leader                                # keeps the leader alive as long as the follower

    def step_follow(self, n: int, out: Optional[np.ndarray] = None, on_numeric: str = "raise") -> np.ndarray:
        """Follower step on the host path: consumes the encoder output of the leader's latest ``step`` (``out`` / ``on_numeric``
        as in ``step``)."""
        if out is None:
            out = np.empty((n, OUT_STRIDE), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= n * OUT_STRIDE
        rc = self.lib.vapx_step(self._h, n, None, None, 0, _np_ptr(out), 0, None)
        if not (rc == E_NUMERIC and on_numeric == "status"):
            self._check(rc, "vapx_step")
        return out.reshape(-1, OUT_STRIDE)[:n]

    def step_follow_device(self, n: int, out_ptr: int, stream: int = 0):
        self._check(self.lib.vapx_step(self._h, n, None, None, 0, out_ptr, OUT_DEVICE, stream or None), "vapx_step")

    def join(self, stream: int = 0):
        self._check(self.lib.vapx_join(self._h, stream or None), "vapx_join")

    def step_device(self, n: int, audio_ptr: int, spc: int, out_ptr: int, ids_ptr: int = 0, stream: int = 0, defer_join: bool = False):
        """Device path: raw device pointers (e.g. ``tensor.data_ptr()``), work enqueued on ``stream``
        (a hipStream_t as int, 0 = default); returns immediately."""
        flags = AUDIO_DEVICE | OUT_DEVICE | (IDS_DEVICE if ids_ptr else 0) | (8 if defer_join else 0)
        self._check(self.lib.vapx_step(self._h, n, ids_ptr or None, audio_ptr, spc, out_ptr, flags, stream or None), "vapx_step")

    def step_packed_device(self, stream_ids: Optional[Sequence[int]], audio_ptr: int, out_ptr: int, stream: int = 0, n: Optional[int] = None):
        """Device path of an engine with input classes: ``audio_ptr`` is the packed block in device memory (16-byte aligned), the stream
        ids stay on the host (``None`` = 0 .. n-1): the engine computes every slot's offset from them."""
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        n = len(ids) if ids is not None else int(n)
        self._check(self.lib.vapx_step(self._h, n, _np_ptr(ids), audio_ptr, 0, out_ptr, AUDIO_DEVICE | OUT_DEVICE, stream or None), "vapx_step")

    # -- the whole trunk group in one call (this engine leads) -----------------------------------------
    def group_wire_floats(self) -> int:
        """Wire floats per stream of this leader and its followers together (vapx.h, vapx_group_wire_floats)."""
        return int(self.lib.vapx_group_wire_floats(self._h))

    def step_group(self, audio: np.ndarray, stream_ids: Optional[Sequence[int]] = None, out: Optional[np.ndarray] = None,
                   on_numeric: str = "raise") -> np.ndarray:
        """Host path of ``vapx_step_group``: steps this leader and every follower and returns the tick's wire block, flat float32
        [n * group_wire_floats()], model-major (``TrunkGroup.step_wire`` slices it).  ``out``: e.g. a ``pinned_empty`` block.
        ``on_numeric`` as in ``step``; ``group_bad()`` lists the (slot, model) pairs."""
        if self.input_classes is not None:
            audio, n = self._packed_audio(audio, stream_ids)
            spc = 0
        else:
            audio = self._host_audio(audio)
            n, two, spc = audio.shape
            assert two == 2
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        if ids is not None:
            assert ids.shape == (n,)
        need = n * self.group_wire_floats()
        if out is None:
            out = np.empty(max(need, 1), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= need
        rc = self.lib.vapx_step_group(self._h, n, _np_ptr(ids), _np_ptr(audio), spc, _np_ptr(out), 0, None)
        if not (rc == E_NUMERIC and on_numeric == "status"):
            self._check(rc, "vapx_step_group")
        return out.reshape(-1)[:need]

    def step_group_device(self, n: int, audio_ptr: int, spc: int, wire_ptr: int, ids_ptr: int = 0, stream: int = 0):
        """Device path of ``vapx_step_group``: raw device pointers, no copy and no synchronisation; ``wire_ptr`` receives the block."""
        flags = AUDIO_DEVICE | OUT_DEVICE | (IDS_DEVICE if ids_ptr else 0)
        self._check(self.lib.vapx_step_group(self._h, n, ids_ptr or None, audio_ptr, spc, wire_ptr, flags, stream or None), "vapx_step_group")

    def group_bad(self) -> list:
        """(batch slot, model index) pairs of the latest host-path ``step_group`` whose results were not finite."""
        n = self.lib.vapx_group_bad(self._h, None, None, 0)
        if n <= 0:
            return []
        slots, models = np.empty(n, np.int32), np.empty(n, np.int32)
        self.lib.vapx_group_bad(self._h, _np_ptr(slots), _np_ptr(models), n)
        return list(zip(slots.tolist(), models.tolist()))

    def reset_stream(self, sid: int):
        self._check(self.lib.vapx_reset_stream(self._h, sid), "vapx_reset_stream")

    def reset_carry(self, sid: int):
        """Zero only the 320-sample carry (what a reconnect does in the reference, vap_main.py:368-369)."""
        self._check(self.lib.vapx_reset_carry(self._h, sid), "vapx_reset_carry")

    def get_state(self, sid: int):
        ring = np.zeros((2, self.T, 256), np.float32)
        lstm = np.zeros((2, 2, 256), np.float32)
        carry = np.zeros((2, 320), np.float32)
        n = C.c_int32(0)
        if getattr(self, "_leader", None) is not None:       # follower: LSTM / carry live in the leader
            lstm = carry = None
        self._check(self.lib.vapx_get_state(self._h, sid, _np_ptr(ring), C.byref(n), _np_ptr(lstm), _np_ptr(carry)), "vapx_get_state")
        return {"ring": ring, "n_frames": n.value, "lstm": lstm, "carry": carry}

    def set_state(self, sid: int, state: dict):
        """``ring`` [2,T,256] with ``n_frames``, ``lstm`` and ``carry``: a section that is missing or None is left as it is."""
        ring = None if state.get("ring") is None else np.ascontiguousarray(state["ring"], np.float32)
        lstm = None if state.get("lstm") is None else np.ascontiguousarray(state["lstm"], np.float32)
        carry = None if state.get("carry") is None else np.ascontiguousarray(state["carry"], np.float32)
        self._check(self.lib.vapx_set_state(self._h, sid, _np_ptr(ring), int(state.get("n_frames", 0)), _np_ptr(lstm), _np_ptr(carry)), "vapx_set_state")

    # -- bulk state export / import (snapshot, restore, migrate) -----------------------------------------
    def state_floats(self, cache: bool = False) -> int:
        """Floats of one state record of this engine (vapx.h, vapx_state_floats): ``state_record_floats`` for its window and role."""
        return int(self.lib.vapx_state_floats(self._h, STATE_CACHE if cache else 0))

    def _state_ids(self, ids):
        if ids is None:
            ids = np.arange(self.max_streams, dtype=np.int32)
        return np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)

    def export_streams(self, ids: Optional[Sequence[int]] = None, cache: bool = False, out: Optional[np.ndarray] = None) -> np.ndarray:
        """State records of streams ``ids`` (None: every slot) as float32 [n, state_floats(cache)], in ONE stream-ordered call
        (vapx_export_streams; ``split_state`` names the fields).  ``out``: e.g. a ``pinned_empty`` block, filled by DMA directly."""
        ids = self._state_ids(ids)
        n, fl = ids.size, self.state_floats(cache)
        if out is None:
            out = np.empty((n, fl), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= n * fl
        self._check(self.lib.vapx_export_streams(self._h, n, _np_ptr(ids), _np_ptr(out), STATE_CACHE if cache else 0, None),
                    "vapx_export_streams")
        return out.reshape(-1)[:n * fl].reshape(n, fl)

    def import_streams(self, ids: Optional[Sequence[int]], records: np.ndarray, cache: Optional[bool] = None):
        """Put state records [n, floats] into streams ``ids`` (None: slots 0..n-1).  ``cache``: the records carry the layer-0 Q|K|V
        cache (None: told from their length).  Every header is validated before any stream changes (vapx_import_streams)."""
        records = np.asarray(records)
        if records.dtype != np.float32 or not records.flags.c_contiguous:
            records = np.ascontiguousarray(records, dtype=np.float32)
        if records.ndim != 2:
            raise VapxError(f"records must be [n, floats], got shape {records.shape}")
        if cache is None:
            cache = records.shape[1] == self.state_floats(True)
        if records.shape[1] != self.state_floats(cache):
            raise VapxError(f"record length {records.shape[1]} floats: this engine's records have {self.state_floats(False)} "
                            f"(without cache) or {self.state_floats(True)} (with cache)")
        n = records.shape[0]
        ids = np.arange(n, dtype=np.int32) if ids is None else self._state_ids(ids)
        if ids.size != n:
            raise VapxError(f"{ids.size} stream ids for {n} records")
        self._check(self.lib.vapx_import_streams(self._h, n, _np_ptr(ids), _np_ptr(records), STATE_CACHE if cache else 0, None),
                    "vapx_import_streams")

    def export_streams_device(self, n: int, dst_ptr: int, ids_ptr: int = 0, cache: bool = False, stream: int = 0):
        """Device twin of ``export_streams``: raw device pointers, one gather kernel enqueued on ``stream``, no synchronisation."""
        flags = OUT_DEVICE | (IDS_DEVICE if ids_ptr else 0) | (STATE_CACHE if cache else 0)
        self._check(self.lib.vapx_export_streams(self._h, n, ids_ptr or None, dst_ptr, flags, stream or None), "vapx_export_streams")

    def import_streams_device(self, n: int, src_ptr: int, ids_ptr: int = 0, cache: bool = False, stream: int = 0):
        """Device twin of ``import_streams``: the records are trusted (only n_frames is clamped), no synchronisation."""
        flags = OUT_DEVICE | (IDS_DEVICE if ids_ptr else 0) | (STATE_CACHE if cache else 0)
        self._check(self.lib.vapx_import_streams(self._h, n, ids_ptr or None, src_ptr, flags, stream or None), "vapx_import_streams")

    def profile_enable(self, classes=()):
        mask = 0
        for c in classes:
            mask |= 1 << int(c)
        self._check(self.lib.vapx_profile_enable(self._h, mask), "vapx_profile_enable")

    def profile_read(self) -> dict:
        """{class_name: (total_ms, launches)} since the last read (synchronises the device)."""
        n = len(PROF_CLASSES)
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._check(self.lib.vapx_profile_read(self._h, ms, cnt, n), "vapx_profile_read")
        return {PROF_CLASSES[i]: (ms[i], cnt[i]) for i in PROF_CLASSES if cnt[i]}

    def peek(self, name: str, shape) -> np.ndarray:
        """A scratch buffer of the latest step (vapx.h, vapx_peek): the encoder stages, ``x0``, ``o``, ``stereo0`` .. ``stereo2`` [n,2,T,256],
        ``last`` [n,2,256] (the last layer's newest row where that layer runs on the newest row alone) and, nod only, ``comb`` [n,T,256].
        After a ``prefill`` and until the next step: ``h0`` .. ``h3``, ``z``, ``e`` of its last chunk, [V, 2, ...] with entry
        v = j * n + k = frame j of the chunk, stream k of the call; everything else is refused."""
        buf = np.empty(int(np.prod(shape)), np.float32)
        got = self._check(self.lib.vapx_peek(self._h, name.encode(), _np_ptr(buf), buf.size), "vapx_peek")
        assert got == buf.size, (name, got, buf.size)
        return buf.reshape(shape)

    # -- stage-level (device pointers) -------------------------------------------------------------
    def encode_audio_device(self, n: int, frames_ptr: int, e_ptr: int, stream_ids=None, stream: int = 0):
        ids = None if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.int32)
        self._check(self.lib.vapx_encode_audio(self._h, n, _np_ptr(ids), frames_ptr, e_ptr, stream or None), "vapx_encode_audio")

    def transformer_device(self, n: int, rows: int, x_ptr: int, o_ptr: int = 0, x12_ptr: int = 0, comb_ptr: int = 0,
                           stage: int = 0, stream: int = 0):
        self._check(self.lib.vapx_transformer(self._h, n, rows, x_ptr, o_ptr or None, x12_ptr or None, comb_ptr or None,
                                              stage, stream or None), "vapx_transformer")

    def transformer_maps_device(self, n: int, rows: int, x_ptr: int, o_ptr: int = 0, x12_ptr: int = 0, comb_ptr: int = 0,
                                stage: int = 0, attn_ptr: int = 0, self_attn_ptr: int = 0, cross_attn_ptr: int = 0, stream: int = 0):
        """``transformer_device`` plus the attention weights (vapx.h, vapx_transformer_maps): ``attn`` [n,2,1,4,rows,rows],
        ``self_attn`` / ``cross_attn`` [n,2,3,4,rows,rows], device pointers, 0 = not wanted."""
        self._check(self.lib.vapx_transformer_maps(self._h, n, rows, x_ptr, o_ptr or None, x12_ptr or None, comb_ptr or None, stage,
                                                   attn_ptr or None, self_attn_ptr or None, cross_attn_ptr or None, stream or None),
                    "vapx_transformer_maps")


TRUNK_RATIOS = (1, 2, 4, 5, 10)     # leader rate / follower rate (vapx.h, vapx_attach_trunk): 50->10, 50->5, 20->10, 20->5, 10->5


def trunk_plan(modes: Sequence[str], frame_hz, context_len_sec) -> dict:
    """Per-mode geometry of a trunk group, without a device: ``frame_hz`` / ``context_len_sec`` are scalars (every model), ``{mode:
    value}`` dictionaries or sequences in ``modes`` order.  Returns ``{"leader": mode, "order": [leader, followers ...], "hz" / "ctx" /
    "hop" / "L" / "T" / "R": {mode: value}}``.  The fastest model leads (ties: the earliest in ``modes``); ``R`` is the leader's
    rate over the model's.  Raises ``VapxError`` for what ``vapx_attach_trunk`` refuses."""
    modes = list(modes)

    def per_mode(v, what):
        if isinstance(v, dict):
            if set(v) != set(modes):
                raise VapxError(f"{what} names {sorted(v)}, the group serves {modes}")
            return {m: v[m] for m in modes}
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) == 1:
                return {m: v[0] for m in modes}
            if len(v) != len(modes):
                raise VapxError(f"{what} has {len(v)} values for {len(modes)} models ({modes}): give one, or one per model in model order")
            return dict(zip(modes, v))
        return {m: v for m in modes}
    hz = {m: int(v) for m, v in per_mode(frame_hz, "frame_hz").items()}
    ctx = {m: float(v) for m, v in per_mode(context_len_sec, "context_len_sec").items()}
    for m in modes:
        if hz[m] not in (5, 10, 20, 50):
            raise VapxError(f"{m}: frame_hz must be 5, 10, 20 or 50 (got {hz[m]})")
    leader = max(modes, key=lambda m: hz[m])                 # max() keeps the first of equals
    R = {}
    for m in modes:
        if hz[leader] % hz[m]:
            raise VapxError(f"{m} at {hz[m]} Hz cannot follow {leader} at {hz[leader]} Hz: the leader's rate must be an integer "
                            f"multiple of every model's (its frames would not end on leader ticks)")
        R[m] = hz[leader] // hz[m]
    return {"leader": leader, "order": [leader] + [m for m in modes if m != leader], "hz": hz, "ctx": ctx,
            "hop": {m: 16000 // hz[m] for m in modes}, "L": {m: 16000 // hz[m] + 320 for m in modes},
            "T": {m: int(ctx[m] * hz[m]) for m in modes}, "R": R}


class TrunkGroup:
    """Several weight sets (vap / bc / nod) served from ONE pass of the CPC CNN + LSTM per tick.

    The reference runs one process per model, each re-encoding the same audio with the same ``cpc_model``
    weights (vap_main.py:199-201, vap_bc_main.py, vap_nod_main.py).  Here ``blobs`` is ``{mode: blob}``.  ``frame_hz`` and
    ``context_len_sec`` are scalars (every model, as before) or per model: ``{mode: value}`` or a sequence in ``blobs`` order — the
    reference's own deployment is vap 20 Hz / 2.5 s, bc 20 Hz / 5 s, nod 10 Hz / 10 s.  ``input_hz`` (8000 / 16000 / 32000 / 48000) is the
    sample rate of the audio and ``input_format`` ("f32" / "s16" / "mulaw" / "alaw") its sample format; both are applied to the leader, which then
    takes ``hop_in`` samples of that format per tick.  The fastest model leads (runs the encoder;
    ties: the first entry), the others follow; ``hz / hop_of / L_of / T_of / R`` hold each mode's geometry, ``R[mode]`` being the
    leader ticks per frame of that model.  Input framing (``hop``, ``L``) is the leader's.

    ``step`` returns ``{mode: out[n, OUT_STRIDE]}``.  A model with ``R > 1`` answers every R-th tick of a stream: its block still has
    n rows in the batch order, rows without a frame are zero with column OUT_STATUS = STATUS_NO_FRAME (``due`` masks them)."""

    def __init__(self, blobs: dict, frame_hz=20, context_len_sec=2.5, max_streams: int = 1,
                 max_batch: Optional[int] = None, device_id: int = 0, input_hz: int = 16000, input_format: str = "f32", input_classes=None, **engine_kw):
        self.modes = list(blobs)
        plan = trunk_plan(self.modes, frame_hz, context_len_sec)
        self.hz, self.ctx, self.hop_of, self.L_of, self.T_of, self.R = (plan[k] for k in ("hz", "ctx", "hop", "L", "T", "R"))
        self.order = plan["order"]                             # model order of vapx_step_group's wire block: leader, then followers
        self.engines = {}
        for m in self.order:                                   # engine_kw: groups / split_f16 / ... — the same for every weight set
            kw = dict(engine_kw, input_hz=input_hz, input_format=input_format, input_classes=input_classes) if m == self.order[0] else engine_kw      # the leader owns the audio
            self.engines[m] = Engine(blobs[m], self.hz[m], self.ctx[m], max_streams, max_batch, m, device_id, **kw)
        self.leader = self.engines[self.order[0]]
        for m in self.order[1:]:
            self.engines[m].attach_trunk(self.leader)
        self.hop, self.L, self.T = self.leader.hop, self.leader.L, self.leader.T
        self.input_hz, self.hop_in, self.input_format = self.leader.input_hz, self.leader.hop_in, self.leader.input_format
        self.input_classes = self.leader.input_classes     # a table: ``step`` / ``step_wire`` take per-slot arrays or a packed block, as the leader does

    def step(self, audio: np.ndarray, stream_ids: Optional[Sequence[int]] = None) -> dict:
        res = {self.order[0]: self.leader.step(audio, stream_ids)}
        for m in self.order[1:]:
            res[m] = self.engines[m].step_follow(len(res[self.order[0]]))
        return {m: res[m] for m in self.modes}

    @staticmethod
    def due(mode: str, rows: np.ndarray) -> np.ndarray:
        """Boolean mask over ``rows`` (a model's block of ``step`` or ``step_wire``): True where the row carries a frame."""
        return rows[:, OUT_STATUS] != STATUS_NO_FRAME

    def wire_floats(self, mode: str) -> int:
        return wire_floats(mode, self.T_of[mode])

    def step_wire(self, audio: np.ndarray, stream_ids: Optional[Sequence[int]] = None, out: Optional[np.ndarray] = None,
                  on_numeric: str = "raise") -> dict:
        """One ``vapx_step_group`` call for the whole group: ``{mode: wire rows [n, wire_floats(mode)]}`` (views of one block; name
        the columns with ``split_wire``).  One compact device-to-host copy and one synchronisation per tick, where ``step`` pays a
        full [n, OUT_STRIDE] copy and a synchronisation per model."""
        n = len(stream_ids) if stream_ids is not None else len(audio)
        block = self.leader.step_group(audio, stream_ids, out, on_numeric)
        res, at = {}, 0
        for m in self.order:
            wf = self.wire_floats(m)
            res[m] = block[at:at + n * wf].reshape(n, wf)
            at += n * wf
        return {m: res[m] for m in self.modes}

    def step_device(self, n: int, audio_ptr: int, spc: int, out_ptrs: dict, ids_ptr: int = 0, stream: int = 0):
        self.leader.step_device(n, audio_ptr, spc, out_ptrs[self.order[0]], ids_ptr, stream)
        for m in self.order[1:]:
            self.engines[m].step_follow_device(n, out_ptrs[m], stream)

    def reset_stream(self, sid: int):
        self.leader.reset_stream(sid)                      # cascades to the followers

    def export_streams(self, ids: Optional[Sequence[int]] = None, cache: bool = False) -> dict:
        """``{mode: records}``: the leader's records carry LSTM + carry, a follower's only its ring (+ cache).  A group with a
        follower slower than its leader raises the engine's refusal (its records do not carry the half-collected frame yet)."""
        return {m: self.engines[m].export_streams(ids, cache) for m in sorted(self.modes, key=lambda m: -self.R[m])}

    def import_streams(self, ids: Optional[Sequence[int]], records: dict, cache: Optional[bool] = None):
        """Inverse of ``export_streams``; ``records`` must name exactly this group's modes."""
        if set(records) != set(self.modes):
            raise VapxError(f"records for modes {sorted(records)}, this group serves {self.modes}")
        for m in sorted(self.modes, key=lambda m: -self.R[m]):     # a refusing (slower) model first: no stream is touched
            self.engines[m].import_streams(ids, records[m], cache)

    def close(self):
        for m in reversed(self.order):                     # followers before their leader
            self.engines[m].close()


def gemm_tile_rows(M: int, N: int, K: int, epi: int) -> int:
    """Rows per workgroup the library's GEMM dispatch picks for this shape and epilogue (vapx.h, vapx_gemm_tile_rows)."""
    return int(load_library().vapx_gemm_tile_rows(int(M), int(N), int(K), int(epi)))


def prefill_chunks(max_batch: int, n: int, frames: int, ctx_frames: int) -> list:
    """The plan of one ``vapx_prefill`` call, as the engine walks it (csrc/engine_buffers.h prefill_chunk_frames): a list of
    (first frame, frames in the chunk, fills the ring).  A chunk holds floor(max_batch / n) frames, at least one; a chunk all of whose
    frames a later frame of the call overwrites (frames > ctx_frames) runs the encoder alone."""
    if not 1 <= n <= max_batch or frames < 1 or ctx_frames < 1:
        raise ValueError("prefill_chunks: 1 <= n <= max_batch, frames >= 1 and ctx_frames >= 1 are needed")
    fc = max(1, max_batch // n)
    return [(f0, min(fc, frames - f0), f0 + min(fc, frames - f0) + ctx_frames > frames) for f0 in range(0, frames, fc)]


def split_outputs(out: np.ndarray) -> dict:
    """Name the columns of a vapx_step output block."""
    return {
        "p_now": out[:, OUT_P_NOW:OUT_P_NOW + 2], "p_future": out[:, OUT_P_FUTURE:OUT_P_FUTURE + 2],
        "vad": out[:, OUT_VAD:OUT_VAD + 2], "aux": out[:, OUT_AUX:OUT_AUX + 4],
        "n": out[:, OUT_NVALID].astype(np.int32), "logits": out[:, OUT_LOGITS:OUT_LOGITS + 256],
        "vad_logit": out[:, OUT_VAD_LOGIT:OUT_VAD_LOGIT + 2],
        "status": out[:, OUT_STATUS].astype(np.int32),
        "e": out[:, OUT_E:OUT_E + 512].reshape(-1, 2, 256),
    }


def state_record_floats(ctx_frames: int, cache: bool = False, follower: bool = False, input_hz: int = 16000) -> int:
    """Length of a state record (the layout in vapx.h): header, LSTM + carry unless ``follower``, the resampler history of a leader /
    stand-alone engine with an input rate, ring, optional Q|K|V cache."""
    from .resample import history_floats
    T = int(ctx_frames)
    return (STATE_HEADER_FLOATS + (0 if follower else STATE_LSTM_FLOATS + STATE_CARRY_FLOATS + history_floats(input_hz)) + 2 * T * 256
            + (2 * T * 768 if cache else 0))


def split_state(records: np.ndarray, T: int, follower: bool = False, input_hz: int = 16000) -> dict:
    """Name the fields of state records [n, floats] (views, as ``split_outputs`` does for output rows): the header words
    ``magic`` / ``ctx_frames`` / ``frame_hz`` / ``bits`` / ``n_frames`` / ``mode``, ``lstm`` [n,2,2,256] and ``carry`` [n,2,320] (None
    for a follower's records), ``ring`` [n,2,T,256] oldest -> newest (zero beyond ``n_frames``) and ``cache`` [n,2,T,768] or None.  Records
    of an engine with ``input_hz`` other than 16000 also give ``input_hz`` (header word [6]), ``resample_started`` (word [7]) and
    ``resample_hist`` [n,2,H]; for the others the three are 0 / 0 / None."""
    from .resample import geometry, history_floats
    records = np.asarray(records)
    n, fl = records.shape
    cache = fl == state_record_floats(T, True, follower, input_hz)
    if fl != state_record_floats(T, cache, follower, input_hz):
        raise VapxError(f"record length {fl} fits no layout of a {'follower' if follower else 'leader / stand-alone'} engine with T={T}")
    hdr = records[:, :STATE_HEADER_FLOATS].view(np.int32)
    d = {"magic": hdr[:, 0], "ctx_frames": hdr[:, 1], "frame_hz": hdr[:, 2], "bits": hdr[:, 3], "n_frames": hdr[:, 4], "mode": hdr[:, 5],
         "lstm": None, "carry": None, "cache": None, "input_hz": hdr[:, 6], "resample_started": hdr[:, 7], "resample_hist": None}
    at = STATE_HEADER_FLOATS
    if not follower:
        d["lstm"] = records[:, at:at + STATE_LSTM_FLOATS].reshape(n, 2, 2, 256)
        at += STATE_LSTM_FLOATS
        d["carry"] = records[:, at:at + STATE_CARRY_FLOATS].reshape(n, 2, 320)
        at += STATE_CARRY_FLOATS
        if history_floats(input_hz):
            H = geometry(input_hz)["H"]
            d["resample_hist"] = records[:, at:at + 2 * H].reshape(n, 2, H)
            at += history_floats(input_hz)
    d["ring"] = records[:, at:at + 2 * T * 256].reshape(n, 2, T, 256)
    at += 2 * T * 256
    if cache:
        d["cache"] = records[:, at:at + 2 * T * 768].reshape(n, 2, T, 768)
    return d


def wire_floats(mode: str, ctx_frames: int) -> int:
    """Length of a model's wire row (vapx.h, vapx_wire_floats): 16, or for nod 16 + ctx_frames rounded up to a multiple of 4."""
    got = int(load_library().vapx_wire_floats(MODE[mode], int(ctx_frames)))
    if got <= 0:
        raise VapxError(f"vapx_wire_floats({mode}, {ctx_frames}): bad mode or window")
    return got


def split_wire(mode: str, rows: np.ndarray) -> dict:
    """Name the columns of wire rows [n, wire_floats] (``TrunkGroup.step_wire``): the head of ``split_outputs``' columns; for nod,
    ``p_bc_rows`` [n, ctx_frames] is p_bc of every window row (valid up to each row's ``n``, vap_nod_main.py:276)."""
    d = {
        "p_now": rows[:, OUT_P_NOW:OUT_P_NOW + 2], "p_future": rows[:, OUT_P_FUTURE:OUT_P_FUTURE + 2],
        "vad": rows[:, OUT_VAD:OUT_VAD + 2], "aux": rows[:, OUT_AUX:OUT_AUX + 4],
        "n": rows[:, OUT_NVALID].astype(np.int32), "vad_logit": rows[:, OUT_VAD_LOGIT:OUT_VAD_LOGIT + 2],
        "status": rows[:, OUT_STATUS].astype(np.int32),
    }
    if mode == "nod":
        d["p_bc_rows"] = rows[:, OUT_LOGITS:]
    return d
