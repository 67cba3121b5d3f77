"""ctypes binding of libvapx's native many-stream TCP front-end (include/vapx.h, ``vapx_ingest_*``).

Stands in for the reference's server threads (``proc_serv_in`` / ``proc_serv_out`` / ``proc_serv_out_dist``,
rvap/vap_main/vap_main.py:338-457) for thousands of dialogues per process: epoll receive threads decode the 2560-byte
packets straight into page-locked staging, a tick thread steps the ready streams, sender threads write result packets
byte-identical to ``rvap/common/util.py``'s.  ``server.ManyStreamServer`` is the readable Python twin of the same
behaviour (one thread, ~2 k real-time streams); this one carries a whole GPU.

``NativeServer(engine)`` serves an ``engine.Engine``; ``NativeServer.over_function(step, ...)`` runs the same front-end
over a Python step function (host-logic tests without a GPU).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import numpy as np

from . import engine as _engine

MODE = _engine.MODE


_CONFIG_FIELDS = [("struct_size", C.c_int32), ("port_in", C.c_int32), ("port_out", C.c_int32), ("rx_threads", C.c_int32),
                  ("tx_threads", C.c_int32), ("max_wait_us", C.c_int32), ("min_batch", C.c_int32), ("reset_on_connect", C.c_int32),
                  ("broadcast", C.c_int32), ("bind_any", C.c_int32), ("gain", C.c_double), ("target_util_pct", C.c_int32),
                  ("flags", C.c_int32), ("cpu_first", C.c_int32), ("cpu_count", C.c_int32), ("input_format", C.c_int32)]


class _IngestConfigNoClasses(C.Structure):
    """vapx_ingest_config as it was before the input classes (it ended with input_format): the library still takes it, as "no classes"."""
    _fields_ = _CONFIG_FIELDS


class _IngestConfig(C.Structure):
    _fields_ = _CONFIG_FIELDS + [("n_input_classes", C.c_int32), ("input_classes", _engine._InputClass * _engine.MAX_INPUT_CLASSES),
                                 ("class_ports_in", C.c_int32 * _engine.MAX_INPUT_CLASSES)]


MAX_PAIR_PORTS = 16


class _PairPort(C.Structure):
    _fields_ = [("cls_ch1", C.c_int32), ("cls_ch2", C.c_int32), ("port_in", C.c_int32)]


class _IngestConfigPairs(C.Structure):
    """vapx_ingest_config with the pair ports at its end; ``_IngestConfig`` keeps the size it had before them, which still means "none"."""
    _fields_ = _IngestConfig._fields_ + [("n_pair_ports", C.c_int32), ("pair_ports", _PairPort * MAX_PAIR_PORTS)]


def class_table(classes) -> list:
    """An input-class table for a front-end: ``engine.input_class_table`` with the wire's name "f64" (the reference's framing: f64 pairs,
    cast to the engine's f32 on the host) accepted for "f32"."""
    return _engine.input_class_table([("f32" if f == "f64" else f, hz) for f, hz in classes])


def parse_input_class(text: str):
    """``FORMAT@RATE[:PORT]`` (``serve --input_class``, the load tools) -> ((engine format name, rate), port or 0)."""
    spec, _, port = text.partition(":")
    fmt, at, rate = spec.partition("@")
    if not at or not rate.isdigit() or (port and not port.isdigit()):
        raise ValueError(f"input class {text!r}: expected FORMAT@RATE[:PORT], e.g. mulaw@8000:50017")
    return class_table([(fmt, int(rate))])[0], int(port or 0)


def parse_input_port(text: str):
    """``FORMAT@RATE[:PORT]`` or ``FORMAT@RATE+FORMAT@RATE[:PORT]`` (a pair port: channel 1's class, then channel 2's) ->
    ([class] or [class of channel 1, class of channel 2], port or 0)."""
    spec, _, port = text.partition(":")
    legs = spec.split("+")
    if len(legs) == 1:
        c, p = parse_input_class(text)
        return [c], p
    if len(legs) != 2 or (port and not port.isdigit()):
        raise ValueError(f"input class {text!r}: expected FORMAT@RATE[:PORT] or FORMAT@RATE+FORMAT@RATE[:PORT], e.g. s16@48000+mulaw@8000:50027")
    return [parse_input_class(leg)[0] for leg in legs], int(port or 0)


def input_ports(specs):
    """The ``--input_class`` arguments of a server -> (table, class_ports, pair_ports): the table is the distinct classes named anywhere, in
    order of first appearance; ``class_ports[c]`` is the port of class c's own port (0 = ephemeral: also for a class that only pair ports
    name); ``pair_ports`` is ``[(c1, c2, port)]`` with indices into the table.  A class or a pair named twice is refused."""
    table, class_ports, pair_ports, seen = [], [], [], set()
    for text in specs:
        legs, port = parse_input_port(text)
        if tuple(legs) in seen:
            raise ValueError(f"two equal input classes: {text.partition(':')[0]!r} is named twice")
        seen.add(tuple(legs))
        for c in legs:
            if c not in table:
                table.append(c)
                class_ports.append(0)
        if len(legs) == 1:
            class_ports[table.index(legs[0])] = port
        else:
            pair_ports.append((table.index(legs[0]), table.index(legs[1]), port))
    class_table(table)      # at most 16
    if len(pair_ports) > MAX_PAIR_PORTS:
        raise ValueError(f"{len(pair_ports)} pair ports: at most {MAX_PAIR_PORTS}")
    return table, class_ports, pair_ports


WIRE_FORMATS = {"f64": 0, "s16": 1, "mulaw": 2, "alaw": 3}      # wire format of the input port; f64 = the reference's framing (engine format f32)


def wire_format_id(fmt) -> int:
    """Name or id of an input-port wire format -> the id of vapx_ingest_config.input_format; None -> 0 (the engine's own)."""
    if fmt is None:
        return 0
    if isinstance(fmt, str):
        if fmt not in WIRE_FORMATS:
            raise ValueError(f"unknown input format {fmt!r}: one of {', '.join(WIRE_FORMATS)}")
        return WIRE_FORMATS[fmt]
    return int(fmt)


def _raw_view(audio_ptr, n: int, hop: int, fmt_id: int) -> np.ndarray:
    """The audio block a step function receives, [n, 2, hop]: float32, or the raw samples of the wire format (int16 / uint8)."""
    dt = {0: np.float32, 1: np.int16, 2: np.uint8, 3: np.uint8}[fmt_id]
    nbytes = n * 2 * hop * np.dtype(dt).itemsize
    buf = (C.c_char * nbytes).from_address(C.addressof(audio_ptr.contents))
    return np.frombuffer(buf, dtype=dt).reshape(n, 2, hop)


class _IngestStats(C.Structure):
    _fields_ = [("frames_done", C.c_int64), ("ticks", C.c_int64), ("rx_bytes", C.c_int64), ("tx_bytes", C.c_int64),
                ("in_connections", C.c_int64), ("out_connections", C.c_int64), ("dropped_listeners", C.c_int64),
                ("numeric_resets", C.c_int64), ("overruns", C.c_int64), ("mean_batch", C.c_double), ("lat_mean_ms", C.c_double),
                ("lat_p50_ms", C.c_double), ("lat_p99_ms", C.c_double), ("lat_max_ms", C.c_double), ("step_mean_ms", C.c_double)]


_STEP_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float))
_RESET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int32)


class NativeServer:
    def __init__(self, eng: "_engine.Engine", port_in: int = 50007, port_out: int = 50008, gain: float = 1.0, max_wait_s: float = 0.002,
                 min_batch: int = 0, reset_on_connect: bool = True, broadcast: Optional[bool] = None, rx_threads: int = 0,
                 tx_threads: int = 0, bind_any: bool = False, target_util: float = 0.9, cores: Optional[tuple] = None,
                 keep_nofile: bool = False, core_set: bool = False, keep_state: bool = False, input_format: Optional[str] = None,
                 class_ports=None, pair_ports=None):
        """``class_ports``: with an engine that has input classes (``Engine(input_classes=...)``) the input port of every class, in table
        order (default: all ephemeral; ``.class_ports`` lists the bound ones); ``port_in`` is then ignored.
        ``pair_ports``: ``[(c1, c2, port)]``, input ports for dialogues whose channel 1 is of class c1 and channel 2 of class c2; they take
        planar 10 ms packets (``wire.encode_input_planar``; ``.pair_ports`` lists the bound ports).
        ``input_format``: wire format of the input port, "f64" (the reference's framing) / "s16" / "mulaw" / "alaw"; it is the engine's
        (``Engine(input_format=...)``, "f32" there is "f64" here) and may be left out; one that disagrees with the engine's is refused.
        ``cores`` = (first, count): pin the front-end's tick / receive / sender threads to that core range (the GPU's NUMA node; keep
        load generators and other tenants off it), one core each — or, with ``core_set``, all of them to the range as one affinity set.  ``keep_nofile``: never raise the process's RLIMIT_NOFILE (include/vapx.h).
        ``keep_state``: the engine holds imported stream state — skip the warm-up steps and resets of the open (VAPX_INGEST_KEEP_STATE);
        pass ``reset_on_connect=False`` with it."""
        self.lib = _engine.load_library()
        self._keep = [eng]
        self._check_format(getattr(eng, "input_format", "f32"), input_format)
        cfg = self._cfg(port_in, port_out, gain, max_wait_s, min_batch, reset_on_connect, broadcast, rx_threads, tx_threads, bind_any, target_util,
                        cores, keep_nofile, core_set, keep_state, input_format, getattr(eng, "input_classes", None), class_ports, pair_ports)
        h = C.c_void_p()
        rc = self.lib.vapx_ingest_open(eng._h, C.byref(cfg), C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_open failed ({rc}): {self.lib.vapx_ingest_last_open_error().decode()}")
        self._h = h
        self._ports()

    @staticmethod
    def _check_format(engine_format: str, input_format):
        """"f64" asked of an engine with a raw format cannot be told to the library (0 there means "the engine's"): refuse it here."""
        if input_format is not None and wire_format_id(input_format) != wire_format_id("f64" if engine_format == "f32" else engine_format):
            raise _engine.VapxError(f"input_format {input_format!r} differs from the engine's input format {engine_format!r}")

    @staticmethod
    def _cfg(port_in, port_out, gain, max_wait_s, min_batch, reset_on_connect, broadcast, rx_threads, tx_threads, bind_any, target_util=0.9,
             cores=None, keep_nofile=False, core_set=False, keep_state=False, input_format=None, input_classes=None, class_ports=None,
             pair_ports=None):
        first, count = (int(cores[0]), int(cores[1])) if cores else (0, 0)
        struct = _IngestConfigPairs if pair_ports else _IngestConfig
        cfg = struct(C.sizeof(struct), port_in, port_out, rx_threads, tx_threads, int(max_wait_s * 1e6), min_batch,
                            1 if reset_on_connect else 0, -1 if broadcast is None else int(bool(broadcast)), int(bool(bind_any)), gain,
                            int(round(target_util * 100)), (1 if keep_nofile else 0) | (2 if core_set else 0) | (4 if keep_state else 0), first, count,
                            wire_format_id(input_format))
        if input_classes:
            from . import pcm
            tab = class_table(input_classes)
            ports = list(class_ports) if class_ports is not None else [0] * len(tab)
            if len(ports) != len(tab):
                raise ValueError(f"{len(tab)} input classes need {len(tab)} input ports, got {len(ports)}")
            cfg.n_input_classes = len(tab)
            for i, ((f, hz), port) in enumerate(zip(tab, ports)):
                cfg.input_classes[i] = _engine._InputClass(hz, pcm.FORMATS[f])
                cfg.class_ports_in[i] = int(port)
        elif class_ports:
            raise ValueError("class_ports without input classes")
        if pair_ports:
            if len(pair_ports) > MAX_PAIR_PORTS:
                raise ValueError(f"{len(pair_ports)} pair ports: at most {MAX_PAIR_PORTS}")
            cfg.n_pair_ports = len(pair_ports)
            for i, (c1, c2, port) in enumerate(pair_ports):
                cfg.pair_ports[i] = _PairPort(int(c1), int(c2), int(port))
        return cfg

    @classmethod
    def over_function(cls, step: Callable, n_streams: int, frame_hz: int = 20, mode: str = "vap", max_batch: Optional[int] = None,
                      reset: Optional[Callable] = None, port_in: int = 0, port_out: int = 0, gain: float = 1.0, max_wait_s: float = 0.002,
                      min_batch: int = 0, reset_on_connect: bool = True, broadcast: Optional[bool] = None, rx_threads: int = 0,
                      tx_threads: int = 0, target_util: float = 1.0, input_format: Optional[str] = None, input_classes=None,
                      class_ports=None, pair_ports=None):
        """``step(ids int32[n], audio float32[n,2,hop], out float32[n,OUT_STRIDE]) -> int`` fills ``out`` in place;
        ``reset(stream_id)`` gets negative ids (``-(id+1)``) for carry-only resets.  With ``input_format`` "s16" / "mulaw" / "alaw" the
        input port takes packets of that format and ``audio`` is the de-interleaved raw block, int16 or uint8 [n,2,hop].
        With ``input_classes`` (and ``class_ports``, default ephemeral) there is one input port per class and ``audio`` is the packed block
        exactly as an engine with that table takes it, a uint8 array: slot k holds [2, hop_in] samples of the class
        ``self.stream_class(ids[k])`` (valid inside ``step``), the slots back to back in batch order.  With ``pair_ports`` a slot holds
        channel 1's row and then channel 2's, in the classes ``self.stream_channel_classes(ids[k])``."""
        self = cls.__new__(cls)
        self.lib = _engine.load_library()
        hop = 16000 // frame_hz
        fmt_id = wire_format_id(input_format)
        tab = class_table(input_classes) if input_classes else None

        def _step(_user, n, ids, audio, out):
            try:
                i = np.ctypeslib.as_array(ids, shape=(n,))
                if tab:
                    nbytes = sum(_engine.input_row_bytes(tab[c], frame_hz) for s in i for c in self.stream_channel_classes(int(s)))
                    a = np.frombuffer((C.c_char * nbytes).from_address(C.addressof(audio.contents)), dtype=np.uint8)
                else:
                    a = _raw_view(audio, n, hop, fmt_id)
                o = np.ctypeslib.as_array(out, shape=(n, _engine.OUT_STRIDE))
                o[:, _engine.OUT_STATUS] = 0.0
                return int(step(i, a, o) or 0)
            except Exception:          # noqa: BLE001 — never unwind through the C caller
                import traceback
                traceback.print_exc()
                return -1

        def _reset(_user, sid):
            if reset is not None:
                reset(int(sid))

        self._keep = [_STEP_FN(_step), _RESET_FN(_reset)]
        cfg = cls._cfg(port_in, port_out, gain, max_wait_s, min_batch, reset_on_connect, broadcast, rx_threads, tx_threads, False, target_util,
                       input_format=fmt_id, input_classes=tab, class_ports=class_ports, pair_ports=pair_ports)
        h = C.c_void_p()
        rc = self.lib.vapx_ingest_open_fn(C.cast(self._keep[0], C.c_void_p), C.cast(self._keep[1], C.c_void_p), None, n_streams,
                                          max_batch or n_streams, frame_hz, MODE[mode], C.byref(cfg), C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_open_fn failed ({rc}): {self.lib.vapx_ingest_last_open_error().decode()}")
        self._h = h
        self._ports()
        return self

    @classmethod
    def for_group(cls, trunk_group: "_engine.TrunkGroup", port_in: int = 50007, ports_out=None, gain: float = 1.0, max_wait_s: float = 0.002,
                  min_batch: int = 0, reset_on_connect: bool = True, broadcast: Optional[bool] = None, rx_threads: int = 0,
                  tx_threads: int = 0, bind_any: bool = False, target_util: float = 0.9, cores: Optional[tuple] = None,
                  keep_nofile: bool = False, core_set: bool = False, keep_state: bool = False, input_format: Optional[str] = None):
        """One front-end for a whole ``engine.TrunkGroup`` (``vapx_ingest_open_group``): one input port, the audio encoded once, one
        output port per model in ``trunk_group.modes`` order (``ports_out``: one per model, default 50008, 50009, ...; 0 = ephemeral),
        each with its model's reference framing.  ``.ports_out`` is the bound ``{mode: port}``.  In a mixed group (models with rates
        of their own) input framing and ticks are the leader's; a model at 1/R of its rate sends one packet per R leader hops of a
        dialogue, echoing all R hops (vapx.h, vapx_ingest_open_group)."""
        self = cls.__new__(cls)
        self.lib = _engine.load_library()
        ports = list(ports_out) if ports_out is not None else [50008 + i for i in range(len(trunk_group.modes))]
        if len(ports) != len(trunk_group.modes):
            raise ValueError(f"{len(trunk_group.modes)} models need {len(trunk_group.modes)} output ports, got {len(ports)}")
        by_mode = dict(zip(trunk_group.modes, ports))
        modes = list(trunk_group.order)                        # the engine's model order: the leader (fastest model) first
        ports = [by_mode[m] for m in modes]
        self._keep = [trunk_group]
        cls._check_format(getattr(trunk_group, "input_format", "f32"), input_format)               # the leader's (``TrunkGroup(input_format=...)``)
        cfg = cls._cfg(port_in, ports[0], gain, max_wait_s, min_batch, reset_on_connect, broadcast, rx_threads, tx_threads, bind_any, target_util,
                       cores, keep_nofile, core_set, keep_state, input_format)
        fol = (C.c_void_p * max(len(modes) - 1, 1))(*[trunk_group.engines[m]._h.value for m in modes[1:]])
        fports = (C.c_int32 * max(len(modes) - 1, 1))(*ports[1:])
        h = C.c_void_p()
        rc = self.lib.vapx_ingest_open_group(trunk_group.leader._h, fol, len(modes) - 1, C.byref(cfg), fports, C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_open_group failed ({rc}): {self.lib.vapx_ingest_last_open_error().decode()}")
        self._h = h
        self._group_ports(modes)
        return self

    @classmethod
    def over_group_function(cls, step: Callable, modes, n_streams: int, frame_hz=20, ctx_frames=50,
                            max_batch: Optional[int] = None, reset: Optional[Callable] = None, port_in: int = 0, ports_out=None,
                            gain: float = 1.0, max_wait_s: float = 0.002, min_batch: int = 0, reset_on_connect: bool = True,
                            broadcast: Optional[bool] = None, rx_threads: int = 0, tx_threads: int = 0, target_util: float = 1.0,
                            input_format: Optional[str] = None):
        """The group front-end over a Python step function (``vapx_ingest_open_group_fn``; host-logic tests without a GPU):
        ``step(ids int32[n], audio float32[n,2,hop], wire {mode: float32[n, wire_floats]}) -> int`` fills the views of that tick's wire
        block in place (status columns start at 0); ``reset`` as in ``over_function``.  ``frame_hz`` / ``ctx_frames`` may be sequences,
        one value per model (``vapx_ingest_open_group_fn2``): ``modes[0]`` leads, ``hop`` is its hop, and the step function marks a
        slower model's rows without a frame with ``engine.STATUS_NO_FRAME``."""
        self = cls.__new__(cls)
        self.lib = _engine.load_library()
        modes = list(modes)
        mixed = not (np.isscalar(frame_hz) and np.isscalar(ctx_frames))
        hzs = [int(frame_hz)] * len(modes) if np.isscalar(frame_hz) else [int(v) for v in frame_hz]
        ctxs = [int(ctx_frames)] * len(modes) if np.isscalar(ctx_frames) else [int(v) for v in ctx_frames]
        if len(hzs) != len(modes) or len(ctxs) != len(modes):
            raise ValueError(f"{len(modes)} models need {len(modes)} rates and windows")
        frame_hz = hzs[0]
        hop = 16000 // frame_hz
        fmt_id = wire_format_id(input_format)                  # a raw format: ``audio`` is the raw block, as in ``over_function``
        wf = [int(self.lib.vapx_wire_floats(MODE[m], c)) for m, c in zip(modes, ctxs)]
        ports = list(ports_out) if ports_out is not None else [0] * len(modes)
        if len(ports) != len(modes):
            raise ValueError(f"{len(modes)} models need {len(modes)} output ports, got {len(ports)}")

        def _step(_user, n, ids, audio, out):
            try:
                i = np.ctypeslib.as_array(ids, shape=(n,))
                a = _raw_view(audio, n, hop, fmt_id)
                block = np.ctypeslib.as_array(out, shape=(n * sum(wf),))
                wire, at = {}, 0
                for m, w in zip(modes, wf):
                    wire[m] = block[at:at + n * w].reshape(n, w)
                    wire[m][:, _engine.OUT_STATUS] = 0.0
                    at += n * w
                return int(step(i, a, wire) or 0)
            except Exception:          # noqa: BLE001 — never unwind through the C caller
                import traceback
                traceback.print_exc()
                return -1

        def _reset(_user, sid):
            if reset is not None:
                reset(int(sid))

        self._keep = [_STEP_FN(_step), _RESET_FN(_reset)]
        cfg = cls._cfg(port_in, ports[0], gain, max_wait_s, min_batch, reset_on_connect, broadcast, rx_threads, tx_threads, False, target_util,
                       input_format=fmt_id)
        marr = (C.c_int32 * len(modes))(*[MODE[m] for m in modes])
        fports = (C.c_int32 * max(len(modes) - 1, 1))(*ports[1:])
        h = C.c_void_p()
        if mixed:
            harr, carr = (C.c_int32 * len(modes))(*hzs), (C.c_int32 * len(modes))(*ctxs)
            rc = self.lib.vapx_ingest_open_group_fn2(C.cast(self._keep[0], C.c_void_p), C.cast(self._keep[1], C.c_void_p), None, n_streams,
                                                     max_batch or n_streams, harr, carr, marr, len(modes), C.byref(cfg), fports, C.byref(h))
        else:
            rc = self.lib.vapx_ingest_open_group_fn(C.cast(self._keep[0], C.c_void_p), C.cast(self._keep[1], C.c_void_p), None, n_streams,
                                                    max_batch or n_streams, frame_hz, ctxs[0], marr, len(modes), C.byref(cfg), fports,
                                                    C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_open_group_fn failed ({rc}): {self.lib.vapx_ingest_last_open_error().decode()}")
        self._h = h
        self._group_ports(modes)
        return self

    def _group_ports(self, modes):
        a = C.c_int32(0)
        arr = (C.c_int32 * len(modes))()
        self.lib.vapx_ingest_group_ports(self._h, C.byref(a), arr, len(modes))
        self.port_in, self.port_out = a.value, arr[0]
        self.ports_out = {m: int(arr[i]) for i, m in enumerate(modes)}

    @classmethod
    def over_native_function(cls, step_ptr: int, user_ptr: int, n_streams: int, frame_hz: int = 20, mode: str = "vap", max_batch: Optional[int] = None,
                             keep=(), port_in: int = 0, port_out: int = 0, gain: float = 1.0, max_wait_s: float = 0.002, min_batch: int = 0,
                             rx_threads: int = 0, tx_threads: int = 0, target_util: float = 0.9, cores: Optional[tuple] = None,
                             input_format: Optional[str] = None):
        """The same front-end over a C step function (address of a ``vapx_ingest_step_fn``, ``user_ptr`` handed to it): no Python on the tick
        thread.  ``tools/server_load.py --standin`` puts a stand-in for the GPU engine here (tools/standin_step.cpp) to load-test the host side of
        N x 4096 dialogues; ``port_in = port_out = -1`` makes it a passive shard of a ``FrontDoor``.  ``keep``: objects that must outlive it."""
        self = cls.__new__(cls)
        self.lib = _engine.load_library()
        self._keep = list(keep)
        cfg = cls._cfg(port_in, port_out, gain, max_wait_s, min_batch, True, None, rx_threads, tx_threads, False, target_util, cores,
                       input_format=input_format)
        h = C.c_void_p()
        rc = self.lib.vapx_ingest_open_fn(C.c_void_p(step_ptr), None, C.c_void_p(user_ptr), n_streams, max_batch or n_streams, frame_hz, MODE[mode],
                                          C.byref(cfg), C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_open_fn failed ({rc}): {self.lib.vapx_ingest_last_open_error().decode()}")
        self._h = h
        self._ports()
        return self

    def attach_link(self, link_fd: int):
        """Make this PASSIVE front-end a shard of a front door in another process (``RemoteFrontDoor``): ``link_fd`` is this process's end of an
        ``AF_UNIX / SOCK_SEQPACKET`` socket pair; accepted connections arrive over it as descriptors (include/vapx.h)."""
        rc = self.lib.vapx_ingest_attach_link(self._h, int(link_fd))
        if rc != 0:
            raise _engine.VapxError(f"vapx_ingest_attach_link failed ({rc}): the front-end must be passive (port_in = port_out = -1) and not linked yet")

    def _ports(self):
        a, b = C.c_int32(0), C.c_int32(0)
        self.lib.vapx_ingest_ports(self._h, C.byref(a), C.byref(b))
        self.port_in, self.port_out = a.value, b.value
        arr = (C.c_int32 * _engine.MAX_INPUT_CLASSES)()
        n = self.lib.vapx_ingest_class_ports(self._h, arr, _engine.MAX_INPUT_CLASSES)
        self.class_ports = [int(arr[c]) for c in range(max(n, 0))]      # the bound input port of every input class; [] without a table
        arr = (C.c_int32 * MAX_PAIR_PORTS)()
        n = self.lib.vapx_ingest_pair_ports(self._h, arr, MAX_PAIR_PORTS)
        self.pair_ports = [int(arr[p]) for p in range(max(n, 0))]       # the bound input port of every pair port

    def stream_class(self, sid: int) -> int:
        """The input class of stream ``sid`` as the tick thread knows it: for a step function of ``over_function(input_classes=...)``."""
        c = self.lib.vapx_ingest_stream_class(self._h, int(sid))
        if c < 0:
            raise _engine.VapxError(f"vapx_ingest_stream_class failed ({c}): no input classes, a bad stream id, or a stream whose channels differ")
        return c

    def stream_channel_classes(self, sid: int) -> tuple:
        """The input classes of the two channels of stream ``sid`` as the tick thread knows them (a pair port's stream has two)."""
        out = (C.c_int32 * 2)()
        rc = self.lib.vapx_ingest_stream_channel_classes(self._h, int(sid), out)
        if rc < 0:
            raise _engine.VapxError(f"vapx_ingest_stream_channel_classes failed ({rc}): no input classes, or a bad stream id")
        return int(out[0]), int(out[1])

    def stats(self, reset_latency_window: bool = False) -> dict:
        """Counters + the latency window (frame complete on the host -> packet handed to the kernel); ``late_over_10ms`` / ``answered`` are the
        exact counts of the window (read BEFORE an optional reset of the window)."""
        late, ans = C.c_int64(0), C.c_int64(0)
        self.lib.vapx_ingest_late_read(self._h, C.byref(late), C.byref(ans))
        st = _IngestStats()
        self.lib.vapx_ingest_stats_read(self._h, C.byref(st), 1 if reset_latency_window else 0)
        d = {k: getattr(st, k) for k, _ in _IngestStats._fields_}
        d["late_over_10ms"], d["answered"] = late.value, ans.value
        return d

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vapx_ingest_close(self._h)
            self._h = None
            for e in self._keep:                               # an engine with input classes: the front-end moved its streams between classes
                if getattr(e, "input_classes", None) and hasattr(e, "refresh_stream_classes") and getattr(e, "_h", None):
                    e.refresh_stream_classes()

    stop = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_input(data: bytes, gain: float = 1.0):
    """Native twin of ``wire.decode_input`` (== util.conv_bytearray_2_2floatarray): bytes -> (x1 f64, x2 f64, x1 f32, x2 f32)."""
    lib = _engine.load_library()
    if len(data) % 16:
        raise ValueError("input packet length must be a multiple of 16 bytes")
    n = len(data) // 16
    buf = np.frombuffer(data, dtype=np.uint8)
    x1, x2 = np.empty(n, np.float64), np.empty(n, np.float64)
    f1, f2 = np.empty(n, np.float32), np.empty(n, np.float32)
    got = lib.vapx_wire_decode_input(buf.ctypes.data_as(C.c_void_p), len(data), gain, f1.ctypes.data_as(C.c_void_p), f2.ctypes.data_as(C.c_void_p),
                                     x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p))
    assert got == n
    return x1, x2, f1, f2


def encode_result(mode: str, t: float, x1: np.ndarray, x2: np.ndarray, out_row: np.ndarray) -> bytes:
    """Native twin of ``wire.frame_result``: one length-prefixed result packet for a ``vapx_step`` output row."""
    lib = _engine.load_library()
    x1 = np.ascontiguousarray(x1, np.float64)
    x2 = np.ascontiguousarray(x2, np.float64)
    row = np.ascontiguousarray(out_row, np.float32)
    assert row.size >= _engine.OUT_STRIDE and x1.size == x2.size
    need = lib.vapx_wire_encode_result(MODE[mode], t, x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), x1.size,
                                       row.ctypes.data_as(C.c_void_p), None, 0)
    if need < 0:
        raise ValueError(f"vapx_wire_encode_result failed ({need})")
    dst = np.empty(need, np.uint8)
    got = lib.vapx_wire_encode_result(MODE[mode], t, x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), x1.size,
                                      row.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), need)
    assert got == need
    return dst.tobytes()


def link_pair():
    """(door end, worker end) of a front-door link: ``socket.socketpair(AF_UNIX, SOCK_SEQPACKET)``; hand the worker end to the process that owns
    the GPU (``subprocess.Popen(..., pass_fds=[worker.fileno()])``), keep both objects alive as long as the link is used."""
    import socket
    a, b = socket.socketpair(socket.AF_UNIX, socket.SOCK_SEQPACKET)
    a.set_inheritable(False)
    b.set_inheritable(True)
    return a, b


class RemoteFrontDoor:
    """The reference's ONE port pair in front of N per-GPU WORKER PROCESSES (``vapx_frontdoor_open_links``): this process only accepts, decides the
    dialogue's GPU and slot (same placement as ``FrontDoor``) and passes the socket on; engines, audio and results never come here.  ``links`` are
    the door ends of ``link_pair()``; every worker runs a passive ``NativeServer`` with ``attach_link(worker_end)``.  The constructor waits for the
    workers' greetings (they may still be loading weights)."""

    def __init__(self, links, port_in: int = 50007, port_out: int = 50008, bind_any: bool = False):
        self.lib = _engine.load_library()
        self._links = list(links)
        fds = [l if isinstance(l, int) else l.fileno() for l in self._links]
        arr = (C.c_int32 * len(fds))(*fds)
        h = C.c_void_p()
        rc = self.lib.vapx_frontdoor_open_links(arr, len(fds), port_in, port_out, int(bool(bind_any)), C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_frontdoor_open_links failed ({rc}): a worker did not greet (died while starting?), the workers disagree on "
                                    f"frame rate / mode, or the ports are taken")
        self._h = h
        a, b = C.c_int32(0), C.c_int32(0)
        self.lib.vapx_frontdoor_ports(self._h, C.byref(a), C.byref(b))
        self.port_in, self.port_out = a.value, b.value

    counts = None      # (bound below: same as FrontDoor.counts)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vapx_frontdoor_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FrontDoor:
    """ONE port pair in front of N per-GPU front-ends (``vapx_frontdoor_*``): the reference's single ``port_num_in`` / ``port_num_out``
    (vap_main.py:338-366,470-471) for a whole node.  ``shards`` are ``NativeServer`` objects opened PASSIVE (``port_in=-1, port_out=-1``),
    one per engine / GPU.  Dialogue slots are global, ``g = local_slot * N + shard``: input connections take the lowest free one (GPUs
    fill evenly; a reconnecting dialogue returns to the GPU holding its state while its slot is the lowest free one), the k-th output
    connection hears the k-th dialogue."""

    def __init__(self, shards, port_in: int = 50007, port_out: int = 50008, bind_any: bool = False):
        self.lib = _engine.load_library()
        self.shards = list(shards)
        arr = (C.c_void_p * len(self.shards))(*[s._h.value for s in self.shards])
        h = C.c_void_p()
        rc = self.lib.vapx_frontdoor_open(arr, len(self.shards), port_in, port_out, int(bool(bind_any)), C.byref(h))
        if rc != 0:
            raise _engine.VapxError(f"vapx_frontdoor_open failed ({rc}): shards must be passive front-ends of one frame rate and mode, ports free")
        self._h = h
        a, b = C.c_int32(0), C.c_int32(0)
        self.lib.vapx_frontdoor_ports(self._h, C.byref(a), C.byref(b))
        self.port_in, self.port_out = a.value, b.value

    @staticmethod
    def owner_of(global_slot: int, n_shards: int):
        """(shard, local slot) of a global dialogue slot."""
        return global_slot % n_shards, global_slot // n_shards

    def counts(self) -> dict:
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.vapx_frontdoor_counts(self._h, C.byref(a), C.byref(b), C.byref(c))
        return {"accepted_in": a.value, "accepted_out": b.value, "refused": c.value}

    def stats(self, reset_latency_window: bool = False) -> list:
        return [s.stats(reset_latency_window) for s in self.shards]

    def close(self, close_shards: bool = True):
        if getattr(self, "_h", None):
            self.lib.vapx_frontdoor_close(self._h)
            self._h = None
        if close_shards:
            for s in self.shards:
                s.close()

    stop = close

    def __del__(self):
        try:
            self.close(close_shards=False)
        except Exception:
            pass


RemoteFrontDoor.counts = FrontDoor.counts
