"""The one resampling filter of the project: 8 / 32 / 48 kHz input to the model's 16 kHz, in float64.

It restates ``torchaudio.functional.resample``'s default (``sinc_interp_hann``, ``lowpass_filter_width = 6``, ``rolloff = 0.99``), the
filter through which the telephone corpora reached the published checkpoints.  With ``g = gcd(in_hz, 16000)``, ``orig = in_hz / g``,
``new = 16000 / g``::

    base  = min(orig, new) * 0.99
    width = ceil(6 * orig / base)
    K     = 2 * width + orig
    t[p][k] = (-p / new + (k - width) / orig) * base      clamped to [-6, 6],   p in [0, new), k in [0, K)
    h[p][k] = sinc(pi * t) * cos(pi * t / 12)^2 * base / orig                    (sinc(0) = 1), then rounded to fp32
    Y[new*i + p] = sum_k h[p][k] * x[orig*i + k - width]                         (x = 0 outside the signal)

``taps`` is that table; ``csrc/resample_taps.h`` is written from it (``write_taps_header``), so the HIP kernel, the tests and every
client that wants to reproduce the engine use the same numbers.

Streaming form (what an engine with an input rate computes, csrc/resample.hip).  A dialogue has no future samples, so the 16 kHz
stream the model sees is ``Y`` delayed by ``d = ceil(width / orig)`` whole blocks: ``z[m] = Y[m - new*d]`` and zero for ``m < new*d``
(d = 7 for all three rates: 0.875 ms at 8 kHz, 0.4375 ms at 32 and 48 kHz).  Tick ``t`` consumes ``x[t*hop_in, (t+1)*hop_in)`` and
emits ``z[t*hop, (t+1)*hop)``; for that it keeps the last ``H = orig*d + width`` input samples of a stream (``stream_ref``).
"""
from __future__ import annotations

import math
import os

import numpy as np

MODEL_HZ = 16000
RATES = (8000, 32000, 48000)            # 16000 = no resampling
LOWPASS_WIDTH = 6
ROLLOFF = 0.99


def geometry(in_hz: int) -> dict:
    """``orig, new, width, K, d, H`` of a supported rate; ``ValueError`` for any other (16000 included: nothing to resample)."""
    if int(in_hz) not in RATES:
        raise ValueError(f"input rate {in_hz} Hz: supported are {', '.join(map(str, RATES))} (and 16000 = no resampling)")
    g = math.gcd(int(in_hz), MODEL_HZ)
    orig, new = int(in_hz) // g, MODEL_HZ // g
    base = min(orig, new) * ROLLOFF
    width = math.ceil(LOWPASS_WIDTH * orig / base)
    d = -(-width // orig)
    return {"orig": orig, "new": new, "base": base, "width": width, "K": 2 * width + orig, "d": d, "H": orig * d + width}


def hop_in(in_hz: int, frame_hz: int) -> int:
    """Input samples per channel and frame."""
    return int(in_hz) // int(frame_hz)


def history_floats(in_hz: int) -> int:
    """Floats the history [2][H] takes in a state record: padded to a multiple of 4; 0 for 16000."""
    return 0 if int(in_hz) == MODEL_HZ else (2 * geometry(in_hz)["H"] + 3) // 4 * 4


def taps(in_hz: int) -> np.ndarray:
    """h[new][K]: the float64 formula, rounded to fp32 and returned as float64 (exactly the values the kernel multiplies by)."""
    q = geometry(in_hz)
    k = np.arange(q["K"], dtype=np.float64)
    p = np.arange(q["new"], dtype=np.float64)
    t = (-p[:, None] / q["new"] + (k[None, :] - q["width"]) / q["orig"]) * q["base"]
    t = np.clip(t, -LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = np.cos(t * np.pi / LOWPASS_WIDTH / 2) ** 2
    tp = t * np.pi
    sinc = np.where(tp == 0, 1.0, np.sin(tp) / np.where(tp == 0, 1.0, tp))
    h = sinc * window * (q["base"] / q["orig"])
    return h.astype(np.float32).astype(np.float64)


def whole_ref(x: np.ndarray, in_hz: int) -> np.ndarray:
    """Y of a whole signal ``x`` [..., n_in] in float64: [..., ceil(new * n_in / orig)]."""
    q = geometry(in_hz)
    orig, new, width, K = q["orig"], q["new"], q["width"], q["K"]
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[-1]
    n_out = -(-new * n_in // orig)
    nblk = -(-n_out // new)
    xp = np.zeros(x.shape[:-1] + (width + orig * nblk + K,), np.float64)
    xp[..., width:width + n_in] = x
    h = taps(in_hz)
    y = np.zeros(x.shape[:-1] + (nblk, new), np.float64)
    for kk in range(K):                                      # the same order of summation for every output
        seg = xp[..., kk:kk + orig * nblk:orig]
        for p in range(new):
            y[..., p] = y[..., p] + h[p, kk] * seg
    return y.reshape(x.shape[:-1] + (nblk * new,))[..., :n_out]


def delayed(y: np.ndarray, in_hz: int, n_out: int) -> np.ndarray:
    """z[..., n_out]: ``y`` shifted by new*d samples, zeros in front (the stream an engine with this input rate feeds its model)."""
    q = geometry(in_hz)
    shift = q["new"] * q["d"]
    z = np.zeros(y.shape[:-1] + (n_out,), y.dtype)
    take = max(0, min(n_out - shift, y.shape[-1]))
    z[..., shift:shift + take] = y[..., :take]
    return z


def stream_state(in_hz: int, shape=()) -> dict:
    """A fresh stream: zero history, nothing consumed yet."""
    return {"hist": np.zeros(tuple(shape) + (geometry(in_hz)["H"],), np.float64), "started": False}


def stream_ref(chunk: np.ndarray, state: dict, in_hz: int) -> np.ndarray:
    """One tick of the streaming form in float64: ``chunk`` [..., hop_in] (a multiple of orig) -> [..., hop]; ``state`` is updated in
    place.  The first d blocks after a fresh start are zero (``z[m] = 0`` for ``m < new*d``): ``Y`` has no samples there."""
    q = geometry(in_hz)
    orig, new, K, d, H = q["orig"], q["new"], q["K"], q["d"], q["H"]
    chunk = np.asarray(chunk, dtype=np.float64)
    n = chunk.shape[-1]
    assert n % orig == 0 and n >= H
    nblk = n // orig
    buf = np.concatenate([state["hist"], chunk], axis=-1)
    h = taps(in_hz)
    out = np.zeros(chunk.shape[:-1] + (nblk, new), np.float64)
    for kk in range(K):
        seg = buf[..., kk:kk + orig * nblk:orig]
        for p in range(new):
            out[..., p] = out[..., p] + h[p, kk] * seg
    if not state["started"]:
        out[..., :d, :] = 0.0
    state["hist"] = buf[..., n:]                             # the last H samples
    state["started"] = True
    return out.reshape(chunk.shape[:-1] + (nblk * new,))


def taps_header_text() -> str:
    """csrc/resample_taps.h: the fp32 tables of the three rates, nine significant digits (round-trips fp32)."""
    lines = ["// Written by vap-realtime_amd/resample.py (write_taps_header): the fp32 taps h[new][K] of torchaudio's default resampler",
             "// (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) for 8 / 32 / 48 kHz -> 16 kHz.  Do not edit.",
             "#pragma once"]
    for hz in RATES:
        q, h = geometry(hz), taps(hz)
        lines.append(f"// {hz} Hz: orig {q['orig']}, new {q['new']}, width {q['width']}, K {q['K']}, d {q['d']}, H {q['H']}")
        vals = ", ".join(f"{float(v):.9e}f" for v in h.reshape(-1))
        lines.append(f"#define VAPX_RESAMPLE_TAPS_{hz} {vals}")
    return "\n".join(lines) + "\n"


def write_taps_header(path: str):
    text = taps_header_text()
    if os.path.exists(path) and open(path).read() == text:
        os.utime(path)                                       # up to date for make, content untouched
        return
    with open(path, "w") as f:
        f.write(text)
