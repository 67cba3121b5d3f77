"""Input sample formats: 16-bit linear PCM and G.711 mu-law / A-law, decoded to fp32 on the device (vapx.h "Input format").

This file is the definition, in the role ``resample.py`` plays for the taps: csrc/pcm.hip, the front-end's echo (csrc/ingest.cpp) and the
client-side encoders of ``wire.py`` are all held against the tables below, and ``write_tables_header`` writes them into
csrc/pcm_tables.h.  A sample's value is its 16-bit linear expansion times 2**-15, which is exact in fp32: nothing here rounds.

  format  id  bytes/sample  value
  f32     0   4             the float itself (an engine that never asked for a format)
  s16     1   2, LE         float(v) * 2**-15
  mulaw   2   1             float(U[c]) * 2**-15
  alaw    3   1             float(A[c]) * 2**-15

U and A are the ITU-T G.711 expansions to 16-bit linear (the values of the standard library's audioop.ulaw2lin / alaw2lin)."""
from __future__ import annotations

import os

import numpy as np

FORMATS = {"f32": 0, "s16": 1, "mulaw": 2, "alaw": 3}
NAMES = {v: k for k, v in FORMATS.items()}
BYTES_PER_SAMPLE = {"f32": 4, "s16": 2, "mulaw": 1, "alaw": 1}
DTYPES = {"f32": np.dtype("<f4"), "s16": np.dtype("<i2"), "mulaw": np.dtype(np.uint8), "alaw": np.dtype(np.uint8)}
SILENCE = {"f32": 0.0, "s16": 0, "mulaw": 0xFF, "alaw": 0xD5}     # the sample of smallest magnitude: 0.0, except A-law's 8 * 2**-15
SCALE = 2.0 ** -15


def format_id(fmt) -> int:
    """Name or id -> id; anything else is refused by name."""
    if isinstance(fmt, str):
        if fmt not in FORMATS:
            raise ValueError(f"unknown input format {fmt!r}: one of {', '.join(FORMATS)}")
        return FORMATS[fmt]
    if int(fmt) not in NAMES:
        raise ValueError(f"unknown input format id {fmt}: 0 (f32), 1 (s16), 2 (mulaw), 3 (alaw)")
    return int(fmt)


def format_name(fmt) -> str:
    return NAMES[format_id(fmt)]


def mulaw_expand(c: int) -> int:
    """G.711 mu-law code -> 16-bit linear."""
    c = ~c & 0xFF
    e, m = (c >> 4) & 7, c & 15
    t = (((m << 3) + 0x84) << e) - 0x84
    return -t if c & 0x80 else t


def alaw_expand(c: int) -> int:
    """G.711 A-law code -> 16-bit linear."""
    c ^= 0x55
    e, m = (c >> 4) & 7, c & 15
    t = (m << 4) + 8 if e == 0 else ((m << 4) + 0x108) << (e - 1)
    return t if c & 0x80 else -t


MULAW = np.array([mulaw_expand(c) for c in range(256)], dtype=np.int16)
ALAW = np.array([alaw_expand(c) for c in range(256)], dtype=np.int16)
TABLES = {"mulaw": MULAW, "alaw": ALAW}


def linear(fmt, raw: np.ndarray) -> np.ndarray:
    """Raw samples -> their 16-bit linear values (int16); ``fmt`` is s16, mulaw or alaw."""
    name = format_name(fmt)
    if name == "f32":
        raise ValueError("f32 samples have no 16-bit linear form")
    raw = np.asarray(raw)
    if raw.dtype != DTYPES[name]:
        raise TypeError(f"{name} samples are {DTYPES[name].name}, not {raw.dtype.name}")
    return raw.astype(np.int16) if name == "s16" else TABLES[name][raw]


def decode(fmt, raw: np.ndarray, dtype=np.float32) -> np.ndarray:
    """Raw samples -> floats (``dtype`` float32 or float64; both hold every value exactly).  Integer zero gives +0.0."""
    if format_name(fmt) == "f32":
        return np.asarray(raw, dtype=np.float32).astype(dtype)
    return linear(fmt, raw).astype(dtype) * dtype(SCALE)


def _g711_encoder(table: np.ndarray):
    """Nearest table value, ties to the smaller magnitude; among codes of equal value (mu-law's two zeros) the one with the positive sign
    bit.  Returns (the distinct table values in ascending order, the code of each)."""
    order = sorted(range(256), key=lambda c: (int(table[c]), -c))
    vals, codes = [], []
    for c in order:
        v = int(table[c])
        if vals and vals[-1] == v:
            continue                                         # the first of equal values is kept: the larger code (0xFF for mu-law's zero)
        vals.append(v)
        codes.append(c)
    return np.array(vals, np.int64), np.array(codes, np.uint8)


_ENC = {name: _g711_encoder(t) for name, t in TABLES.items()}


def encode(fmt, x) -> np.ndarray:
    """What a client does: floats in [-1, 1) -> raw samples.  s16: round(x * 2**15) clipped to int16.  G.711: the code whose table value
    is nearest to that 16-bit value, ties to the smaller magnitude.  decode(encode(x)) == x for every x that a format can hold."""
    name = format_name(fmt)
    x = np.asarray(x, dtype=np.float64)
    if name == "f32":
        return x.astype(np.float32)
    v = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int64)
    if name == "s16":
        return v.astype("<i2")
    vals, codes = _ENC[name]
    hi = np.clip(np.searchsorted(vals, v, side="left"), 0, len(vals) - 1)      # first table value >= v
    lo = np.clip(hi - 1, 0, len(vals) - 1)
    dh, dl = np.abs(vals[hi] - v), np.abs(v - vals[lo])
    take_lo = (dl < dh) | ((dl == dh) & (np.abs(vals[lo]) < np.abs(vals[hi])))
    return codes[np.where(take_lo, lo, hi)]


def tables_header_text() -> str:
    """csrc/pcm_tables.h: the two 256-entry int16 tables."""
    lines = ["// Written by vap-realtime_amd/pcm.py (write_tables_header): the ITU-T G.711 expansions of the 256 mu-law and A-law codes to 16-bit",
             "// linear.  A sample's value is the entry times 2^-15.  Do not edit.",
             "#pragma once"]
    for name, t in (("MULAW", MULAW), ("ALAW", ALAW)):
        lines.append(f"#define VAPX_PCM_{name}_TABLE \\")
        rows = [", ".join(str(int(v)) for v in t[i:i + 16]) for i in range(0, 256, 16)]
        lines.append(", \\\n".join("  " + r for r in rows))
    return "\n".join(lines) + "\n"


def write_tables_header(path: str):
    text = tables_header_text()
    if os.path.exists(path) and open(path).read() == text:
        os.utime(path)                                       # up to date for make, content untouched
        return
    with open(path, "w") as f:
        f.write(text)
