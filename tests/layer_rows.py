"""Row-level check of the transformer's per-layer buffers against the float64 oracle.

The step's outputs see the window through the newest row of the last layer only; every older row of
layers 0-2 reaches them through attention weights spread over T keys and damped by ALiBi.  So the tests
that need to see a kernel that is wrong on some rows compare the rows themselves: ``o`` (ar_channel
layer 0) and ``stereo0..2`` (the three stereo layers), every valid row of every (stream, channel).

The bound is not tuned to the kernels.  It is the torch fp32 oracle's own error on the same buffer of
the same window, times a small factor:

    bound = FACTOR * max(E32, FLOOR * max|x|)

with E32 = max |oracle_fp32 - oracle_float64| over the buffer's valid rows and max|x| the largest
magnitude among them.  ``tests/test_layer_rows.py`` proves on the CPU that this bound rejects a 1e-3
relative error in one 32-row tile of one attention output in every layer and window class, so a larger
factor fails there.
"""
from typing import Dict, Optional, Sequence

import numpy as np

FACTOR = 8.0
FLOOR = 1e-6
TILE = 32
BUFFERS = ("o", "stereo0", "stereo1", "stereo2")
LAYER = {"o": "ar_channel.layers.0", "stereo0": "ar.layers.0", "stereo1": "ar.layers.1", "stereo2": "ar.layers.2"}


def row_bound(want64: np.ndarray, want32: np.ndarray):
    """(bound, E32) for one buffer of one stream: [2, n, 256] float64 truth and fp32 oracle rows."""
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    scale = float(np.abs(want64).max())
    return FACTOR * max(e32, FLOOR * scale), e32


def check_rows(buf: str, got: np.ndarray, ns: Sequence[int], want64: Sequence[np.ndarray], want32: Sequence[np.ndarray],
               streams: Optional[Sequence] = None, what: str = "", excess: Optional[dict] = None) -> float:
    """Check one peeked buffer.  ``got``: [B, 2, T, 256] as ``Engine.peek`` returns it (batch rows in the step's order,
    window rows chronological, rows t >= n undefined); ``ns[b]``: valid rows of batch row b; ``want64[b]`` / ``want32[b]``:
    the oracles' rows [2, ns[b], 256] of that stream.  Returns the worst err / E32 over the batch.  Fails on the first
    batch row with a non-finite valid row or a valid row beyond the bound, naming stream, channel, row, tile and layer.
    ``excess[buf]``, if given, collects the worst err / bound (the asserted figure: it cannot pass 1)."""
    streams = list(range(len(ns))) if streams is None else list(streams)
    worst = 0.0
    for b, n in enumerate(ns):
        w64 = np.asarray(want64[b], dtype=np.float64)
        assert w64.shape == (2, n, 256), (buf, b, w64.shape, n)
        g = got[b, :, :n].astype(np.float64)
        where = f"{what} stream {streams[b]}"
        fin = np.isfinite(g).all(axis=2)
        if not fin.all():
            c, t = _first_row(~fin)
            raise AssertionError(f"{where}: non-finite value in channel {c} row {t} (tile {t // TILE}) of {buf} "
                                 f"({LAYER[buf]}), n = {n}")
        bound, e32 = row_bound(w64, want32[b])
        err = np.abs(g - w64).max(axis=2)                      # [2, n]
        bad = err > bound
        if bad.any():
            c, t = _first_row(bad)
            raise AssertionError(f"{where}: channel {c} row {t} (tile {t // TILE}) of {buf} ({LAYER[buf]}) is off by "
                                 f"{err[c, t]:.3e} > bound {bound:.3e} (E32 {e32:.3e}, worst {err.max():.3e}), n = {n}")
        worst = max(worst, float(err.max()) / max(e32, 1e-30))
        if excess is not None:
            excess[buf] = max(excess.get(buf, 0.0), float(err.max()) / bound)
    return worst


def _first_row(mask: np.ndarray):
    """(channel, row) of the earliest flagged row of a [2, n] mask."""
    rows = np.flatnonzero(mask.any(axis=0))
    t = int(rows[0])
    return int(np.flatnonzero(mask[:, t])[0]), t


def split_rows(ref: Dict[str, np.ndarray], k: int) -> Dict[str, np.ndarray]:
    """Stream k's rows [2, n, 256] of every buffer of an ``VapOracle.layers`` result."""
    return {name: v[k] for name, v in ref.items()}
