"""Stage-level check of the CPC encoder's buffers against the float64 oracle: the analogue of tests/layer_rows.py for
conv0 .. conv4, the LSTM and the downsample.

The step's outputs see the encoder through ``e`` at 1e-4 absolute, which is too coarse to notice a ChannelNorm epsilon
that is wrong by ten times in one layer (tests/test_encoder_stages.py shows it).  So every stage buffer is compared by
value: ``h0`` .. ``h3`` (conv0 .. conv3 after ChannelNorm and ReLU, channels-last with zero guard rows), ``z``
(conv4, positions 1 .. P4-2), ``lstm_out``, ``e``, and the persistent LSTM state and carry.

The bound is ``layer_rows.row_bound`` unchanged, taken per batch row over that stream's [2, P, 256] block:

    bound = factor(stage) * max(E32, FLOOR * max|x|)

with E32 the torch fp32 oracle's own error on the same block (2-9e-7 of max|x| on these stages, so FLOOR = 1e-6 usually sets the
bound: 8e-6 of the block's largest value).  factor(stage) is ``layer_rows.FACTOR`` for every stage
(``STAGE_FACTOR`` holds nothing today): a stage may only be raised as far as tests/test_encoder_stages.py still rejects every fault of
that stage with a 1.5 x margin, and never from the kernels' error alone.

Guard rows of ``h0`` .. ``h3`` must be exactly 0.0.  The edge positions of ``h0`` .. ``h3`` do not reach
``z[:, 1:-1]`` (``live_range``); they are checked all the same, because ``Engine.peek`` promises the reference's hook
values, and a failure there says so.
"""
from typing import Dict, Optional, Sequence

import numpy as np

from layer_rows import FACTOR, FLOOR, TILE

STAGES = ("h0", "h1", "h2", "h3", "z", "lstm_out", "e")
GUARD = {"h0": 2, "h1": 1, "h2": 1, "h3": 1}          # zero rows on each side of a stream's block
STAGE_FACTOR: Dict[str, float] = {}                    # stage -> factor where it differs from layer_rows.FACTOR
MARGIN = 1.5                                           # what a raised factor must leave of every CPU-proof rejection
LSTM_TILE = 16                                         # lstm_kernel takes 16 rows of [B * 2] per workgroup
PAD = 320


def geometry(hz: int) -> Dict[str, int]:
    """Positions per stage of one frame at this frame rate (conv strides 5, 4, 2, 2, 2 on hop + 320 samples)."""
    L = 16000 // hz + PAD
    P0 = L // 5
    P1 = P0 // 4
    P2 = P1 // 2
    P3 = P2 // 2
    P4 = P3 // 2
    return {"h0": P0, "h1": P1, "h2": P2, "h3": P3, "z": P4 - 2, "lstm_out": P4 - 2, "e": 1}


def live_range(stage: str, P: int):
    """[lo, hi] of the positions of ``h0`` .. ``h3`` that reach ``z[:, 1:-1]``: conv4 / conv3 / conv2 (k 4, s 2, p 1) at outputs
    1 .. P-2 read inputs 1 .. 2P-2 of the 2P below, conv1 (k 8, s 4, p 2) at outputs 1 .. P1-2 reads inputs 2 .. P0-3."""
    if stage == "h0":
        return 2, P - 3
    if stage in ("h1", "h2", "h3"):
        return 1, P - 2
    return 0, P - 1


def kernel_of(stage: str, path: str) -> str:
    """The kernel that writes ``stage`` on an encoder path: "fused" (fp32, conv_tail_kernel), "chain" (fp32 implicit GEMMs),
    "split" (split-precision implicit GEMMs), "follower" / "follower_split" (a trunk follower's own downsample)."""
    gemm = "gemm_f32_kernel<SPLIT>" if path.endswith("split") else "gemm_f32_kernel"
    if stage == "h0":
        return "conv0_kernel"
    if stage in ("h1", "h2", "h3"):
        return f"conv{stage[1]}: {gemm} EPI_CN_RELU"
    if stage == "z":
        return "conv2-4: conv_tail_kernel" if path == "fused" else f"conv4: {gemm} EPI_CN_RELU"
    if stage == "lstm_out":
        return f"gx {gemm} + lstm_kernel"
    if stage == "e":
        return f"downsample: {gemm} EPI_BIAS_LN_GELU" if path.startswith("follower") else "downsample in lstm_kernel"
    return "lstm_kernel, persistent state"


def stage_bound(stage: str, want64: np.ndarray, want32: np.ndarray):
    """(bound, E32, max|x|) of one stream's block: layer_rows.row_bound with this stage's factor."""
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    scale = float(np.abs(want64).max())
    return STAGE_FACTOR.get(stage, FACTOR) * max(e32, FLOOR * scale), e32, scale


def collect_stages(oracle, frames, state) -> Dict[str, np.ndarray]:
    """One ``VapOracle.encode`` of ``frames`` [S, 2, L]: every stage as [S, 2, P, 256] (``e`` with P = 1), plus the LSTM state
    ``h`` and ``c`` [S, 2, 1, 256] after the frame.  Advances ``state.h / .c``; the window ring is not touched."""
    import torch
    col: dict = {}
    x = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.float32)).to(oracle.dtype)
    with torch.no_grad():
        e = oracle.encode(x, state, col)
    S = x.shape[0]
    out = {}
    for i in range(4):
        c = col[f"cnn{i}"]                                           # [S * 2, 256, P]
        out[f"h{i}"] = c.transpose(1, 2).reshape(S, 2, c.shape[2], 256).numpy()
    out["z"] = col["z"].numpy()
    out["lstm_out"] = col["lstm_out"].numpy()
    out["e"] = e.numpy()[:, :, None, :]
    out["h"] = state.h.numpy()[:, :, None, :].copy()
    out["c"] = state.c.numpy()[:, :, None, :].copy()
    return out


def with_guards(stage: str, x: np.ndarray) -> np.ndarray:
    """[..., P, 256] -> [..., P + 2g, 256] with the stage's zero guard rows, the layout ``Engine.peek`` returns."""
    g = GUARD.get(stage, 0)
    if not g:
        return x
    pad = [(0, 0)] * (x.ndim - 2) + [(g, g), (0, 0)]
    return np.pad(x, pad)


def check_stage(stage: str, got: np.ndarray, want64: Sequence[np.ndarray], want32: Sequence[np.ndarray], *, path: str = "",
                streams: Optional[Sequence] = None, what: str = "", excess: Optional[dict] = None) -> float:
    """Check one encoder buffer of a batch.  ``got``: [B, 2, P + 2g, 256] as ``Engine.peek`` returns it (g guard rows on each side
    for ``h0`` .. ``h3``); ``want64[b]`` / ``want32[b]``: the oracles' [2, P, 256] block of batch row b.  Returns the worst
    err / E32 over the batch.  Fails on the first batch row with a non-zero guard row, a non-finite value or a row beyond the bound,
    naming stage, kernel, stream, channel, position, column and the 32-row and 32-column tile of the value.  ``excess[key]``, if
    given, collects the worst err / bound under key = stage (err / E32 can pass 8 where FLOOR sets the bound, err / bound cannot pass 1)."""
    B = got.shape[0]
    streams = list(range(B)) if streams is None else list(streams)
    assert len(want64) == B and len(want32) == B, (stage, B, len(want64), len(want32))
    g0 = GUARD.get(stage, 0)
    kern = kernel_of(stage, path)
    worst = 0.0
    for b in range(B):
        w64 = np.asarray(want64[b], dtype=np.float64)
        P = w64.shape[1]
        assert got.shape[1:] == (2, P + 2 * g0, 256) and w64.shape == (2, P, 256), (stage, got.shape, w64.shape)
        where = f"{what} stream {streams[b]}: {stage} ({kern})"
        if g0:
            guards = np.concatenate([got[b, :, :g0], got[b, :, P + g0:]], axis=1)          # [2, 2g, 256]
            if not (guards == 0.0).all():
                c, r, col = (int(v[0]) for v in np.nonzero(guards != 0.0))
                row = r if r < g0 else P + r
                raise AssertionError(f"{where} channel {c}: guard row {row} of the [{P + 2 * g0}]-row block is not zero "
                                     f"(column {col}: {guards[c, r, col]!r}); guard rows stay zero forever")
        g = got[b, :, g0:g0 + P].astype(np.float64)

        def locate(c, t, col):
            m = (b * 2 + c) * P + t
            lo, hi = live_range(stage, P)
            edge = "" if lo <= t <= hi else (f"; edge position: it does not reach z[:, 1:-1] (live positions {lo} .. {hi}), "
                                             f"the step's outputs are not affected")
            tile = (f"row {b * 2 + c} of [B * 2] ({LSTM_TILE}-row tile {(b * 2 + c) // LSTM_TILE})" if stage in ("lstm_out", "e", "h", "c")
                    else f"row {m} of [B * 2 * {P}] ({TILE}-row tile {m // TILE})")
            return f"channel {c} position {t} column {col} ({tile}, {TILE}-column tile {col // TILE})", edge
        fin = np.isfinite(g)
        if not fin.all():
            c, t = _first_row(~fin.all(axis=2))
            col = int(np.flatnonzero(~fin[c, t])[0])
            at, edge = locate(c, t, col)
            raise AssertionError(f"{where}: non-finite value at {at}{edge}")
        bound, e32, scale = stage_bound(stage, w64, want32[b])
        diff = np.abs(g - w64)
        err = diff.max(axis=2)                                   # [2, P]
        bad = err > bound
        if bad.any():
            c, t = _first_row(bad)
            col = int(diff[c, t].argmax())
            at, edge = locate(c, t, col)
            raise AssertionError(f"{where}: {at} is off by {err[c, t]:.3e} > bound {bound:.3e} "
                                 f"(E32 {e32:.3e}, max|x| {scale:.3e}, worst {err.max():.3e} = {err.max() / bound:.2f} x bound){edge}")
        worst = max(worst, float(err.max()) / max(e32, 1e-30))
        if excess is not None:
            excess[stage] = max(excess.get(stage, 0.0), float(err.max()) / bound)
    return worst


def check_carry(got: np.ndarray, frame: np.ndarray, what: str = "") -> None:
    """The carry [2, 320] of one stream must be the last 320 samples of its latest frame [2, L], bit for bit."""
    want = np.ascontiguousarray(frame[:, -PAD:], dtype=np.float32)
    got = np.ascontiguousarray(got, dtype=np.float32)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        c, i = (int(v[0]) for v in np.nonzero(~same))
        raise AssertionError(f"{what}: carry channel {c} sample {i} is {got[c, i]!r}, the frame's sample is {want[c, i]!r} "
                             f"({int((~same).sum())} of {same.size} differ)")


def _first_row(mask: np.ndarray):
    """(channel, position) of the earliest flagged position of a [2, P] mask."""
    rows = np.flatnonzero(mask.any(axis=0))
    t = int(rows[0])
    return int(np.flatnonzero(mask[:, t])[0]), t
