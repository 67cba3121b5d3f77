"""Stage-level check of the tail of the step against the float64 oracle: the newest row of the last stereo layer, the combinator,
vap_head, the VAD and the bc / nod heads.  The analogue of tests/layer_rows.py and tests/encoder_stages.py for everything behind
``stereo1``.

Stages (``stages_of(mode)`` lists the ones a mode has):

    last        [2, 256]   last layer's output for the newest row of both channels (``collect["stereo2"][:, :, -1]``); on the device
                           ``peek("last")`` (last_block_kernel, or the ten launches of unfused_last_row), or row n - 1 of ``stereo2``
                           where the whole layer runs (full_last_layer, nod: head_kernel reads it with x_last_only = 0)
    comb        [n, 256]   nod: the combinator of every window row (run_combinator_all_rows, ``peek("comb")``)
    logits      [256]      vap_head of the newest row (vap, bc; a nod engine writes p_bc of the window rows over these slots)
    vad_logit   [2]        va_classifier on the newest row of ``o``, before the sigmoid
    p_now, p_future [2]    softmax -> 256 classes to 2 x 4 bins -> bins 0-1 / 2-3 -> x / (sum + 1e-5)   (objective.py:186-206)
    vad         [2]        sigmoid(vad_logit)
    aux         [3] / [4]  EVERY column of the bc / nod softmax, also the column 0 that the reference drops
    p_bc_rows   [n]        nod: sigmoid(bc_head(comb)) of every window row (pbc_rows_kernel)

The bound is the project's rule, unchanged:

    bound = factor(stage) * max(E32, FLOOR * max|x|),   FACTOR = 8, FLOOR = 1e-6

E32 = max |oracle_fp32 - oracle_float64| is POOLED over the streams of the tick (several stages have 2-4 numbers per stream: a
per-stream E32 would be noise); max|x| stays the stream's own.  factor(stage) is ``layer_rows.FACTOR`` unless ``STAGE_FACTOR`` names
the stage, and a stage may only be named there while tests/test_head_stages.py still rejects every seeded fault of that stage with a
``MARGIN`` = 1.5 x margin (the test asserts it), never from what the kernels give.

``check_own`` is the second, sharper check of the probability outputs: p_now / p_future and vad recomputed in float64 on the host from
the values the checked path itself emitted (its ``logits`` and ``vad_logit``), so that the device's softmax, aggregation and sigmoid
code stands alone, without the error of everything upstream; held to FACTOR * FLOOR * max|p|.
"""
from typing import Dict, Optional, Sequence

import numpy as np

from layer_rows import FACTOR, FLOOR

STAGES = ("last", "comb", "logits", "vad_logit", "p_now", "p_future", "vad", "aux", "p_bc_rows")
AUX_COLS = {"vap": 0, "bc": 3, "nod": 4}
STAGE_FACTOR: Dict[str, float] = {}                    # stage -> factor where it differs from layer_rows.FACTOR
MARGIN = 1.5                                           # what a raised factor must leave of every CPU-proof rejection
OWN = ("p_now", "p_future", "vad")                     # the stages check_own recomputes

_IDX = np.arange(256)
_BITS = ((_IDX[:, None] >> np.arange(8)[None, :]) & 1).astype(np.float64).reshape(256, 2, 4)   # states[i, c, b] = bit(4c + b)
W_NOW = _BITS[:, :, 0:2].sum(-1)                       # [256, 2]: bins 0-1
W_FUTURE = _BITS[:, :, 2:4].sum(-1)                    # bins 2-3


def stages_of(mode: str):
    if mode == "nod":
        return ("last", "comb", "vad_logit", "p_now", "p_future", "vad", "aux", "p_bc_rows")
    return ("last", "logits", "vad_logit", "p_now", "p_future", "vad") + (("aux",) if mode == "bc" else ())


def kernel_of(stage: str, path: str = "") -> str:
    """The device code that writes ``stage``; ``path``: "fused" (last_block_kernel), "unfused" (VAPX_FLAG_UNFUSED_LAST_ROW), "full"
    (every row of the last layer: full_last_layer, nod), with "_split" appended on the split_f16 path."""
    if stage == "last":
        if path.startswith("unfused"):
            return "gather_last_ln_kernel + attention_last_kernel + M = 2B GEMMs"
        if path.startswith("full"):
            return "row n - 1 of stereo2, which head_kernel reads with x_last_only = 0"
        return "last_block_kernel"
    if stage == "comb":
        return "run_combinator_all_rows"
    if stage == "p_bc_rows":
        return "pbc_rows_kernel"
    return "head_kernel"


def collect_heads(oracle, frame, state, pre: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """One ``VapOracle.step`` of ``frame`` [S, 2, L]: every stage the oracle's mode has as [S, ...] (``comb`` [S, n, 256] and
    ``p_bc_rows`` [S, n] only where the mode is nod; ``logits`` also for nod, where only the device lacks them), plus ``e``
    [S, 2, 256] and ``n``.  ``pre``: a dict that receives the inputs of the oracle's non-linearities (``VapOracle._collect_pre``)."""
    col: dict = {} if pre is None else {"pre": pre}
    out = oracle.step(frame, state, col)
    res = {"last": col["stereo2"][:, :, -1].numpy(), "logits": out["logits"], "vad_logit": col["vad_logit"].numpy(),
           "p_now": out["p_now"], "p_future": out["p_future"], "vad": out["vad"], "e": out["e"], "n": len(state.ring)}
    if oracle.mode in ("bc", "nod"):
        res["aux"] = col["aux"].numpy()
        if "aux_logit" in col:                                   # for ``propagate``; no path emits it
            res["aux_logit"] = col["aux_logit"].numpy()
    if oracle.mode == "nod":
        res["comb"] = col["comb"].numpy()
        res["p_bc_rows"] = out["p_bc"]
        if "p_bc_logit" in col:
            res["p_bc_logit"] = col["p_bc_logit"].numpy()
    return res


def row_of(res: Dict[str, np.ndarray], k: int) -> Dict[str, np.ndarray]:
    """Stream k's share of a ``collect_heads`` result."""
    return {name: (v if name == "n" else v[k]) for name, v in res.items()}


def stage_bound(stage: str, e32: float, want64: np.ndarray):
    """(bound, max|x|) of one stream's block under the tick's pooled E32."""
    scale = float(np.abs(want64).max())
    return STAGE_FACTOR.get(stage, FACTOR) * max(e32, FLOOR * scale), scale


def pooled_e32(stage: str, want64: Sequence[dict], want32: Sequence[dict]) -> float:
    return max(float(np.abs(np.asarray(w32[stage], np.float64) - np.asarray(w64[stage], np.float64)).max())
               for w64, w32 in zip(want64, want32))


# ``propagate``: stage -> (the logits it is a sigmoid / a softmax column of, a, r).  For logits moved by at most B in the maximum norm the
# probability p moves by at most a p (1 - p) B + r B^2: a sigmoid has p' = p (1 - p) and |p''| <= 0.097; a softmax column has
# sum_j |dp_i / dz_j| = 2 p_i (1 - p_i) and sum_jk |d2p_i / dz_j dz_k| <= 6 p_i.  p is the float64 oracle's value, so a saturated
# probability (p (1 - p) -> 0) keeps its own bound
PROPAGATE = {"vad": ("vad_logit", 1.0, 0.05), "aux": ("aux_logit", 2.0, 3.0), "p_bc_rows": ("p_bc_logit", 1.0, 0.05)}


def check_tick(mode: str, got: Sequence[dict], want64: Sequence[dict], want32: Sequence[dict], *, path: str = "",
               streams: Optional[Sequence] = None, what: str = "", stages: Optional[Sequence[str]] = None,
               worst: Optional[dict] = None, excess: Optional[dict] = None, propagate: bool = False) -> None:
    """Check one tick.  ``got[b]`` / ``want64[b]`` / ``want32[b]``: batch row b's stages (``row_of`` layout; ``comb`` and ``p_bc_rows``
    hold that stream's n valid rows).  Stages run in pipeline order, and the first one with a non-finite value or a value beyond the
    bound fails, naming stage, device code, stream and position.  ``worst[stage]`` collects the largest err / E32, ``excess[stage]`` the
    largest err / bound (err / E32 may pass 8 where FLOOR sets the bound; err / bound cannot pass 1).

    ``propagate`` (off unless a caller asks; tests/test_weight_regimes_gpu.py does under its ``heads`` regime): the rule holds a head's
    logits to B = 8 x max(E32, 1e-6 max|logit|), so a path with an EXACT sigmoid / softmax may still be wrong on a probability p by
    a p (1 - p) B + r B^2 (``PROPAGATE``).  With head weights x 8 the logits reach 50 and, where p is not saturated, that passes the
    probability's own bound 8 x max(E32, 1e-6 max|p|) <= 8e-6 several times; then each value is held to max(the stage's own bound, that
    allowance at ITS float64 p), B taken from the two oracles' logits alone (``want64`` / ``want32``; the path's logits are not used)."""
    B = len(got)
    streams = list(range(B)) if streams is None else list(streams)
    assert len(want64) == B and len(want32) == B, (B, len(want64), len(want32))
    for stage in (stages_of(mode) if stages is None else stages):
        e32 = pooled_e32(stage, want64, want32)
        e32_src = pooled_e32(PROPAGATE[stage][0], want64, want32) if propagate and stage in PROPAGATE else 0.0
        for b in range(B):
            w64 = np.asarray(want64[b][stage], np.float64)
            g = np.asarray(got[b][stage], np.float64)
            where = f"{what} stream {streams[b]}: {stage} ({kernel_of(stage, path)})"
            assert g.shape == w64.shape, f"{where}: shape {g.shape}, the oracle's is {w64.shape}"
            if not np.isfinite(g).all():
                at = tuple(int(i[0]) for i in np.nonzero(~np.isfinite(g)))
                raise AssertionError(f"{where}: non-finite value at {at}")
            bound, scale = stage_bound(stage, e32, w64)
            diff = np.abs(g - w64)
            if propagate and stage in PROPAGATE:
                src, a, r = PROPAGATE[stage]
                bsrc = stage_bound(src, e32_src, np.asarray(want64[b][src], np.float64))[0]
                allowed = np.maximum(bound, a * w64 * (1.0 - w64) * bsrc + r * bsrc * bsrc)
                at = tuple(int(i) for i in np.unravel_index(int((diff / allowed).argmax()), diff.shape))
                bound = float(allowed[at])
            else:
                at = tuple(int(i) for i in np.unravel_index(int(diff.argmax()), diff.shape))
            err = float(diff[at])
            if err > bound:
                raise AssertionError(f"{where}: index {at} of {list(w64.shape)} is off by {err:.3e} > bound {bound:.3e} "
                                     f"(pooled E32 {e32:.3e}, max|x| {scale:.3e}: {err / bound:.2f} x bound; got {g[at]!r}, want {w64[at]!r})")
            if worst is not None:
                worst[stage] = max(worst.get(stage, 0.0), err / max(e32, 1e-30))
            if excess is not None:
                excess[stage] = max(excess.get(stage, 0.0), err / bound)


def own_probabilities(logits: Optional[np.ndarray], vad_logit: np.ndarray) -> Dict[str, np.ndarray]:
    """float64 p_now / p_future (objective.py:186-206: softmax, 256 classes -> 2 x 4 bins, bins 0-1 / 2-3, x / (sum + 1e-5)) of
    ``logits`` [..., 256] (None: left out) and vad = sigmoid(vad_logit)."""
    res = {"vad": 1.0 / (1.0 + np.exp(-np.asarray(vad_logit, np.float64)))}
    if logits is not None:
        z = np.asarray(logits, np.float64)
        p = np.exp(z - z.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        for name, w in (("p_now", W_NOW), ("p_future", W_FUTURE)):
            q = p @ w
            res[name] = q / (q.sum(axis=-1, keepdims=True) + 1e-5)
    return res


def check_own(got: Sequence[dict], *, streams: Optional[Sequence] = None, what: str = "", excess: Optional[dict] = None) -> None:
    """The sharper check: every row's p_now / p_future (where the row has ``logits``) and vad against ``own_probabilities`` of the
    row's own logits and vad_logit, within FACTOR * FLOOR * max|p|.  ``excess["own " + stage]`` collects the largest err / bound."""
    streams = list(range(len(got))) if streams is None else list(streams)
    for b, row in enumerate(got):
        own = own_probabilities(row.get("logits"), row["vad_logit"])
        for stage in OWN:
            if stage not in own:
                continue
            g = np.asarray(row[stage], np.float64)
            bound = FACTOR * FLOOR * float(np.abs(own[stage]).max())
            err = float(np.abs(g - own[stage]).max())
            if not np.isfinite(g).all() or err > bound:
                raise AssertionError(f"{what} stream {streams[b]}: {stage} (head_kernel) differs from float64 softmax / aggregation / sigmoid of "
                                     f"the path's OWN logits and vad_logit by {err:.3e} > {bound:.3e} = {FACTOR:g} x {FLOOR:g} x max|p| "
                                     f"(got {g.tolist()}, want {own[stage].tolist()})")
            if excess is not None:
                excess["own " + stage] = max(excess.get("own " + stage, 0.0), err / bound)


def check_exact(mode: str, out: np.ndarray, ns: Sequence[int], e_peek: np.ndarray, T: int, *, streams: Optional[Sequence] = None,
                what: str = "") -> None:
    """The fields of the output rows [B, 784] that are exact: n, status, the reserved slots, the aux slots a mode does not define, the
    zero p_bc slots of nod behind a stream's n rows, and the ``e`` copy, bit-equal to ``peek("e")`` [B, 2, 256]."""
    B = out.shape[0]
    streams = list(range(B)) if streams is None else list(streams)
    e_out = np.ascontiguousarray(out[:, 272:784]).view(np.uint32)
    e_want = np.ascontiguousarray(e_peek, np.float32).reshape(B, 512).view(np.uint32)
    for b in range(B):
        where = f"{what} stream {streams[b]}"
        assert out[b, 10] == float(ns[b]), f"{where}: out[OUT_NVALID] = {out[b, 10]!r}, the window holds {ns[b]} rows"
        assert out[b, 13] == 0.0, f"{where}: status {out[b, 13]!r}"
        assert (out[b, 14:16].view(np.uint32) == 0).all(), f"{where}: reserved slots 14 / 15 hold {out[b, 14:16]!r}"
        k = AUX_COLS[mode]
        assert (out[b, 6 + k:10].view(np.uint32) == 0).all(), f"{where}: aux columns {k} .. 3 of a {mode} engine hold {out[b, 6 + k:10]!r}"
        if mode == "nod":
            assert (out[b, 16 + ns[b]:16 + T] == 0.0).all(), f"{where}: p_bc slots {ns[b]} .. {T - 1} are not zero"
        if not (e_out[b] == e_want[b]).all():
            i = int(np.flatnonzero(e_out[b] != e_want[b])[0])
            raise AssertionError(f"{where}: e copy of the output row differs from peek(\"e\") at channel {i // 256} column {i % 256}")
