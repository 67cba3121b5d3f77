"""Attention maps of the oracle, and the check that holds the engine's maps against them.

``VapOracle._mha`` computes the softmax weights ``att`` and drops them; ``RecordingOracle`` restates it to keep them (with the
reference's own causal mask, whose kept entries are 1, so that its fp32 rounding is the reference's).  The call
order of ``VapOracle.transformer`` is fixed — o1, o2, then per stereo layer a-self, a-cross, b-self, b-cross — so one run yields the
14 maps (times 4 heads) the reference returns with ``attention=True`` (modules.py:356-423), in fp32 or float64, without touching
``oracle/``.

``check_maps`` has the form of ``tests/layer_rows.py`` applied to each map (one stream, channel, layer, head): the error against the
float64 oracle is bounded by ``layer_rows.FACTOR * max(E32, layer_rows.FLOOR)`` with E32 the fp32 oracle's own error on that map (a
softmax weight is <= 1, so the floor needs no scale); every row must be finite, sum to 1 within 1e-5, and be exactly 0 above the
diagonal.  ``tests/test_attention_maps.py`` proves on the CPU that this rejects a 1e-3 relative error in one 32 x 32 tile.
"""
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from layer_rows import FACTOR, FLOOR, TILE
from oracle.vap_oracle import DIM, HEADS, VapOracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn20.npz")   # tools/make_golden_attn.py
ROW_SUM_TOL = 1e-5
KINDS = ("attn", "self_attn", "cross_attn")


def layer_name(kind: str, l: int) -> str:
    return "ar_channel.layers.0" if kind == "attn" else f"ar.layers.{l}"


def golden_context(z, n):
    """The seeded context tensor [1, 2, n, 256] of a golden case, checked against its stored fingerprint."""
    x = np.random.default_rng(int(z[f"n{n}.seed"])).standard_normal((1, 2, n, 256)).astype(np.float32) * np.float32(float(z["meta.scale"]))
    fp = np.array([x.astype(np.float64).sum(), np.abs(x.astype(np.float64)).sum()])
    assert np.allclose(fp, z[f"n{n}.x_fp"], rtol=0, atol=1e-9), "seeded context differs from the golden's"
    return x


def golden_weights(z):
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(int(z["meta.seed"]), int(z["meta.frame_hz"]), str(z["meta.mode"]))
    assert np.array_equal(W.weights_fingerprint(cpc, vap), z["meta.weights_fp"]), "seeded weights differ from the golden's"
    return cpc, vap


class RecordingOracle(VapOracle):
    """VapOracle whose ``_mha`` also appends ``att`` [B, 4, n, n] to ``self.recorded`` (when it is a list)."""

    recorded: Optional[list] = None

    def _mha(self, pre: str, q_in: torch.Tensor, kv_in: torch.Tensor) -> torch.Tensor:
        v = self.v
        B, n, _ = q_in.shape
        q = (q_in @ v[f"{pre}.query.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
        k = (kv_in @ v[f"{pre}.key.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
        val = (kv_in @ v[f"{pre}.value.weight"].T).view(B, n, HEADS, 64).transpose(1, 2)
        att = torch.einsum("bhid,bhjd->bhij", q, k) * (1.0 / math.sqrt(DIM))
        m = v[f"{pre}.m"].view(1, HEADS, 1, 1)
        j = torch.arange(n, dtype=self.dtype).view(1, 1, 1, n)
        # the reference's mask is tril(ones) with -inf above the diagonal (modules.py:179-186): the kept scores carry a + 1 that the
        # softmax cancels but fp32 rounding does not, so it is restated here (VapOracle adds 0 there)
        causal = torch.ones(n, n, dtype=self.dtype).tril()
        causal = causal.masked_fill(causal == 0, float("-inf"))
        att = (att + (m * j + causal)).softmax(dim=-1)
        if self.recorded is not None:
            self.recorded.append(att)
        y = (att @ val).transpose(1, 2).reshape(B, n, DIM)
        return y @ v[f"{pre}.proj.weight"].T

    def _stereo_maps(self, rec) -> Dict[str, np.ndarray]:
        """12 recorded maps of the three stereo layers (a-self, a-cross, b-self, b-cross per layer) -> [S, 2, 3, 4, n, n] each."""
        assert len(rec) == 12, len(rec)
        self_attn = torch.stack([torch.stack([rec[4 * l + 2 * c] for l in range(3)], 1) for c in range(2)], 1)
        cross_attn = torch.stack([torch.stack([rec[4 * l + 2 * c + 1] for l in range(3)], 1) for c in range(2)], 1)
        return {"self_attn": self_attn.numpy(), "cross_attn": cross_attn.numpy()}

    def maps(self, x) -> Dict[str, np.ndarray]:
        """x [S, 2, n, 256]: ar_channel on both channels, then ar on its outputs (the engine's stage 0).  Returns the three map
        arrays ``attn`` [S, 2, 1, 4, n, n], ``self_attn`` / ``cross_attn`` [S, 2, 3, 4, n, n] next to the rows ``o`` [S, 2, n, 256],
        ``x12`` [S, 2, n, 256] and ``comb`` [S, n, 256]."""
        x = torch.as_tensor(np.asarray(x)).to(self.dtype)
        self.recorded = []
        try:
            with torch.no_grad():
                o1, o2, a, b, h = self.transformer(x[:, 0], x[:, 1])
            rec = self.recorded
        finally:
            self.recorded = None
        assert len(rec) == 14, len(rec)
        out = {"attn": torch.stack([rec[0], rec[1]], 1)[:, :, None].numpy(), **self._stereo_maps(rec[2:])}
        out.update(o=torch.stack([o1, o2], 1).numpy(), x12=torch.stack([a, b], 1).numpy(), comb=h.numpy())
        return out

    def stereo_maps(self, o) -> Dict[str, np.ndarray]:
        """o [S, 2, n, 256] taken as the ar_channel outputs: ar alone (GPTStereo.forward, modules.py:395-423; the engine's stage 2)."""
        o = torch.as_tensor(np.asarray(o)).to(self.dtype)
        v = self.v
        self.recorded = []
        try:
            with torch.no_grad():
                a, b = o[:, 0], o[:, 1]
                for l in range(3):
                    a, b = self.layer(f"ar.layers.{l}", a, b), self.layer(f"ar.layers.{l}", b, a)
                ha = torch.nn.functional.gelu(self._ln(a @ v["ar.combinator.h0_a.weight"].T, "ar.combinator.ln"))
                hb = torch.nn.functional.gelu(self._ln(b @ v["ar.combinator.h0_b.weight"].T, "ar.combinator.ln"))
            rec = self.recorded
        finally:
            self.recorded = None
        out = self._stereo_maps(rec)
        out.update(x12=torch.stack([a, b], 1).numpy(), comb=(ha + hb).numpy())
        return out


def check_maps(kind: str, got: np.ndarray, want64: np.ndarray, want32: np.ndarray, rows: Optional[Sequence[int]] = None,
               streams: Optional[Sequence] = None, what: str = "") -> float:
    """Check one map array.  ``got`` / ``want64`` / ``want32``: [B, 2, layers, 4, R, n] — every query row (R = n) or the rows
    ``rows``.  Returns the worst err / E32 over the maps.  Fails on the first map with a non-finite row, a non-zero above the
    diagonal, a row that does not sum to 1 within ROW_SUM_TOL, or an entry beyond the bound, naming stream, channel, layer, kind,
    head, row and key tile."""
    assert kind in KINDS, kind
    got = np.asarray(got)
    w64 = np.asarray(want64, dtype=np.float64)
    w32 = np.asarray(want32).astype(np.float64)
    assert got.shape == w64.shape == w32.shape and got.ndim == 6, (kind, got.shape, w64.shape, w32.shape)
    B, C, L, H, R, n = got.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    assert rows.shape == (R,), (rows.shape, R)
    streams = list(range(B)) if streams is None else list(streams)
    g = got.astype(np.float64)
    above = np.arange(n)[None, :] > rows[:, None]                  # [R, n]: keys above the diagonal
    worst = 0.0
    for b in range(B):
        for c in range(C):
            for l in range(L):
                for h in range(H):
                    m, t64 = g[b, c, l, h], w64[b, c, l, h]
                    where = f"{what} stream {streams[b]} channel {c} {layer_name(kind, l)} {kind} head {h}"
                    err = np.abs(m - t64)

                    def at(r):
                        e = np.where(np.isfinite(err[r]), err[r], np.inf)
                        return f"row {rows[r]} (key tile {int(np.argmax(e)) // TILE}), n = {n}"
                    fin = np.isfinite(m).all(axis=1)
                    if not fin.all():
                        raise AssertionError(f"{where}: non-finite value in {at(int(np.flatnonzero(~fin)[0]))}")
                    nz = ((got[b, c, l, h] != 0) & above).any(axis=1)
                    if nz.any():
                        r = int(np.flatnonzero(nz)[0])
                        k = int(np.flatnonzero((got[b, c, l, h, r] != 0) & above[r])[0])
                        raise AssertionError(f"{where}: key {k} above the diagonal is {got[b, c, l, h, r, k]!r}, not 0, in row {rows[r]} "
                                             f"(key tile {k // TILE}), n = {n}")
                    e32 = float(np.abs(w32[b, c, l, h] - t64).max())
                    bound = FACTOR * max(e32, FLOOR)
                    bad = err.max(axis=1) > bound
                    if bad.any():
                        r = int(np.flatnonzero(bad)[0])
                        raise AssertionError(f"{where}: off by {err[r].max():.3e} > bound {bound:.3e} (E32 {e32:.3e}, worst "
                                             f"{err.max():.3e}) in {at(r)}")
                    dev = np.abs(m.sum(axis=1) - 1.0)
                    if (dev > ROW_SUM_TOL).any():
                        r = int(np.flatnonzero(dev > ROW_SUM_TOL)[0])
                        raise AssertionError(f"{where}: sums to 1 {m[r].sum() - 1.0:+.3e} (> {ROW_SUM_TOL:.0e}) in {at(r)}")
                    worst = max(worst, float(err.max()) / max(e32, 1e-30))
    return worst
