#!/usr/bin/env python3
"""Golden attention maps from the UNMODIFIED reference (imported from /root/reference), as tools/make_golden.py does for the step.

Runs only where /root/reference exists.  Nothing of the reference is copied: the script writes seeded synthetic checkpoints
(``weights.synthetic_weights``, 20 Hz, mode ``vap``) to a temp dir, builds the reference's own ``VAPRealTime``
(rvap/vap_main/vap_main.py:185-247) and calls its model the way a user who wants the maps does:

    vap.ar_channel(x_c, attention=True)          -> "x", "attn"        [1, 1, 4, n, n]          (modules.py:356-372)
    vap.ar(o1, o2, attention=True)               -> "self_attn", "cross_attn"  [1, 2, 3, 4, n, n]   (modules.py:395-423)

on seeded context tensors ``default_rng(seed).standard_normal((1, 2, n, 256)).astype(float32) * 0.7``.  ``tests/golden/attn20.npz``
stores the seeds, the inputs' fingerprint and the maps: every row for n = 33, rows ROWS_100 only for n = 100.

Usage:  python tools/make_golden_attn.py [output.npz]
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, REPO)

WEIGHT_SEED, FRAME_HZ, MODE = 31, 20, "vap"
CASES = {33: 1033, 100: 1100}            # n: input seed
ROWS_100 = [0, 32, 64, 96, 99]
SCALE = 0.7


def context(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((1, 2, n, 256)).astype(np.float32) * np.float32(SCALE)


def fingerprint(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    return np.array([x.sum(), np.abs(x).sum()])


def main(path: str) -> None:
    import torch
    from vap_realtime_amd import weights as W

    sys.path[:0] = [REF, os.path.join(REF, "rvap", "vap_main")]
    import vap_main as ref

    cpc_sd, vap_sd = W.synthetic_weights(WEIGHT_SEED, FRAME_HZ, MODE)
    tmp = tempfile.mkdtemp(prefix="vapgold_")
    cpc_pt, vap_pt = os.path.join(tmp, "cpc.pt"), os.path.join(tmp, "vap.pt")
    torch.save({"weights": {k: torch.from_numpy(v.copy()) for k, v in cpc_sd.items()}}, cpc_pt)
    torch.save({k: torch.from_numpy(v.copy()) for k, v in vap_sd.items()}, vap_pt)
    with contextlib.redirect_stdout(io.StringIO()):
        rt = ref.VAPRealTime(vap_pt, cpc_pt, torch.device("cpu"), FRAME_HZ, 2.5)
    vap = rt.vap

    out = {"meta.mode": np.array(MODE), "meta.frame_hz": np.array(FRAME_HZ), "meta.seed": np.array(WEIGHT_SEED),
           "meta.weights_fp": W.weights_fingerprint(cpc_sd, vap_sd), "meta.cases": np.array(sorted(CASES), np.int64),
           "meta.scale": np.array(SCALE)}
    for n, seed in CASES.items():
        x = context(seed, n)
        rows = list(range(n)) if n == 33 else ROWS_100
        with torch.no_grad():
            ch = [vap.ar_channel(torch.from_numpy(x[:, c]), attention=True) for c in range(2)]
            st = vap.ar(ch[0]["x"], ch[1]["x"], attention=True)
        attn = torch.stack([ch[0]["attn"], ch[1]["attn"]], dim=1).numpy()          # [1, 2, 1, 4, n, n]
        assert attn.shape == (1, 2, 1, 4, n, n) and st["self_attn"].shape == (1, 2, 3, 4, n, n) == st["cross_attn"].shape
        out[f"n{n}.seed"] = np.array(seed)
        out[f"n{n}.x_fp"] = fingerprint(x)
        out[f"n{n}.rows"] = np.array(rows, np.int32)
        out[f"n{n}.attn"] = attn[..., rows, :].astype(np.float32)
        out[f"n{n}.self_attn"] = st["self_attn"].numpy()[..., rows, :].astype(np.float32)
        out[f"n{n}.cross_attn"] = st["cross_attn"].numpy()[..., rows, :].astype(np.float32)
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} B)")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "attn20.npz"))
