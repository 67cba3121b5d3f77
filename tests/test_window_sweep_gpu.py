"""Every window fill and ring rotation of the HIP path against the float64 oracle, from T = 1: one ragged batch per window size.

tests/window_sweep.py puts one stream per state (n, rot) into a batch - for T <= 64 every fill n = 1 .. T and every rotation 0 .. T - 1,
for longer windows every edge of every 32-key tile, one interior fill per valid-tile count and the rotations around 0, 32, 64, T - 64,
T - 32 and T - 1 - and checks the final tick once: every valid row of ``o``, ``stereo0``, ``stereo1`` (``stereo2`` where the variant
materialises it) with ``layer_rows.check_rows``, and ``last`` (last_block_kernel) where the last layer runs on the newest row alone.
The truth is both oracles' ``layers`` on the window the engine itself exports, after the export has been anchored bit for bit to the
injected rows and to ``peek("e")``; the bound is 8 x max(E32, 1e-6 max|x|) per stream, E32 not pooled.

All cases run at 50 Hz (the kernels under test do not see the frame rate).  Variants, poison and the forced XL kernel are those of
tests/test_layer_rows_gpu.py.

    short  T in 1 .. 64     attn_block_kernel + ffn_block mode 0: fp32 and split (both poisoned) + fp32_full / split_full alternating
    long   T in 65 .. 256   attention_long2 / f16x3 / proj_f16x3 + the mode-1 flat-row blocks: the four base variants, T = 250 the
                            unfused projections and split_qkv_in_ffn, T = 65 / 256 the forced XL kernel
    XL     T in 257 .. 512  attention_xl_kernel, fp32 (the split path uses the same kernel there)

Each case prints the worst err / E32 per variant and buffer and the state that gave it (run with -s).  Measured on the MI355X, the
worst over the fp32 variants (left) and over the split variants (right) of each case; the bound is 8 (``last``: the tick's pooled
E32, as tests/head_stages.py defines that check; "worst at": the state of the largest figure of the row).  No case needed a pooled
E32; the largest figure is 6.90 (stereo0, fp32, T = 289).  The slowest case takes 9.1 s (T = 512: 81 streams, 511 ticks, two engines,
7 s of it the two oracles on the CPU); the whole module 60 s.

                 | fp32, fp32_full, fp32_force_xl, unfused_proj              | split, split_full, split_unfused_proj, split_qkv_in_ffn   |
       T streams |       o stereo0 stereo1 stereo2    last  worst at (n, rot) |       o stereo0 stereo1 stereo2    last  worst at (n, rot) | case s
       1       1 |    1.84    2.03    1.81    2.00    1.91  (1, 0)            |    0.96    1.18    1.20       -    1.42  (1, 0)            | 0.3
       2       3 |    1.84    2.03    1.81       -    1.43  (1, 0)            |    1.06    1.28    1.20    1.42    1.28  (1, 0)            | 0.0
       3       5 |    2.45    2.80    2.06    2.15    1.77  (2, 0)            |    1.47    1.35    1.42       -    1.10  (3, 1)            | 0.1
       4       7 |    2.22    2.80    2.53       -    1.57  (2, 0)            |    1.41    1.75    1.77    2.00    1.41  (3, 0)            | 0.1
       5       9 |    2.24    2.80    2.16    2.31    1.64  (2, 0)            |    1.41    1.40    1.57       -    1.47  (3, 0)            | 0.1
       7      13 |    2.33    2.80    2.22       -    1.54  (2, 0)            |    1.68    1.90    1.65    1.80    1.48  (3, 0)            | 0.1
       8      15 |    2.22    2.80    2.67    2.67    1.62  (2, 0)            |    1.64    1.52    1.46       -    1.54  (6, 0)            | 0.2
      16      31 |    2.40    2.80    2.07       -    1.36  (2, 0)            |    1.62    1.57    1.59    1.58    1.43  (16, 3)           | 0.4
      20      39 |    2.27    2.80    2.67    2.34    1.89  (2, 0)            |    1.60    1.68    1.51       -    1.61  (4, 0)            | 0.5
      31      61 |    2.39    2.85    2.50       -    1.31  (31, 25)          |    1.77    1.60    1.83    1.52    1.00  (21, 0)           | 0.9
      32      63 |    2.39    2.80    2.67    2.69    2.01  (2, 0)            |    2.27    1.75    1.60       -    1.51  (29, 0)           | 0.9
      33      65 |    2.40    2.80    2.67       -    1.54  (2, 0)            |    1.70    1.76    1.64    1.53    1.13  (7, 0)            | 0.9
      36      71 |    2.45    3.14    2.50    2.65    1.76  (36, 11)          |    1.63    1.68    1.83       -    1.11  (36, 17)          | 1.1
      37      73 |    3.00    2.80    2.41       -    1.53  (37, 35)          |    2.02    1.92    1.81    1.63    1.09  (30, 0)           | 1.1
      48      95 |    2.62    2.80    2.46    2.91    1.63  (48, 13)          |    2.33    1.79    1.81       -    1.52  (19, 0)           | 1.6
      49      97 |    2.44    2.80    2.50       -    1.62  (2, 0)            |    1.71    1.76    1.74    1.68    1.35  (5, 0)            | 1.6
      52     103 |    2.59    2.80    2.51    2.45    0.90  (2, 0)            |    1.79    1.73    1.76       -    0.96  (25, 0)           | 1.9
      53     105 |    2.76    2.80    2.56       -    2.02  (2, 0)            |    1.78    1.97    1.62    1.65    1.41  (53, 39)          | 1.9
      63     125 |    2.81    2.80    2.41    2.82    1.58  (44, 0)           |    1.73    1.88    1.83       -    1.47  (59, 0)           | 2.6
      64     127 |    3.42    3.30    2.69       -    1.75  (64, 55)          |    1.77    1.73    1.86    1.65    1.41  (12, 0)           | 2.5
      65      18 |    5.04    6.68    5.31    4.89    2.56  (65, 1)           |    2.96    3.48    2.78    3.09    1.65  (65, 1)           | 0.7
      97      26 |    5.04    5.51    5.31    5.09    2.96  (95, 0)           |    2.58    3.92    2.72    2.88    1.72  (97, 64)          | 1.0
     129      32 |    5.04    6.28    5.31    4.78    3.49  (77, 0)           |    2.72    3.58    3.14    3.69    1.78  (129, 98)         | 1.5
     160      37 |    5.04    6.10    5.31    5.14    2.32  (160, 128)        |    2.86    4.09    3.14    3.38    2.18  (160, 32)         | 2.0
     193      42 |    5.04    5.49    5.31    6.32    3.18  (193, 31)         |    2.56    3.94    3.45    3.32    2.19  (141, 0)          | 2.7
     250      49 |    5.04    5.94    5.31    5.56    2.43  (250, 218)        |    2.64    3.73    3.31    3.97    1.81  (109, 0)          | 5.4
     256      49 |    5.04    5.70    5.31    5.58    2.78  (173, 0)          |    2.80    4.09    3.09    3.97    1.75  (256, 65)         | 4.8
     257      50 |    5.04    6.61    5.31    5.37    2.41  (223, 0)          |       -       -       -       -       -  -                 | 2.6
     289      54 |    5.04    6.90    5.31    5.92    2.69  (289, 225)        |       -       -       -       -       -  -                 | 3.2
     385      66 |    5.04    6.22    5.31    5.61    2.38  (65, 0)           |       -       -       -       -       -  -                 | 5.7
     512      81 |    5.04    6.34    5.31    5.63    2.89  (447, 0)          |       -       -       -       -       -  -                 | 9.1
"""
import hashlib
import time

import pytest

import window_sweep as ws
from test_layer_rows_gpu import Variant, base_variants, make_engine

pytestmark = pytest.mark.gpu

HZ = 50
SHORT, LONG, XL = ws.SHORT, ws.LONG, ws.XL


@pytest.fixture(scope="module")
def rig():
    """Weights, blob, both oracles (``layers`` does not depend on the window size) and the donor sequence of the longest window."""
    import torch
    from oracle.vap_oracle import VapOracle
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(23, HZ, "vap")
    return {"blob": W.pack_blob(cpc, vap, "vap"), "o64": VapOracle(cpc, vap, HZ, 1.0, dtype=torch.float64), "o32": VapOracle(cpc, vap, HZ, 1.0),
            "donor": ws.donor(cpc, vap, HZ, max(XL) + ws.DONOR_EXTRA)}


def run_case(rig, T, variants):
    t0 = time.time()
    ctx = (T + 0.5) / HZ
    prog = ws.schedule(ws.plan(T), T)
    inject = ws.injected_rows(prog, T, rig["donor"])
    audio = ws.step_audio(prog, HZ)
    truths = {}                                               # exported windows (bytes) -> Truth: engines with bit-equal encoders share one
    for v in variants:
        eng = make_engine(rig["blob"], HZ, ctx, prog.max_streams, v, "vap")
        try:
            assert eng.T == T, (ctx, eng.T, T)
            pruned = "stereo2" not in v.buffers("vap")
            cap = ws.drive(eng, T, prog, inject, audio, HZ, v.buffers("vap"), pruned, what=v.label)
        finally:
            eng.close()
        key = hashlib.sha1(b"".join(w.tobytes() for w in cap.windows)).digest()
        if key not in truths:
            truths[key] = ws.truth(rig["o64"], rig["o32"], cap)
        at: dict = {}
        worst = ws.check(cap, truths[key], v.buffers("vap"), T, what=v.label, path="fused_split" if v.kw.get("split_f16") else "fused", at=at)
        print(f"\nsweep T={T} {v.label}: {len(prog.states)} streams, worst err/E32", {b: round(r, 2) for b, r in worst.items()},
              "at (n, rot)", at)
    print(f"sweep T={T}: {time.time() - t0:.1f} s, {len(truths)} distinct exported windows")


@pytest.mark.parametrize("T", SHORT)
def test_short_window_sweep(rig, T):
    """T = 1 .. 64: every fill and every rotation; both edges of the 32 + 5 x 4 row tiling (32 < T <= 52), n > 32, and every window smaller
    than a flat-row tile (at T = 1 a 32-row tile holds 16 (stream, channel) windows)."""
    full = (Variant("fp32_full", full_last_layer=True) if SHORT.index(T) % 2 == 0 else
            Variant("split_full", split_f16=True, full_last_layer=True))
    run_case(rig, T, [Variant("fp32", poison=True), Variant("split", poison=True, split_f16=True), full])


@pytest.mark.parametrize("T", LONG)
def test_long_window_sweep(rig, T):
    """T = 65 .. 256: valid-tile counts 1 .. 8 with one-row last tiles and full tiles, wave w's query tiles w and 7 - w at every count."""
    run_case(rig, T, base_variants(T))


@pytest.mark.parametrize("T", XL)
def test_xl_window_sweep(rig, T):
    """T = 257 .. 512: attention_xl_kernel at valid-tile counts 1 .. 16, fills 288 .. 480 included."""
    run_case(rig, T, [Variant("fp32", poison=True), Variant("fp32_full", full_last_layer=True)])
