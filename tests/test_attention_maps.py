"""CPU half of the attention-map tests: the recording oracle of tests/attention_maps_ref.py reproduces the maps the unmodified
reference returned (tests/golden/attn20.npz, tools/make_golden_attn.py), and ``check_maps`` has detection power: it accepts the
fp32 oracle against the float64 oracle and rejects a 1e-3 relative error in one 32 x 32 tile of one map (for an early, a middle
and the last query tile, the key tile that holds most of those rows' weight), for self and cross
attention, the first and the last stereo layer, and one window of each attention dispatch class (n = 33, 100, 300).  A looser
``layer_rows.FACTOR`` fails here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from attention_maps_ref import GOLDEN, KINDS, RecordingOracle, check_maps, golden_context, golden_weights, layer_name
from layer_rows import TILE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
REL = 1e-3


def test_recording_oracle_reproduces_the_reference_maps():
    z = np.load(GOLDEN)
    cpc, vap = golden_weights(z)
    o32 = RecordingOracle(cpc, vap, int(z["meta.frame_hz"]), 5.0)
    assert [int(n) for n in z["meta.cases"]] == [33, 100]
    assert [int(r) for r in z["n33.rows"]] == list(range(33)) and [int(r) for r in z["n100.rows"]] == [0, 32, 64, 96, 99]
    for n in (33, 100):
        got = o32.maps(golden_context(z, n))
        rows = z[f"n{n}.rows"]
        for kind in KINDS:
            want = z[f"n{n}.{kind}"]
            assert want.shape == (1, 2, 1 if kind == "attn" else 3, 4, len(rows), n)
            err = float(np.abs(got[kind][..., rows, :] - want).max())
            assert err <= 1e-6, (n, kind, err)


@pytest.fixture(scope="module")
def oracles():
    import torch
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(23, 20, "vap")
    return RecordingOracle(cpc, vap, 20, 15.0, dtype=torch.float64), RecordingOracle(cpc, vap, 20, 15.0)


@pytest.mark.parametrize("n", [33, 100, 300])
def test_check_maps_accepts_fp32_and_rejects_a_one_tile_error(oracles, n):
    o64, o32 = oracles
    x = np.random.default_rng(700 + n).standard_normal((1, 2, n, 256)).astype(np.float32) * np.float32(0.7)
    ref64, ref32 = o64.maps(x), o32.maps(x)
    for kind in KINDS:
        ratio = check_maps(kind, ref32[kind].astype(np.float32), ref64[kind], ref32[kind], what=f"n={n} fp32 oracle")
        assert ratio <= 1.0 + 1e-9
    last = (n - 1) // TILE
    for kind in ("self_attn", "cross_attn"):
        for layer in (0, 2):
            # an early, a middle and the last query tile; in each the key tile that holds most of its rows' weight (cross-attention of a
            # late layer is not diagonal: some tiles hold weights of 1e-7 and below, where a relative error of 1e-3 is below every
            # absolute bound and below what fp32 resolves in the row sum)
            for channel, head, qt in ((0, 0, 0), (1, 3, last // 2), (1, 1, last), (0, 2, last)):
                q = slice(qt * TILE, (qt + 1) * TILE)
                mass = [ref64[kind][0, channel, layer, head, q, kt * TILE:(kt + 1) * TILE].sum(axis=1).max() for kt in range(qt + 1)]
                kt = int(np.argmax(mass))
                bad = ref64[kind].copy()
                bad[0, channel, layer, head, q, kt * TILE:(kt + 1) * TILE] *= 1.0 + REL
                with pytest.raises(AssertionError) as e:
                    check_maps(kind, bad, ref64[kind], ref32[kind], what=f"n={n}")
                msg = str(e.value)
                assert f"channel {channel} {layer_name(kind, layer)} {kind} head {head}" in msg and f"(key tile {kt})" in msg, msg
                assert int(msg.split(" row ")[1].split()[0]) // TILE == qt, msg
    # the other properties, one each: a weight above the diagonal, a NaN
    bad = ref64["attn"].astype(np.float32)
    bad[0, 1, 0, 2, 0, n - 1] = 1e-30
    with pytest.raises(AssertionError, match="above the diagonal"):
        check_maps("attn", bad, ref64["attn"], ref32["attn"])
    bad = ref64["attn"].astype(np.float32)
    bad[0, 0, 0, 1, n - 1, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_maps("attn", bad, ref64["attn"], ref32["attn"])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference checkout is not on this machine")
def test_golden_regenerates_from_the_reference(tmp_path):
    """tools/make_golden_attn.py on the unmodified reference writes the committed file again, array for array: seeds, fingerprints and
    row lists exactly, the maps within 1e-6 (the reference's fp32 BLAS may pick another summation order on another CPU)."""
    out = str(tmp_path / "attn20.npz")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_golden_attn.py"), out], stdout=subprocess.DEVNULL)
    new, old = np.load(out), np.load(GOLDEN)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].shape == old[k].shape and new[k].dtype == old[k].dtype, k
        if old[k].dtype == np.float32:
            assert float(np.abs(new[k] - old[k]).max()) <= 1e-6, k
        else:
            assert np.array_equal(new[k], old[k]), k
