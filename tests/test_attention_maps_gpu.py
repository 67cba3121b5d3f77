"""Attention maps of the HIP path (vapx_transformer_maps, csrc/attention_map.hip) against the reference's and the float64 oracle's.

Engines run at 20 Hz with windows of 50, 100 and 300 frames: the three attention dispatch classes (attn_block, attention_long2 /
attention_f16x3, attention_xl), next to whose launches the map kernel is enqueued.

  (a) goldens     the maps the unmodified reference returned (tests/golden/attn20.npz) through ``VapGPT.ar_channel_with_attention`` and
                  ``ar_with_attention``, 1e-4 absolute (the project's parity bar)
  (b) row sweep   rows 1, 2, 31, 32, 33, 50 | 33, 64, 65, 100 | 257, 300 with a batch of 3 (2 for the longest window), stages 0, 1, 2,
                  every map under ``attention_maps_ref.check_maps`` against the float64 oracle; the destination buffers are NaN-filled
                  and carry a tail that must stay untouched
  (c) outputs     o / x12 / comb of a maps call are bit-identical to vapx_transformer's on the same input (fp32 engine)
  (d) split path  VAPX_FLAG_SPLIT_F16 engines (T = 100 changes its Q|K|V routing for a maps call): maps under check_maps, rows under
                  ``layer_rows.row_bound``
  (e) arguments   a map pointer for a stage that does not run is refused; all-NULL maps are vapx_transformer
  (f) state       a maps call between two steps changes no bit of the following steps' outputs
"""
import numpy as np
import pytest

from attention_maps_ref import GOLDEN, KINDS, RecordingOracle, check_maps, golden_context, golden_weights
from layer_rows import row_bound

pytestmark = pytest.mark.gpu

HZ = 20
WINDOWS = {50: 2.5, 100: 5.0, 300: 15.0}          # T: context seconds
SWEEP = [(50, r) for r in (1, 2, 31, 32, 33, 50)] + [(100, r) for r in (33, 64, 65, 100)] + [(300, r) for r in (257, 300)]
SEED = 23
TAIL = 4096                                        # floats behind every map buffer that no kernel may touch


@pytest.fixture(scope="module")
def model():
    """Seeded weights, their blob, and the float64 / fp32 recording oracles."""
    import torch
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(SEED, HZ, "vap")
    return {"blob": W.pack_blob(cpc, vap, "vap"), "cpc": cpc, "vap": vap,
            "o64": RecordingOracle(cpc, vap, HZ, 15.0, dtype=torch.float64), "o32": RecordingOracle(cpc, vap, HZ, 15.0)}


@pytest.fixture(scope="module")
def engines(model):
    """Engines by (T, split), built on first use, closed with the module."""
    from vap_realtime_amd import engine
    made = {}

    def get(T, split=False):
        if (T, split) not in made:
            made[(T, split)] = engine.Engine(model["blob"], HZ, WINDOWS[T], max_streams=3, split_f16=split)
            assert made[(T, split)].T == T
        return made[(T, split)]
    yield get
    for e in made.values():
        e.close()


def context(n, batch, seed=0):
    return np.random.default_rng(1000 * seed + 10 * n + batch).standard_normal((batch, 2, n, 256)).astype(np.float32) * np.float32(0.7)


def run(eng, x, stage, maps=True, via_maps_call=True):
    """One stage call on x [B, 2, n, 256]: every output the stage has, as numpy arrays; the map buffers start as NaN and their
    tails must come back untouched."""
    import torch
    B, _, n, _ = x.shape
    dev = torch.device("cuda")
    dx = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t = {}
    if stage != 2:
        t["o"] = torch.full((B, 2, n, 256), float("nan"), device=dev)
    if stage != 1:
        t["x12"] = torch.full((B, 2, n, 256), float("nan"), device=dev)
        t["comb"] = torch.full((B, n, 256), float("nan"), device=dev)
    shapes = {}
    if maps and stage != 2:
        shapes["attn"] = (B, 2, 1, 4, n, n)
    if maps and stage != 1:
        shapes["self_attn"] = shapes["cross_attn"] = (B, 2, 3, 4, n, n)
    flat = {k: torch.full((int(np.prod(s)) + TAIL,), float("nan"), device=dev) for k, s in shapes.items()}
    ptr = lambda d, k: d[k].data_ptr() if k in d else 0
    if via_maps_call:
        eng.transformer_maps_device(B, n, dx.data_ptr(), o_ptr=ptr(t, "o"), x12_ptr=ptr(t, "x12"), comb_ptr=ptr(t, "comb"), stage=stage,
                                    attn_ptr=ptr(flat, "attn"), self_attn_ptr=ptr(flat, "self_attn"), cross_attn_ptr=ptr(flat, "cross_attn"))
    else:
        assert not maps
        eng.transformer_device(B, n, dx.data_ptr(), o_ptr=ptr(t, "o"), x12_ptr=ptr(t, "x12"), comb_ptr=ptr(t, "comb"), stage=stage)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in t.items()}
    for k, s in shapes.items():
        f = flat[k].cpu().numpy()
        assert np.isnan(f[-TAIL:]).all(), f"{k}: the kernel wrote behind the [n][n] maps (n = {n}, batch {B})"
        out[k] = f[:-TAIL].reshape(s)
    return out


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ctx", [(33, 2.5), (100, 5.0)], ids=["n33_T50", "n100_T100"])
def test_maps_match_the_reference_goldens(n, ctx):
    import torch
    from vap_realtime_amd.realtime import VapGPT
    z = np.load(GOLDEN)
    cpc, vap = golden_weights(z)
    m = VapGPT.from_state_dicts(cpc, vap, frame_rate=int(z["meta.frame_hz"]), context_len_sec=ctx, max_batch=2)
    assert m.engine.T == int(ctx * HZ)
    x = torch.from_numpy(golden_context(z, n))
    rows = z[f"n{n}.rows"]
    both = m.ar_channel_with_attention(x[0])                                   # the two channels as a batch of two
    assert tuple(both["x"].shape) == (2, n, 256) and tuple(both["attn"].shape) == (2, 1, 4, n, n)
    err = float(np.abs(both["attn"].cpu().numpy()[..., rows, :] - z[f"n{n}.attn"][0]).max())
    print(f"n={n} attn: max |hip - reference| = {err:.2e}")
    assert err <= 1e-4
    assert torch.equal(both["x"], m.ar_channel(x[0])["x"])
    for c in range(2):                                                         # an odd batch rides with one padding slot
        one = m.ar_channel_with_attention(x[:, c])
        assert tuple(one["attn"].shape) == (1, 1, 4, n, n)
        assert torch.equal(one["attn"][0], both["attn"][c]) and torch.equal(one["x"][0], both["x"][c])
    st = m.ar_with_attention(both["x"][0:1], both["x"][1:2])
    assert set(st) == {"x", "x1", "x2", "self_attn", "cross_attn"}
    plain = m.ar(both["x"][0:1], both["x"][1:2])
    for k in ("x", "x1", "x2"):
        assert torch.equal(st[k], plain[k]), k
    for kind in ("self_attn", "cross_attn"):
        assert tuple(st[kind].shape) == (1, 2, 3, 4, n, n)
        err = float(np.abs(st[kind].cpu().numpy()[..., rows, :] - z[f"n{n}.{kind}"]).max())
        print(f"n={n} {kind}: max |hip - reference| = {err:.2e}")
        assert err <= 1e-4, kind
    for call in (lambda: m.ar_channel(x[0], attention=True), lambda: m.ar(x[:, 0], x[:, 1], attention=True)):
        with pytest.raises(NotImplementedError, match="with_attention"):
            call()
    m.engine.close()


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
def check_stage(eng, model, x, stage, what):
    """Run one stage with maps and check every map it has; returns (outputs, float64 reference, fp32 reference)."""
    ref = (lambda o: o.stereo_maps(x)) if stage == 2 else (lambda o: o.maps(x))
    r64, r32 = ref(model["o64"]), ref(model["o32"])
    got = run(eng, x, stage)
    kinds = [k for k in KINDS if k in got]
    assert kinds == {0: list(KINDS), 1: ["attn"], 2: ["self_attn", "cross_attn"]}[stage]
    worst = {k: round(check_maps(k, got[k], r64[k], r32[k], what=f"{what} stage {stage}"), 2) for k in kinds}
    print(f"{what} stage {stage}: worst err/E32", worst)
    return got, r64, r32


@pytest.mark.parametrize("T,rows", SWEEP, ids=[f"T{t}_n{r}" for t, r in SWEEP])
def test_map_rows_against_float64(engines, model, T, rows):
    batch = 2 if T == 300 else 3
    eng = engines(T)
    for stage in (0, 1, 2):
        check_stage(eng, model, context(rows, batch, seed=stage), stage, f"T={T} n={rows} fp32")


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,rows", [(50, 33), (100, 65), (300, 257)], ids=["T50", "T100", "T300"])
def test_outputs_are_bit_identical_with_and_without_maps(engines, T, rows):
    eng = engines(T)
    x = context(rows, 2, seed=7)
    for stage in (0, 1, 2):
        plain = run(eng, x, stage, maps=False, via_maps_call=False)
        nullm = run(eng, x, stage, maps=False)                  # (e) all-NULL maps: vapx_transformer itself
        withm = run(eng, x, stage)
        for k in plain:
            assert np.isfinite(plain[k]).all(), (stage, k)
            assert np.array_equal(plain[k], nullm[k]), (stage, k)
            assert np.array_equal(plain[k], withm[k]), (stage, k)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,rows", [(50, 33), (50, 50), (100, 65), (100, 100)], ids=["T50_n33", "T50_n50", "T100_n65", "T100_n100"])
def test_split_path_maps_and_rows(engines, model, T, rows):
    eng = engines(T, split=True)
    x = context(rows, 3, seed=11)
    got, r64, r32 = check_stage(eng, model, x, 0, f"T={T} n={rows} split")
    # the maps call takes the routing VAPX_FLAG_SPLIT_QKV_IN_FFN selects (Q|K|V through HBM); a plain call on the same handle afterwards is
    # back on the default routing: both hold the same bound
    plain = run(eng, x, 0, maps=False, via_maps_call=False)
    for call, res in (("maps", got), ("plain", plain)):
        for k in ("o", "x12", "comb"):
            for b in range(x.shape[0]):
                bound, e32 = row_bound(r64[k][b], r32[k][b])
                err = float(np.abs(res[k][b].astype(np.float64) - r64[k][b]).max())
                print(f"T={T} n={rows} split {call} call, {k} stream {b}: err {err:.3e} bound {bound:.3e} (E32 {e32:.3e})")
                assert np.isfinite(res[k][b]).all() and err <= bound, (call, k, b, err, bound)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------
def test_a_map_for_a_stage_that_does_not_run_is_refused(engines):
    import torch
    from vap_realtime_amd.engine import VapxError
    eng = engines(50)
    n = 8
    dev = torch.device("cuda")
    x = torch.zeros(1, 2, n, 256, device=dev)
    buf = torch.zeros(2 * 3 * 4 * n * n, device=dev)
    with pytest.raises(VapxError, match="stage 2"):
        eng.transformer_maps_device(1, n, x.data_ptr(), stage=2, attn_ptr=buf.data_ptr())
    for kw in ({"self_attn_ptr": buf.data_ptr()}, {"cross_attn_ptr": buf.data_ptr()}):
        with pytest.raises(VapxError, match="stage 1"):
            eng.transformer_maps_device(1, n, x.data_ptr(), stage=1, **kw)
    with pytest.raises(VapxError):                               # vapx_transformer's own checks hold
        eng.transformer_maps_device(1, 51, x.data_ptr(), stage=0, attn_ptr=buf.data_ptr())
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                         # a refused call launches nothing


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split"])
def test_a_maps_call_leaves_the_stream_state_alone(model, split):
    from vap_realtime_amd import engine, synth
    S, F_ = 3, 6
    audio = synth.dialogue_batch([40, 41, 42], 800 * F_)
    a = engine.Engine(model["blob"], HZ, 2.5, max_streams=S, split_f16=split)
    b = engine.Engine(model["blob"], HZ, 2.5, max_streams=S, split_f16=split)
    try:
        for f in range(F_):
            new = audio[:, :, f * 800:(f + 1) * 800]
            want = a.step(new).copy()
            if f in (2, 4):                                      # between two steps of the same handle
                run(b, context(33 if f == 2 else 50, 3, seed=f), 0)
            assert np.array_equal(b.step(new), want), f"frame {f}"
    finally:
        a.close()
        b.close()
