"""The weight regimes of tests/weight_regimes.py reach what they are there for, and the checks that tests/test_weight_regimes_gpu.py runs
under them can see something: both proved on the CPU.

Reach: per regime the float64 oracle (3 dialogues at amplitudes 1e-3 / 1 / 30, 40 frames) passes the fp32-derived threshold of its case
(``weight_regimes`` names them: 16.6, 9.01, 5.94, 104, 30), and ``base`` stays where the suite always was.

Detection: the checkers of the GPU module (``check_encoder_tick`` teacher-forced, ``layer_rows.check_rows`` on given windows,
``head_stages.check_tick`` / ``check_own``) run on a stand-in for the engine, an oracle.  Backed by the fp32 oracle the stand-in is accepted
under every regime.  Backed by the float64 oracle with ONE seeded fault (``weight_regimes.FAULTS``: a device-like shortcut that is right
inside the synthetic range) it is accepted under ``base`` and rejected under the fault's regime:

    fault                  regime   rejected as (printed with -s)
    tanh_overflow          lstm     non-finite lstm_out at tick 33 (the cell has passed 44.4 by then; ticks 1 and 2 pass)
    sigmoid_saturates_early lstm    ``e`` at 1.21 x the bound at tick 2: a sigmoid that is 0 / 1 from |x| = 10 on is off by 4.5e-5 at most, and the
                                    second reference of ``recurrent_reference`` (which widens lstm_out / e / h / c under ``lstm``) still sees it
    tanh_fixed_point       tiny    lstm_out at 3.6 x the bound (the bound shrinks with the values, the fault's error does not)
    erfc_unclamped         ffn      non-finite rows of ``o``
    hid_scale_kept         ffn300   rows of ``o`` at 4e4 x the bound
    softmax_without_max    attn     rows of ``stereo1`` at 57 x the bound (inf / inf where a logit passes 88.7, lost keys below that)
    operand_scale_gamma2   gains    non-finite rows (a layer's LN output beyond 15.99 becomes inf in f16 under the 2^12 scale; under ``base``
                                    they stay below 8, under ``gains`` they reach 24)
    exp2_floor             heads    p_future at 1.9 x the bound (255 classes x 2^-24 = 1.5e-5 of the sum)
"""
import numpy as np
import pytest

import head_stages as HS
import weight_regimes as WR
import window_sweep as ws
from layer_rows import BUFFERS, check_rows

HZ, SEED = 20, 23
ENCODER_FAULTS = ("tanh_overflow", "tanh_fixed_point", "sigmoid_saturates_early")
HEAD_FAULTS = ("exp2_floor",)
_CACHE: dict = {}


def _oracles(regime):
    if regime not in _CACHE:
        import torch
        from oracle.vap_oracle import VapOracle
        cpc, vap = WR.weights(regime, SEED, HZ)
        _CACHE[regime] = (cpc, vap, VapOracle(cpc, vap, HZ, 2.5, dtype=torch.float64), VapOracle(cpc, vap, HZ, 2.5))
    return _CACHE[regime]


# ---- the regimes ------------------------------------------------------------------------------------------------------------------------
def test_regimes_are_pure_and_deterministic():
    from vap_realtime_amd import weights as W
    cpc, vap = W.synthetic_weights(SEED, HZ, "nod")
    before = {k: v.copy() for k, v in {**cpc, **vap}.items()}
    for name in WR.REGIMES:
        a, b = WR.apply(name, cpc, vap), WR.apply(name, cpc, vap)
        for x, y in zip(a, b):
            assert set(x) == set(y) and all(np.array_equal(x[k], y[k]) and x[k].dtype == np.float32 for k in x), name
        changed = {k for sd, src in zip(a, (cpc, vap)) for k in sd if not np.array_equal(sd[k], src[k])}
        assert bool(changed) == (name != "base"), (name, sorted(changed))
    assert all(np.array_equal(v, {**cpc, **vap}[k]) for k, v in before.items())              # the inputs are not touched
    g = WR.apply("gains", cpc, vap)
    gam = np.concatenate([v.ravel() for sd in g for k, v in sd.items() if WR.is_norm(k) and k.endswith(".weight")])
    assert 0.05 <= np.abs(gam).min() and np.abs(gam).max() <= 8.0 and gam.size == (5 + 11 + 2) * 256   # cn0-4, 11 layer norms, downsample, combinator


REACH = {
    "lstm": lambda r: r["sigmoid_in"] > WR.SIGMOID_SAT and r["tanh_in"] > WR.TANH_SAT and r["cell"] > WR.TANH_SAT,
    "ffn": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"]) > 20.0,
    "ffn300": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"]) > WR.ERFC_END and r["hidden_bound"] >= 32768.0,
    "attn": lambda r: r["attn_spread"] > WR.EXP_UNDERFLOW,
    "heads": lambda r: r["head_spread"] > WR.HEAD_SPREAD and r["vad_abs"] > WR.SIGMOID_SAT,
    "gains": lambda r: min(r["gelu_ffn_pos"], r["gelu_ffn_neg"], r["gelu_erf_pos"], r["gelu_erf_neg"]) > WR.ERFC_END and r["norm_bound"] <= 138.0,
    "tiny": lambda r: r["gate_in"] < WR.TINY_GATE,
}


@pytest.mark.parametrize("regime", list(WR.REGIMES))
def test_the_float64_oracle_reaches_the_threshold_of_the_regime(regime):
    r = WR.reach(regime)
    print(regime, {k: round(v, 2) for k, v in sorted(r.items())})
    if regime == "base":                                     # the control: where every other float64-held test of the suite stays
        assert r["sigmoid_in"] < WR.SIGMOID_SAT and r["tanh_in"] < WR.TANH_SAT and r["attn_spread"] < WR.EXP_UNDERFLOW
        assert r["head_spread"] < WR.HEAD_SPREAD and r["vad_abs"] < WR.SIGMOID_SAT and r["gelu_ffn_pos"] < 20.0 and r["hidden_bound"] < 32768.0
        assert r["gate_in"] > 1.0
    else:
        assert REACH[regime](r), r


@pytest.mark.parametrize("mode,key", [("bc", "aux_spread"), ("nod", "aux_spread")])
def test_heads_regime_reaches_the_aux_heads(mode, key):
    assert WR.reach("heads", mode, frames=10)[key] > 4.0 * WR.reach("base", mode, frames=10)[key]


# ---- detection --------------------------------------------------------------------------------------------------------------------------
def encoder_checker(regime, make):
    """(a) of the GPU module with an oracle in the engine's place."""
    cpc, vap, _, _ = _oracles(regime)
    orc = make(cpc, vap, 1.0)
    excess: dict = {}
    for tick in WR.teacher_ticks(cpc, vap, HZ, checked=(1, 2, 33, 34, 35), seed=SEED):
        WR.check_encoder_tick(tick, WR.oracle_encoder_tick(orc, tick), path="chain", what=f"{regime} stand-in", excess=excess)
    return excess


def rows_checker(regime, make):
    """(b): every row of o / stereo0-2 on given windows (fills 33 and 40, the second with the channels swapped)."""
    cpc, vap, o64, o32 = _oracles(regime)
    key = ("donor", "gains" if regime == "gains" else "base")
    if key not in _CACHE:
        _CACHE[key] = ws.donor(cpc, vap, HZ, 45)
    don = _CACHE[key]
    windows = [np.ascontiguousarray(don[0, :33].transpose(1, 0, 2)), np.ascontiguousarray(don[1, 5:45].transpose(1, 0, 2)[::-1])]
    got = ws.layers_by_n(make(cpc, vap, 2.5), windows)
    r64, r32 = ws.layers_by_n(o64, windows), ws.layers_by_n(o32, windows)
    worst = {}
    for b, w in enumerate(windows):
        for buf in BUFFERS:
            g = np.asarray(got[b][buf], np.float64).astype(np.float32)[None]
            worst[buf] = max(worst.get(buf, 0.0), check_rows(buf, g, [w.shape[1]], [r64[b][buf]], [r32[b][buf]], what=f"{regime} stand-in window {b}"))
    return worst


def heads_checker(regime, make):
    """(c): 3 dialogues, 6 free-running ticks (T = 50 at 20 Hz), every stage of vap mode and the probabilities of the stand-in's own logits."""
    from oracle.vap_oracle import ServerFramer
    from vap_realtime_amd import synth
    cpc, vap, o64, o32 = _oracles(regime)
    orc = make(cpc, vap, 2.5)
    hop = 16000 // HZ
    audio = synth.dialogue_batch([40, 41, 42], hop * 6) * np.asarray(WR.AMPS, np.float32)[:, None, None]
    fr, st = ServerFramer(3, hop), [o.new_state(3) for o in (o64, o32, orc)]
    excess: dict = {}
    for f in range(6):
        frame = fr.frame(audio[:, :, f * hop:(f + 1) * hop])
        r64, r32, rg = (HS.collect_heads(o, frame, s) for o, s in zip((o64, o32, orc), st))
        rows = lambda r, cast=False: [{k: (np.asarray(v, np.float64).astype(np.float32) if cast else v) for k, v in HS.row_of(r, s).items() if k not in ("n", "e")}
                                      for s in range(3)]
        got = rows(rg, True)
        HS.check_tick("vap", got, rows(r64), rows(r32), what=f"{regime} stand-in tick {f + 1}", excess=excess, propagate=regime == "heads")
        HS.check_own(got, what=f"{regime} stand-in tick {f + 1}", excess=excess)
    return excess


def checker_of(fault):
    return encoder_checker if fault in ENCODER_FAULTS else heads_checker if fault in HEAD_FAULTS else rows_checker


def fp32_stand_in(cpc, vap, ctx):
    from oracle.vap_oracle import VapOracle
    return VapOracle(cpc, vap, HZ, ctx)


@pytest.mark.parametrize("regime", list(WR.REGIMES))
def test_the_fp32_oracle_is_accepted_under_every_regime(regime):
    for checker in (encoder_checker, rows_checker, heads_checker):
        print(regime, checker.__name__, {k: round(v, 3) for k, v in checker(regime, fp32_stand_in).items()})


@pytest.mark.parametrize("fault", list(WR.FAULTS))
def test_a_seeded_fault_passes_base_and_fails_its_regime(fault):
    regime, checker = WR.FAULTS[fault], checker_of(fault)
    make = lambda cpc, vap, ctx: WR.make_faulty(cpc, vap, HZ, ctx, fault)
    print(fault, "under base:", {k: round(v, 3) for k, v in checker("base", make).items()})
    with pytest.raises(AssertionError) as ex:
        checker(regime, make)
    print(fault, "under", regime + ":", str(ex.value)[:400])
    assert f"{regime} stand-in" in str(ex.value)


def test_every_regime_but_the_control_has_a_seeded_fault():
    assert set(WR.FAULTS.values()) == set(WR.REGIMES) - {"base"}
