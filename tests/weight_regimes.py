"""Weight regimes: deterministic transforms of ``weights.synthetic_weights`` that drive the inputs of the non-linearities to where a
trained checkpoint can put them, and the pieces the CPU proof (tests/test_weight_regimes.py) and the GPU module
(tests/test_weight_regimes_gpu.py) share.

``synthetic_weights`` draws isotropic Gaussians of std 1.5 / sqrt(fan_in), gamma = 1 +- 0.2 and beta = +- 0.2; under them the LSTM gates
stay below 6.4, the GELU inputs below 6.5, the head logits below 6.7 and the attention logits below 45.  The thresholds a regime is
there to pass are facts of fp32, not of the kernels:

    16.6   = 24 ln 2: 1 + exp(-x) == 1 in fp32 from there on (the sigmoid saturates)
    9.01   tanh(x) rounds to 1.0f from there on
    5.94   = 4.2 sqrt 2: erfc(|x| / sqrt 2) < 3e-9; the fitted erfc of gelu_fast ends there and is clamped
    104    exp(-x) underflows to 0 in fp32 (denormals included) from there on: a key that far below the row maximum weighs nothing
    30     exp(-30) = 9e-14 is far below half an ulp of the sum: most classes of a confident head add nothing to it

    regime   transform                                                            what it reaches (float64 oracle, ``reach``)
    base     none (control)                                                       the ranges above
    lstm     gAR.baseNet.* x 6                                                    gates beyond 16.6, tanh input / cell beyond 9.01
    ffn      ffnetwork.0 x 4, ffnetwork.3 x 1/4                                   GELU input beyond 20, both signs
    ffn300   ffnetwork.0 x 300, ffnetwork.3 / 300                                 the split path's hid_scale < 1 (``hidden_bound`` >= 2^15)
    attn     every query and key x 3 (self and cross)                             logit spread inside a softmax row beyond 104
    heads    vap_head, va_classifier, bc_head, nod_head x 8                       head logit spread beyond 30, VAD logit beyond 16.6
    gains    every LN / ChannelNorm gamma log-uniform in [0.05, 8] keeping its    GELU beyond 5.94 on both signs, 16 |gamma| + |beta| <= 138
             sign, beta x 10
    tiny     gAR.baseNet.* / 64, ffnetwork.0 and query / 16                       every gate input below 0.25: the cancellation end of fast_tanh

Nothing here runs the reference.
"""
import zlib
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import encoder_stages as ES

SD = Dict[str, np.ndarray]
AMPS = (1e-3, 1.0, 30.0)
SIGMOID_SAT, TANH_SAT, ERFC_END, EXP_UNDERFLOW, HEAD_SPREAD, TINY_GATE = 16.6, 9.01, 5.94, 104.0, 30.0, 0.25
HEAD_KEYS = ("vap_head", "va_classifier", "bc_head", "nod_head")


def _scale(sd: SD, pred: Callable[[str], bool], s: float) -> SD:
    return {k: ((v * np.float32(s)).astype(np.float32) if pred(k) else v) for k, v in sd.items()}


def is_norm(k: str) -> bool:
    return "batchNorm" in k or ".ln." in k or "ln_" in k


def _gains(sd: SD) -> SD:
    out = {}
    for k, v in sd.items():
        if is_norm(k) and k.endswith(".weight") and v.size == 256:
            rng = np.random.default_rng(zlib.crc32(k.encode()))              # per tensor, whatever else the dict holds
            g = np.exp(rng.uniform(np.log(0.05), np.log(8.0), v.shape))
            out[k] = (g * np.where(v < 0, -1.0, 1.0)).astype(np.float32)
        elif is_norm(k) and k.endswith(".bias"):
            out[k] = (v * np.float32(10.0)).astype(np.float32)
        else:
            out[k] = v
    return out


def _qk(k: str) -> bool:
    return k.endswith(("query.weight", "key.weight"))


REGIMES: Dict[str, Callable[[SD, SD], Tuple[SD, SD]]] = {
    "base": lambda c, v: (c, v),
    "lstm": lambda c, v: (_scale(c, lambda k: "baseNet" in k, 6.0), v),
    "ffn": lambda c, v: (c, _scale(_scale(v, lambda k: k.endswith("ffnetwork.0.weight"), 4.0), lambda k: k.endswith("ffnetwork.3.weight"), 0.25)),
    "ffn300": lambda c, v: (c, _scale(_scale(v, lambda k: k.endswith("ffnetwork.0.weight"), 300.0),
                                      lambda k: k.endswith("ffnetwork.3.weight"), 1.0 / 300.0)),
    "attn": lambda c, v: (c, _scale(v, _qk, 3.0)),
    "heads": lambda c, v: (c, _scale(v, lambda k: k.startswith(HEAD_KEYS), 8.0)),
    "gains": lambda c, v: (_gains(c), _gains(v)),
    "tiny": lambda c, v: (_scale(c, lambda k: "baseNet" in k, 1.0 / 64.0),
                          _scale(v, lambda k: k.endswith(("ffnetwork.0.weight", "query.weight")), 1.0 / 16.0)),
}


def apply(name: str, cpc: SD, vap: SD) -> Tuple[SD, SD]:
    return REGIMES[name](dict(cpc), dict(vap))


def transform(name: str) -> Callable[[SD, SD], Tuple[SD, SD]]:
    """The ``weights=`` argument of the run_case harnesses."""
    return lambda cpc, vap: apply(name, cpc, vap)


def weights(name: str, seed: int, hz: int, mode: str = "vap") -> Tuple[SD, SD]:
    from vap_realtime_amd import weights as W
    return apply(name, *W.synthetic_weights(seed, hz, mode))


# ---- static bounds of the split path, as vapx_create derives them from the weights ------------------------------------------------------
def norm_bound(cpc: SD, vap: SD) -> float:
    """max over every ChannelNorm / LayerNorm of 16 |gamma| + |beta|: the bound on a normalised row of 256 values."""
    worst = 0.0
    for sd in (cpc, vap):
        for k, g in sd.items():
            if is_norm(k) and k.endswith(".weight") and g.size == 256:
                b = sd[k[:-len("weight")] + "bias"]
                worst = max(worst, float((16.0 * np.abs(g.astype(np.float64)) + np.abs(b.astype(np.float64))).max()))
    return worst


def hidden_bound(vap: SD, layer: str) -> float:
    """max_j sum_k |W0[j][k]| (16 |gamma_k| + |beta_k|) of one layer's FFN: hid_scale < 1 once it reaches 2^15."""
    w0 = np.abs(vap[f"{layer}.ffnetwork.0.weight"].astype(np.float64))
    y = 16.0 * np.abs(vap[f"{layer}.ln_ffnetwork.weight"].astype(np.float64)) + np.abs(vap[f"{layer}.ln_ffnetwork.bias"].astype(np.float64))
    return float((w0 @ y).max())


# ---- what a regime reaches --------------------------------------------------------------------------------------------------------------
def fold(pre: dict, acc: Optional[dict] = None) -> dict:
    """Fold one ``collect["pre"]`` dict of the oracle into running extremes and empty it."""
    import torch
    acc = {} if acc is None else acc

    def up(key, val):
        acc[key] = max(acc.get(key, 0.0), float(val))
    for name, xs in pre.items():
        for x in xs:
            x = x.detach().double()
            if name == "gates":
                i, f, g, o = x.split(256, dim=1)
                up("sigmoid_in", torch.stack([i, f, o]).abs().max())
                up("tanh_in", g.abs().max())
                up("gate_in", x.abs().max())
            elif name == "cell":
                up("tanh_in", x.abs().max())
                up("cell", x.abs().max())
            elif name.startswith("gelu."):
                site = "erf" if name in ("gelu.downsample", "gelu.combinator") else "ffn"
                up(f"gelu_{site}_pos", x.max())
                up(f"gelu_{site}_neg", -x.min())
            elif name.startswith("att."):
                fin = torch.isfinite(x)
                hi = torch.where(fin, x, torch.full_like(x, -1e300)).amax(-1)
                lo = torch.where(fin, x, torch.full_like(x, 1e300)).amin(-1)
                up("attn_spread", (hi - lo).max())
                up("attn_abs", torch.where(fin, x, torch.zeros_like(x)).abs().max())
            elif name in ("head", "aux"):
                up(f"{name}_spread", (x.amax(-1) - x.amin(-1)).max())
            elif name == "vad":
                up("vad_abs", x.abs().max())
            elif name == "p_bc":
                up("p_bc_abs", x.abs().max())
    pre.clear()
    return acc


_REACH: dict = {}


def reach(name: str, mode: str = "vap", hz: int = 20, seed: int = 23, frames: int = 40) -> dict:
    """The float64 oracle over 3 dialogues at amplitudes 1e-3 / 1 / 30 and ``frames`` free-running frames (T = 50 at 20 Hz): the extremes
    of every non-linearity's input (``fold``), cached."""
    key = (name, mode, hz, seed, frames)
    if key not in _REACH:
        import torch
        from oracle.vap_oracle import ServerFramer, VapOracle
        from vap_realtime_amd import synth
        cpc, vap = weights(name, seed, hz, mode)
        o64 = VapOracle(cpc, vap, hz, 2.5, mode=mode, dtype=torch.float64)
        hop = 16000 // hz
        audio = synth.dialogue_batch([40, 41, 42], hop * frames) * np.asarray(AMPS, np.float32)[:, None, None]
        st, fr, pre, acc = o64.new_state(3), ServerFramer(3, hop), {}, {}
        for f in range(frames):
            o64.step(fr.frame(audio[:, :, f * hop:(f + 1) * hop]), st, {"pre": pre})
            fold(pre, acc)
        acc["norm_bound"] = norm_bound(cpc, vap)
        acc["hidden_bound"] = max(hidden_bound(vap, l) for l in ("ar_channel.layers.0", "ar.layers.0", "ar.layers.1", "ar.layers.2"))
        _REACH[key] = acc
    return _REACH[key]


# ---- (a) the encoder, teacher-forced ----------------------------------------------------------------------------------------------------
class Tick:
    """One teacher-forced tick of S streams: the common state BEFORE it (fp32 values: ``h`` / ``c`` [S, 2, 256], ``carry`` [S, 2, 320],
    ``ring`` [S, 2, n, 256] oldest row first), the new samples [S, 2, hop], the frame [S, 2, L], and both oracles' stages after ONE step
    from that state (``encoder_stages.collect_stages`` layout, ``h`` / ``c`` included).  ``ref`` / ``allow``: ``recurrent_reference``."""

    def __init__(self, k, h, c, carry, ring, new, frame, r64, r32):
        self.k, self.h, self.c, self.carry, self.ring, self.new, self.frame, self.r64, self.r32 = k, h, c, carry, ring, new, frame, r64, r32


CHECKED = (1, 2, 3, 27, 28, 29, 30, 31, 32, 33, 34, 35)   # 12 of 35 frames: the start from reset, then states the recurrence has built up


def teacher_ticks(cpc: SD, vap: SD, hz: int, frames: int = 35, checked: Sequence[int] = CHECKED, seed: int = 23, ctx: float = 1.0):
    """The recurrent stages one tick at a time from a common state.  The float64 oracle runs the dialogue over ``frames`` frames; after
    every frame its state is rounded to fp32, and THAT state is what the float64 oracle, the fp32 oracle and the path under test all
    start the next tick from.  So E32 and the error under test are one step's arithmetic, not the recurrence's amplification of older
    rounding: with the LSTM weights x 6 the fp32 oracle's own error on lstm_out grows a hundredfold within 40 free-running frames, and
    k x E32 over a free run is noise.  Only the frames in ``checked`` (1-based) are yielded; the others build the state up (under ``lstm``
    the cell passes 44 only after some twenty frames, and it reaches 197 at frame 40)."""
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth
    o64, o32 = VapOracle(cpc, vap, hz, ctx, dtype=torch.float64), VapOracle(cpc, vap, hz, ctx)
    S, hop = len(AMPS), 16000 // hz
    audio = synth.dialogue_batch([seed + 100 * k for k in range(S)], hop * frames) * np.asarray(AMPS, np.float32)[:, None, None]
    fr = ServerFramer(S, hop)
    h = np.zeros((S, 2, 256), np.float32)
    c = np.zeros((S, 2, 256), np.float32)
    ring: List[np.ndarray] = []
    for k in range(frames):
        carry = fr.carry.copy()
        new = np.ascontiguousarray(audio[:, :, k * hop:(k + 1) * hop])
        frame = fr.frame(new)
        s64 = o64.new_state(S)
        s64.h, s64.c = torch.from_numpy(h).double(), torch.from_numpy(c).double()
        r64 = ES.collect_stages(o64, frame, s64)
        if k + 1 in checked:
            s32 = o32.new_state(S)
            s32.h, s32.c = torch.from_numpy(h.copy()), torch.from_numpy(c.copy())
            win = np.stack(ring[-o64.T:], axis=2) if ring else np.zeros((S, 2, 0, 256), np.float32)
            tick = Tick(k, h, c, carry, win, new, frame, r64, ES.collect_stages(o32, frame, s32))
            tick.ref = recurrent_reference(o64, tick)
            yield tick
        h, c = r64["h"][:, :, 0].astype(np.float32), r64["c"][:, :, 0].astype(np.float32)
        ring.append(r64["e"][:, :, 0].astype(np.float32))


RECURRENT = ("lstm_out", "e", "h", "c")


def recurrent_reference(o64, tick: Tick) -> Dict[str, List[np.ndarray]]:
    """The reference whose error stands for E32 on the stages behind ``z``, per stream.

    The rule holds ``z`` to 8 x max(E32_z, 1e-6 max|z|), and on ``z`` the floor is the larger term: a path may be wrong on ``z`` by
    1e-6 max|z| / E32_z (some 3 x) more than the fp32 oracle is.  The LSTM hands that on through W_ih and five (20 Hz) recurrent steps;
    under ``base`` what arrives stays below the floor of lstm_out, under ``lstm`` (weights x 6) it is amplified past it, and then the
    fp32 oracle's own error on lstm_out, which starts from ITS smaller error on z, is no measure of what the rule has just allowed.  So
    the stages behind z get a second reference, made of float64 and the fp32 oracle alone: the FLOAT64 LSTM and downsample fed
    z64 + (z32 - z64) x max(1, 1e-6 max|z| / E32_z), the fp32 oracle's own error on z scaled up to the rule's allowance.  Per stream and
    stage the reference with the larger error is used; the rule itself, 8 x max(E(reference), 1e-6 max|x|), stays
    (``encoder_stages.check_stage`` is called unchanged).  There is no free factor in this, and nothing of it comes from the path under
    test.  ``tick.allow[stage]`` keeps max E(second reference) / max(E32, floor) for the printout."""
    import torch
    from layer_rows import FLOOR
    z64, z32 = tick.r64["z"], tick.r32["z"].astype(np.float64)
    S, _, P, _ = z64.shape
    k = np.ones(S)
    for s in range(S):
        e = float(np.abs(z32[s] - z64[s]).max())
        k[s] = max(1.0, FLOOR * float(np.abs(z64[s]).max()) / e) if e > 0 else 1.0
    zp = torch.from_numpy(z64 + (z32 - z64) * k[:, None, None, None]).reshape(S * 2, P, 256)
    with torch.no_grad():
        y, h, c = o64.lstm(zp, torch.from_numpy(tick.h).double().reshape(S * 2, 256), torch.from_numpy(tick.c).double().reshape(S * 2, 256))
        e = o64.downsample(y)
    second = {"lstm_out": y.reshape(S, 2, P, 256).numpy(), "e": e.reshape(S, 2, 1, 256).numpy(), "h": h.reshape(S, 2, 1, 256).numpy(),
              "c": c.reshape(S, 2, 1, 256).numpy()}
    ref, tick.allow = {}, {}
    for st in RECURRENT:
        ref[st] = []
        for s in range(S):
            e2 = float(np.abs(second[st][s] - tick.r64[st][s]).max())
            e32 = float(np.abs(tick.r32[st][s].astype(np.float64) - tick.r64[st][s]).max())
            ref[st].append(second[st][s] if e2 > e32 else tick.r32[st][s])
            tick.allow[st] = max(tick.allow.get(st, 0.0), e2 / max(e32, FLOOR * float(np.abs(tick.r64[st][s]).max())))
    return ref


def check_encoder_tick(tick: Tick, got: Dict[str, np.ndarray], *, path: str, what: str, excess: Optional[dict] = None,
                       plain: Optional[dict] = None) -> None:
    """``got[stage]``: [S, 2, P (+ guard rows), 256] as ``Engine.peek`` returns it; ``h`` / ``c`` [S, 2, 1, 256].  Every stage ``got``
    holds, in pipeline order, under ``encoder_stages.check_stage`` (8 x max(E(reference), 1e-6 max|x|) per stream block): h0 .. z against
    the fp32 oracle, the stages behind z against ``recurrent_reference``.  ``plain[stage]`` collects the worst err / bound those stages
    would have with the fp32 oracle as the only reference (a figure, not asserted)."""
    S = tick.new.shape[0]
    names = [f"{s} (amplitude {AMPS[s]:g})" for s in range(S)]
    for st in ES.STAGES + ("h", "c"):
        if st not in got:
            continue
        if plain is not None and st in RECURRENT and np.isfinite(got[st]).all():
            for s in range(S):
                bound = ES.stage_bound(st, tick.r64[st][s], tick.r32[st][s])[0]
                plain[st] = max(plain.get(st, 0.0), float(np.abs(got[st][s].astype(np.float64) - tick.r64[st][s]).max()) / bound)
        ref = tick.ref[st] if st in RECURRENT else [tick.r32[st][s] for s in range(S)]
        ES.check_stage(st, got[st], [tick.r64[st][s] for s in range(S)], ref, path=path, streams=names,
                       what=f"{what} tick {tick.k + 1}", excess=excess)


def oracle_encoder_tick(orc, tick: Tick) -> Dict[str, np.ndarray]:
    """What a path that computes like ``orc`` gives for the tick, in the layout of ``check_encoder_tick``: the CPU stand-in of an engine."""
    import torch
    st = orc.new_state(tick.new.shape[0])
    st.h, st.c = torch.from_numpy(tick.h).to(orc.dtype), torch.from_numpy(tick.c).to(orc.dtype)
    r = ES.collect_stages(orc, tick.frame, st)
    return {k: ES.with_guards(k, np.asarray(v, np.float64)).astype(np.float32) for k, v in r.items()}


# ---- (b) transformer rows: the states of one ragged batch -------------------------------------------------------------------------------
def row_states(T: int) -> List[Tuple[int, int]]:
    """(n, rot) per stream: windows after 33, T - 1, T and T + 37 frames (a fill inside the second key tile, the last fill, the full window,
    and a slid one whose rotation is no multiple of 32)."""
    return [(n, 0) for n in sorted({min(33, T - 1), T - 1})] + [(T, 0), (T, 37 % T)]


# ---- seeded faults: an oracle that computes in float64 except for ONE device-like shortcut ----------------------------------------------
FAULTS = {
    # fault                  regime    what it is
    "sigmoid_saturates_early": "lstm", # sigmoid(x) = 0 / 1 from |x| = 10 on (fp32 saturates at 16.6): off by 4.5e-5 at most, only beyond +-10
    "tanh_overflow":        "lstm",    # tanh(x) = (E - 1) / (E + 1), E = exp(2 x) in fp32: inf / inf beyond |x| = 44.4
    "erfc_unclamped":       "ffn",     # gelu_fast's fitted erfc without its clamp at z = 4.2: the degree-6 polynomial runs away
    "hid_scale_kept":       "ffn300",  # the GELU hidden row scaled down for f16 by the weight bound's power of two and never scaled back
    "softmax_without_max":  "attn",    # exp(s) / sum exp(s) in fp32 without subtracting the row maximum: overflows beyond 88.7
    "exp2_floor":           "heads",   # the head softmax's exp2 with its argument clamped at -24: every far class still adds 2^-24
    "operand_scale_gamma2": "gains",   # a layer's LN outputs as f16 operands under the scale 2^12 that |xhat| <= 6, |gamma| <= 2.2, |beta| <= 0.7 allow
    "tanh_fixed_point":     "tiny",    # fast_tanh's exp(-2 |x|) in fixed point, 2^-19 steps: an ABSOLUTE error, seen once everything is small
}
GELU_Q = (1.0022112e-4, -4.6157415e-4, -2.3022329e-3, 2.9452506e-2, -1.4896366e-1, -9.1832864e-1, -1.6279137)   # csrc/common.h


def make_faulty(cpc: SD, vap: SD, hz: int, ctx: float, fault: Optional[str], mode: str = "vap"):
    """A float64 ``VapOracle`` with one seeded fault (None: none)."""
    import torch
    import torch.nn.functional as F
    from oracle.vap_oracle import DIM, VapOracle
    assert fault is None or fault in FAULTS, fault

    def f32_round(x):
        return x.float().double()

    class Faulty(VapOracle):
        def _tanh(self, x):
            if fault == "tanh_overflow":
                E = torch.exp(2.0 * x).float()                               # fp32: inf beyond 44.4
                return ((E - 1.0) / (E + 1.0)).double()
            if fault == "tanh_fixed_point":
                t = torch.round(torch.exp(-2.0 * x.abs()) * 2.0 ** 19) / 2.0 ** 19
                return torch.sign(x) * (1.0 - t) / (1.0 + t)
            return torch.tanh(x)

        def _sigmoid(self, x):
            y = torch.sigmoid(x)
            if fault == "sigmoid_saturates_early":
                y = torch.where(x.abs() >= 10.0, (x > 0).to(x.dtype), y)
            return y

        def lstm(self, z, h, c):
            if fault not in ("tanh_overflow", "tanh_fixed_point", "sigmoid_saturates_early"):
                return super().lstm(z, h, c)
            w = self.w
            wih, whh = w["gAR.baseNet.weight_ih_l0"], w["gAR.baseNet.weight_hh_l0"]
            b = w["gAR.baseNet.bias_ih_l0"] + w["gAR.baseNet.bias_hh_l0"]
            outs = []
            for t in range(z.shape[1]):
                g = z[:, t] @ wih.T + h @ whh.T + b
                i, f, gg, o = g.split(DIM, dim=1)
                c = self._sigmoid(f) * c + self._sigmoid(i) * self._tanh(gg)
                h = self._sigmoid(o) * self._tanh(c)
                outs.append(h)
            return torch.stack(outs, dim=1), h, c

        def _gelu(self, x):
            if fault != "erfc_unclamped":
                return F.gelu(x)
            ax = x.abs()
            z = ax * 0.70710678118654752440                                  # the kernel has fminf(., 4.2f) here
            q = torch.full_like(z, GELU_Q[0])
            for coef in GELU_Q[1:]:
                q = q * z + coef
            ec = torch.exp2(q * z).float().double()
            return 0.5 * (x + ax - ax * ec)

        def _ln(self, x, name):
            y = super()._ln(x, name)
            if fault == "operand_scale_gamma2" and ".layers." in name:       # f16 (hi, lo) pair of y * 2^12: hi is inf from |y| = 15.99 on
                hi = (y * 4096.0).half().double()
                y = (hi + (y * 4096.0 - hi).half().double()) / 4096.0
            return y

        def layer(self, pre, x, src):
            if fault not in ("erfc_unclamped", "hid_scale_kept"):
                return super().layer(pre, x, src)
            v = self.v
            z = self._ln(x, f"{pre}.ln_self_attn")
            x = x + self._mha(f"{pre}.mha", z, z)
            if src is not None:
                z = self._ln(x, f"{pre}.ln_src_attn")
                x = x + self._mha(f"{pre}.mha_cross", z, src)
            z = self._ln(x, f"{pre}.ln_ffnetwork")
            hid = self._gelu(z @ v[f"{pre}.ffnetwork.0.weight"].T)
            if fault == "hid_scale_kept":
                hs, worst = 1.0, hidden_bound({k: t.numpy() for k, t in v.items() if k.startswith(pre)}, pre)
                while hs * worst >= 32768.0:
                    hs *= 0.5
                hid = hid * hs
            return x + hid @ v[f"{pre}.ffnetwork.3.weight"].T

        def _mha(self, pre, q_in, kv_in):
            if fault != "softmax_without_max":
                return super()._mha(pre, q_in, kv_in)
            import math
            v = self.v
            B, n, _ = q_in.shape
            q = (q_in @ v[f"{pre}.query.weight"].T).view(B, n, 4, 64).transpose(1, 2)
            k = (kv_in @ v[f"{pre}.key.weight"].T).view(B, n, 4, 64).transpose(1, 2)
            val = (kv_in @ v[f"{pre}.value.weight"].T).view(B, n, 4, 64).transpose(1, 2)
            att = torch.einsum("bhid,bhjd->bhij", q, k) * (1.0 / math.sqrt(DIM))
            att = att + (v[f"{pre}.m"].view(1, 4, 1, 1) * torch.arange(n, dtype=self.dtype).view(1, 1, 1, n)
                         + torch.full((n, n), float("-inf")).triu(1))
            p = torch.exp(att).float()                                       # fp32: inf beyond 88.7
            att = (p / p.sum(-1, keepdim=True)).double()
            y = (att @ val).transpose(1, 2).reshape(B, n, DIM)
            return y @ v[f"{pre}.proj.weight"].T

        def step(self, audio, st, collect=None):
            out = super().step(audio, st, collect)
            if fault == "exp2_floor" and "logits" in out:
                z = torch.from_numpy(out["logits"]).double()
                t = torch.clamp((z - z.amax(-1, keepdim=True)) * 1.4426950408889634, min=-24.0)
                p = torch.exp2(t)
                p = p / p.sum(-1, keepdim=True)
                for name, w in (("p_now", self.abp_now), ("p_future", self.abp_fut)):
                    q = p @ w
                    out[name] = (q / (q.sum(-1, keepdim=True) + 1e-5)).numpy()
            return out

    return Faulty(cpc, vap, hz, ctx, mode=mode, dtype=torch.float64)
