"""Every window fill and ring rotation of one window size T in ONE ragged batch, checked once against the float64 oracle.

The row tests (tests/test_layer_rows_gpu.py, tests/test_ffn_tiles_gpu.py) reach a window state by stepping frame after frame and look
at a handful of checkpoints.  Here ``set_state`` puts an encoder-like window into each stream of a batch, a short tick program slides
the full ones to their rotation, and the final tick runs every stream at once: every fill n = 1 .. T (or, for T > 64, every edge of
every 32-key tile plus one interior fill per valid-tile count) and every ring rotation of interest, ``rot = T - 1`` and the multiples
of 32 included.  One batch therefore holds many distinct (n, rot) pairs, so a 32- or 64-row flat tile straddles windows of different
slots and rotations almost everywhere.

    plan(T)            the target states (n, rot), one stream each; asserts its own coverage
    schedule(plan, T)  the tick program: which rows go into which slot before which tick, who steps on which tick
    donor(...)         encoder-like rows to inject: the fp32 oracle's own ring over a synthetic dialogue
    drive(...)         runs the program on an engine (or a stand-in with the same methods), anchors the export, returns a Capture
    truth(...)         float64 and fp32 ``VapOracle.layers`` of every stream's EXPORTED window (the encoder stays outside the test)
    check(...)         ``layer_rows.check_rows`` on o / stereo0 / stereo1 (/ stereo2), ``head_stages.check_tick`` on ``last``

The bound is the project's rule, unchanged and per stream: 8 x max(E32, 1e-6 max|x|), E32 the fp32 oracle's own error on that
stream's buffer.  E32 is NOT pooled over streams here.
"""
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import head_stages
from layer_rows import TILE, check_rows

State = Tuple[int, int]                  # (n valid rows, ring rotation) of a stream at the final tick
DONOR_EXTRA = 64                         # the donor sequence has T + DONOR_EXTRA rows: room for slices at different offsets
LONG_ROTS = (0, 1, 2, 31, 32, 33, 63, 64, 65)
# the window sizes of tests/test_window_sweep_gpu.py, by attention dispatch class
SHORT = (1, 2, 3, 4, 5, 7, 8, 16, 20, 31, 32, 33, 36, 37, 48, 49, 52, 53, 63, 64)      # attn_block_kernel
LONG = (65, 97, 129, 160, 193, 250, 256)                                               # attention_long2 / f16x3 / proj_f16x3
XL = (257, 289, 385, 512)                                                              # attention_xl_kernel


def tiles(n: int) -> int:
    """Valid 32-key tiles of a window of n rows (the kernels' ``nt_valid``)."""
    return (n + TILE - 1) // TILE


def plan(T: int, interior: int = 13) -> List[State]:
    """Target states of one batch.  T <= 64: every fill and every rotation.  T > 64: 1, 2, T - 1, the three fills around every multiple
    of 32 below T, one interior fill (32k + ``interior``) per valid-tile count, and the rotations around 0, 32, 64, T - 64, T - 32, T."""
    assert T >= 1 and 0 < interior < TILE - 1
    if T <= 64:
        fills = list(range(1, T))
        rots = list(range(T))
    else:
        fills = {1, 2, T - 1}
        for k in range(1, T // TILE + 1):
            if TILE * k < T:                                 # 32k + 1 = T is the full window, which the rotations bring
                fills |= {TILE * k - 1, TILE * k, TILE * k + 1}
        for c in range(1, tiles(T) + 1):                     # one interior fill per valid-tile count that a fill below T can have
            n = TILE * (c - 1) + interior
            if n < T:
                fills.add(n)
        fills = sorted(f for f in fills if 1 <= f < T)
        rots = sorted({r for r in LONG_ROTS + tuple(T - d for d in (65, 64, 63, 33, 32, 31, 2, 1)) if 0 <= r < T})
    states = [(n, 0) for n in fills] + [(T, r) for r in rots]
    check_plan(states, T)
    return states


def check_plan(states: Sequence[State], T: int) -> None:
    """The coverage every plan must have, whatever was thinned out of it."""
    assert len(set(states)) == len(states), "two streams share a state"
    assert all(1 <= n <= T and 0 <= r < T and (r == 0 or n == T) for n, r in states), states
    ns = {n for n, _ in states}
    rots = {r for n, r in states if n == T}
    assert {tiles(n) for n in ns} == set(range(1, tiles(T) + 1)), f"T={T}: valid-tile counts {sorted({tiles(n) for n in ns})}"
    for m in range(TILE, T, TILE):                           # every multiple of 32 below T, with both neighbours (m + 1 may be T itself)
        assert {m - 1, m, m + 1} <= ns, f"T={T}: fill {m} or a neighbour is missing"
    assert T - 1 in rots, f"T={T}: rot = T - 1 is missing"
    assert 0 in rots
    if T > TILE:
        assert any(r and r % TILE == 0 for r in rots), f"T={T}: no rotation is a multiple of 32"
    if T > 1:
        assert {1, T - 1} <= ns


class Program(NamedTuple):
    states: List[State]                  # per stream
    slot: np.ndarray                     # per stream: its slot of the engine, a permutation that is never the identity
    max_streams: int
    rows: List[int]                      # per stream: rows injected
    steps: List[int]                     # per stream: ticks it is stepped on (the last ``steps`` ticks)
    ticks: int
    batches: List[np.ndarray]            # per tick: the streams stepped, in batch order (shuffled)


def schedule(states: Sequence[State], T: int, seed: int = 0) -> Program:
    states = list(states)
    rng = np.random.default_rng(seed * 1000 + T)
    rows, steps = [], []
    for n, r in states:
        if n < T:
            assert r == 0
            rows.append(n - 1)
            steps.append(1)
        else:
            rows.append(T if r >= 1 else T - 1)
            steps.append(max(r, 1))
    ticks = max(steps)                                       # max(rot, 1): every tick steps somebody
    B = len(states)
    max_streams = B + 3
    while True:
        slot = rng.permutation(max_streams)[:B].astype(np.int32)
        if B == 0 or (slot != np.arange(B)).any():
            break
    batches = []
    for k in range(ticks):
        live = np.array([i for i in range(B) if ticks - steps[i] <= k], dtype=np.int64)
        batches.append(live[rng.permutation(len(live))])
    assert len(batches[-1]) == B
    return Program(states, slot, max_streams, rows, steps, ticks, batches)


def donor(cpc, vap, hz: int, frames: int, seed: int = 11) -> np.ndarray:
    """[2 dialogues, frames, 2, 256] float32: the fp32 oracle's ``advance`` over ``frames`` frames of two synthetic dialogues.  The
    encoder is causal, so a shorter donor is a prefix of a longer one."""
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth
    hop = 16000 // hz
    audio = synth.dialogue_batch([seed, seed + 1], hop * frames)
    o32 = VapOracle(cpc, vap, hz, frames / hz + 0.5 / hz)
    st, fr = o32.new_state(2), ServerFramer(2, hop)
    for f in range(frames):
        o32.advance(fr.frame(audio[:, :, f * hop:(f + 1) * hop]), st)
    return np.stack([r.numpy() for r in st.ring], axis=1).astype(np.float32)


def injected_rows(prog: Program, T: int, don: np.ndarray) -> List[np.ndarray]:
    """Per stream: [2, rows, 256], a slice of the donor at an offset of its own (alternating dialogue; odd streams swap the channels)."""
    assert don.shape[1] >= T + DONOR_EXTRA, don.shape
    out = []
    for i, m in enumerate(prog.rows):
        off = (37 * i + 5) % (T + DONOR_EXTRA - m + 1)
        x = don[i % 2, off:off + m].transpose(1, 0, 2)       # [2, m, 256]
        out.append(np.ascontiguousarray(x[::-1] if (i // 2) % 2 else x, dtype=np.float32))
    return out


class Capture(NamedTuple):
    prog: Program
    order: np.ndarray                    # final tick: stream of each batch row
    ns: List[int]                        # per batch row of the final tick
    windows: List[np.ndarray]            # per batch row: the exported window [2, n, 256] float32, oldest row first
    peeks: Dict[str, np.ndarray]         # buffers of the final tick, batch order


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def step_audio(prog: Program, hz: int, seed: int = 0) -> List[np.ndarray]:
    """Per stream: [2, hop * steps] of synthetic dialogue, the audio of the ticks it is stepped on."""
    from vap_realtime_amd import synth
    return [synth.dialogue(500 + seed + i, (16000 // hz) * s) for i, s in enumerate(prog.steps)]


def drive(eng, T: int, prog: Program, inject: Sequence[np.ndarray], audio: Sequence[np.ndarray], hz: int, buffers: Sequence[str],
          want_last: bool, what: str = "") -> Capture:
    """Run the tick program on ``eng`` (``max_streams`` >= prog.max_streams), peek ``buffers`` (and ``last``) of the final tick, export
    every stream and anchor the export: n_frames is the planned n, the rows older than the stepped ones are bit-equal to the injected
    rows shifted by the number of steps, and the newest row is bit-equal to the stream's row of ``peek("e")`` of the final tick."""
    from vap_realtime_amd import engine as E
    hop = 16000 // hz
    B = len(prog.states)
    for k in range(prog.ticks):
        for i in range(B):
            if prog.ticks - prog.steps[i] == k:              # injected just before its first tick; LSTM state and carry stay at reset
                eng.reset_stream(int(prog.slot[i]))
                if prog.rows[i]:
                    ring = np.zeros((2, T, 256), np.float32)
                    ring[:, :prog.rows[i]] = inject[i]
                    eng.set_state(int(prog.slot[i]), {"ring": ring, "n_frames": prog.rows[i]})
        live = prog.batches[k]
        new = np.stack([audio[i][:, (k - (prog.ticks - prog.steps[i])) * hop:(k - (prog.ticks - prog.steps[i]) + 1) * hop] for i in live])
        eng.step(new, prog.slot[live])
    order = prog.batches[-1]
    peeks = {b: eng.peek(b, (B, 2, T, 256)).copy() for b in buffers}
    peeks["e"] = eng.peek("e", (B, 2, 256)).copy()
    if want_last:
        peeks["last"] = eng.peek("last", (B, 2, 256)).copy()
    rec = E.split_state(eng.export_streams(prog.slot[order], cache=False), T)
    ns, windows = [], []
    for b, i in enumerate(order):
        n, r = prog.states[i]
        where = f"{what} stream {i} (slot {prog.slot[i]}, n = {n}, rot = {r})"
        got_n = int(rec["n_frames"][b])
        assert got_n == n, f"{where}: the export says n_frames = {got_n}"
        win = np.ascontiguousarray(rec["ring"][b, :, :n])
        old = n - prog.steps[i]                              # rows that were injected and have not slid out
        if old > 0:
            want = inject[i][:, prog.rows[i] - old:]
            same = (_bits(win[:, :old]) == _bits(want)).all(axis=2)
            if not same.all():
                c, t = [int(v[0]) for v in np.nonzero(~same)]
                raise AssertionError(f"{where}: exported row {t} of channel {c} is not injected row {prog.rows[i] - old + t}")
        assert (_bits(win[:, n - 1]) == _bits(peeks["e"][b])).all(), f"{where}: the newest exported row is not peek(\"e\") of the final tick"
        ns.append(n)
        windows.append(win)
    return Capture(prog, order, ns, windows, peeks)


class Truth(NamedTuple):
    ref64: List[Dict[str, np.ndarray]]   # per batch row: buffer -> [2, n, 256]
    ref32: List[Dict[str, np.ndarray]]


def truth(o64, o32, cap: Capture, layers64=None) -> Truth:
    """Both oracles' ``layers`` on every exported window; streams of equal n run as one batch.  ``layers64``: a replacement for
    ``o64.layers`` (the CPU proof's seeded faults)."""
    return Truth(layers_by_n(o64, cap.windows, layers64), layers_by_n(o32, cap.windows))


def layers_by_n(orc, windows: Sequence[np.ndarray], layers=None) -> List[Dict[str, np.ndarray]]:
    """``orc.layers`` (or ``layers(state)``) of every window [2, n, 256]; windows of equal n run as one batch.  Per window: buffer ->
    [2, n, 256]."""
    import torch
    by_n: Dict[int, List[int]] = {}
    for b, w in enumerate(windows):
        by_n.setdefault(w.shape[1], []).append(b)
    ref: List[Optional[dict]] = [None] * len(windows)
    for n, rows in by_n.items():
        X = np.stack([windows[b] for b in rows])                                  # [S, 2, n, 256]
        st = orc.new_state(len(rows))
        st.ring = [torch.from_numpy(np.ascontiguousarray(X[:, :, t])).to(orc.dtype) for t in range(n)]
        res = (layers or orc.layers)(st)
        for k, b in enumerate(rows):
            ref[b] = {name: v[k] for name, v in res.items()}
    return ref


def check(cap: Capture, tr: Truth, buffers: Sequence[str], T: int, what: str = "", path: str = "", at: Optional[dict] = None,
          excess: Optional[dict] = None) -> Dict[str, float]:
    """``check_rows`` on every buffer of ``buffers``, stream by stream, and, where the capture has it, ``head_stages.check_tick`` on
    ``last`` against row n - 1 of the oracle's stereo2.  Returns the worst err / E32 per buffer (per-stream E32; ``last``: the tick's
    pooled E32, as head_stages defines that check); ``at[buffer]`` receives the state (n, rot) of the stream that gave it, ``excess[buffer]``
    the worst err / bound."""
    states = [cap.prog.states[i] for i in cap.order]
    names = [f"{i} (slot {cap.prog.slot[i]}, n = {n}, rot = {r}, {tiles(n)} tiles)" for i, (n, r) in zip(cap.order, states)]
    worst = {}
    for buf in buffers:
        ratios = [check_rows(buf, cap.peeks[buf][b:b + 1], [cap.ns[b]], [tr.ref64[b][buf]], [tr.ref32[b][buf]], streams=[names[b]],
                             what=f"{what} T={T}", excess=excess) for b in range(len(cap.ns))]
        worst[buf] = max(ratios)
        if at is not None:
            at[buf] = states[int(np.argmax(ratios))]
    if "last" in cap.peeks:
        w: dict = {}
        head_stages.check_tick("vap", [{"last": cap.peeks["last"][b]} for b in range(len(cap.ns))],
                               [{"last": r["stereo2"][:, -1]} for r in tr.ref64], [{"last": r["stereo2"][:, -1]} for r in tr.ref32],
                               path=path, streams=names, what=f"{what} T={T}", stages=("last",), worst=w, excess=excess)
        worst["last"] = w["last"]
    return worst
