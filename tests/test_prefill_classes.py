"""The checker of tests/prefill_classes.py has coverage and detection power, proved on the CPU (what tests/test_window_sweep.py is for the
window sweep and tests/test_encoder_stages.py for the stage bound).

Coverage: ``plan`` asks the library's tile rule for every GEMM of every chunk of every case and asserts what each case is there for;
``check_coverage`` asserts that the cases together reach every dispatch class, frame rate and chunk shape of ``MUST_REACH``.  A table that
lost a case, or a tile rule that moved a threshold, fails here before anything runs on a GPU.

Detection: the whole checker (``run_case``: program, records after every call, the last chunk's buffers, refused peeks, three further
steps) runs on ``StandIn``, an engine stand-in backed by an oracle that walks the engine's own chunk plan.  Backed by the fp32 oracle it
is accepted at err / E32 <= 1 in cases A, B and G, shortened to tens of frames (the chunk shapes stay: one chunk longer than the window;
three streams over a chunk boundary; n_cpc = 20) and in H (five steps, then two calls).  Backed by the float64 oracle with one seeded
fault it is rejected, with the case, the stream and the frame in the message:

    1. a frame that a later frame of the same chunk overwrites is written anyway and wins (A, G: fc > T)
    2. the virtual batch read stream-major instead of frame-major, three streams (B)
    3. the LSTM state restarted from the call's initial state at the second chunk (B)
    4. the second chunk's first frame prefixed by the carry instead of the block's own 320 samples (B)
    5. the call's first ring slot taken as 0 on a ring that holds five frames (H)
    6. a 1e-3 relative error in 128 rows of conv1's output in the last chunk (B; the stage check names h1)
    7. a 1e-4 relative error in c alone (B)

Rejection margins (error / bound, printed with -s): fault 7 at 12.5 x the bound, fault 6 at 125 x, the others above 1e4 x.  In the shortened
case B the second chunk's first frame is still in the window.  At the GPU test's full size (chunks of 341 and 19 frames, T = 12) it is
not, and faults 3 and 4 reach the records only through the LSTM's memory of a frame 7 - 18 frames back: tried once with this stand-in at
full size, the oldest ring row (frame 348) rejects fault 4 at 20 x the bound and fault 3 at 144 x."""
import re

import pytest

import prefill_classes as PC

SHORT = {
    "A": PC.CASES["A"]._replace(must={}, program=(("prefill", 30),)),                               # one chunk, fc = 30 > T = 12
    "B": PC.CASES["B"]._replace(must={}, max_batch=40, program=(("prefill", 20),)),                 # chunks of 13 and 7 frames x 3 streams
    "G": PC.CASES["G"]._replace(must={}, program=(("prefill", 10),)),                               # one chunk, fc = 10 > T = 4, n_cpc = 20
    "H": PC.CASES["H"]._replace(must={}, program=(("step", 5), ("prefill", 20), ("prefill", 15))),
}
FAULTS = [("overwritten_wins", "A", "ring"), ("overwritten_wins", "G", "ring"), ("stream_major", "B", "ring"), ("lstm_restart", "B", "ring"),
          ("carry_prefix", "B", "ring"), ("bhead0", "H", "ring"), ("tile128", "B", "h1"), ("c_rel", "B", "c")]
_TRUTH = {}


def truth(hz):
    if hz not in _TRUTH:
        _TRUTH[hz] = PC.Truth(hz, [c for c in SHORT.values() if c.hz == hz])
    return _TRUTH[hz]


def stand_in(case, fault=None, f64=True):
    tr = truth(case.hz)
    return PC.StandIn(tr.o64 if f64 else tr.o32, case, PC.population(case)[2], fault)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_case_reaches_what_it_is_there_for():
    reached = PC.check_coverage(list(PC.CASES.values()))
    assert PC.MUST_REACH <= reached
    for c in PC.CASES.values():
        for path in c.paths:
            pl = PC.plan(c, path, c.routes)
            assert sum(len(call.chunks) for call in pl.calls) >= 1
            for call in pl.calls:
                assert sum(ch.fc for ch in call.chunks) == call.frames and all(ch.V <= c.max_batch for ch in call.chunks)


def test_the_chunks_of_the_table():
    """V per chunk as the issue's table has it, and the tile classes as the library's rule gives them."""
    V = {cid: [[ch.V for ch in call.chunks] for call in PC.plan(c, "fp32").calls] for cid, c in PC.CASES.items()}
    assert V == {"A": [[300]], "B": [[1023, 57]], "C": [[1840]], "E": [[500]], "F": [[128]], "G": [[40]], "H": [[600], [450]]}
    tiles = lambda cid, i=0: {k: g[4] for k, g in PC.plan(PC.CASES[cid], "fp32").calls[0].chunks[i].gemms.items()}
    assert tiles("A") == {"conv1": 64, "gx": 32, "qkv": 32}
    assert tiles("B") == {"conv1": 64, "conv2": 64, "conv3": 64, "conv4": 32, "gx": 32}    # 341 frames, none among the last 12: no Q|K|V
    assert tiles("B", 1) == {"conv1": 32, "gx": 32, "qkv": 32}
    assert tiles("C") == {"conv1": 128, "conv2": 64, "conv3": 64, "conv4": 64, "gx": 128, "qkv": 32}
    assert PC.plan(PC.CASES["C"], "fp32").calls[0].chunks[0].gemms["conv1"][0] == 206080


def test_a_thinned_table_or_a_moved_threshold_is_refused():
    with pytest.raises(AssertionError, match="conv1_128"):
        PC.check_coverage([c for c in PC.CASES.values() if c.id != "C"])
    with pytest.raises(AssertionError, match="nonzero_bhead"):
        PC.check_coverage([c for c in PC.CASES.values() if c.id != "H"])
    with pytest.raises(AssertionError, match="case A fp32: the plan does not reach .*conv1_64"):
        PC.plan(PC.CASES["A"]._replace(program=(("prefill", 100),)))                       # M = 11200: still the 32-row tile


# ---- detection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["A", "B", "G", "H"])
def test_fp32_oracle_is_accepted(cid):
    case = SHORT[cid]
    res = PC.run_case(stand_in(case, f64=False), case, "fp32", truth(case.hz), route="pageable")
    figs = res["figures"]
    assert {"ring", "cache", "h", "c", "h0", "h1", "z", "e"} <= set(figs), sorted(figs)
    for field, f in figs.items():
        assert f["err/E32"] <= 1.0 + 1e-9 and f["err/bound"] <= 1.0 / 8 + 1e-9, (cid, field, f)
    print(f"case {cid} (shortened), fp32 oracle: err / E32", {k: round(f["err/E32"], 3) for k, f in figs.items()}, "continuation", f"{res['cont']:.2e}")


def test_float64_oracle_is_accepted_at_zero():
    case = SHORT["B"]
    res = PC.run_case(stand_in(case), case, "fp32", truth(case.hz), route="pageable")
    for field, f in res["figures"].items():
        assert f["err/bound"] < 1e-2, (field, f)                                           # float32 records of float64 values: 6e-8 of 8e-6


@pytest.mark.parametrize("fault,cid,field", FAULTS, ids=[f"{f}-{c}" for f, c, _ in FAULTS])
def test_a_seeded_fault_is_rejected(fault, cid, field):
    case = SHORT[cid]
    with pytest.raises(AssertionError) as ex:
        PC.run_case(stand_in(case, fault), case, "fp32", truth(case.hz), route="pageable")
    msg = str(ex.value)
    print(f"{fault} in case {cid}: {msg}")
    assert f"case {cid} fp32" in msg and re.search(r"stream \d+ \(slot \d+, dialogue \d+\)", msg) and re.search(r"frame \d+", msg), msg
    assert (f": {field} (" in msg) if field == "h1" else (f": {field} " in msg), msg
    m = re.search(r"= ([0-9.]+) x bound", msg)
    assert m and float(m.group(1)) >= 1.5, msg                                             # encoder_stages.MARGIN
    if fault == "tile128":
        assert "conv1 32-row tiles" in msg and "entry 1)" in msg, msg                      # rows 128 .. 255: entry 1 (frame 0, stream 1) on


def test_the_faults_are_the_seven_of_the_issue():
    assert {f for f, _, _ in FAULTS} == {"overwritten_wins", "stream_major", "lstm_restart", "carry_prefix", "bhead0", "tile128", "c_rel"}
    doc = PC.StandIn.__doc__
    assert all(f'"{f}"' in doc for f, _, _ in FAULTS)
