"""Random programs of every state-changing call against float64, on engines (program, model, checker: tests/stream_program.py; the CPU
proof of that checker: tests/test_stream_program.py).

    profile      engine                                                             operations
    plain_short  20 Hz, T = 12, 24 slots, max_batch 8, vap; fp32 and split          step (host, device), both resets, get / set_state and
                                                                                    record migrations (cache yes / no, host / device), prefill
                                                                                    attach and continue (1, T-1, T, T+5 frames), maps, peek,
                                                                                    encode_audio on a free slot
    plain_long   50 Hz, ctx 1.3 s, T = 65, 16 slots, max_batch 8, nod; fp32, split  the same
    crowd        20 Hz, T = 12, 88 slots, groups=2, 64 extra streams on one         step (device, defer_join), resets, one flush of 17 queued
                 oracle, so every batch has >= 64 rows; fp32 and split              resets applied by the step, migrations and maps between a
                                                                                    deferred step and its join
    two_engines  an fp32 and a split engine, 20 Hz, T = 12, 12 slots each           step, resets, migration through records without cache
    rate_8k_mulaw    input 8000 Hz mu-law, 20 Hz, T = 12, 16 slots; fp32 and split  step, resets, get / set_state (the resampler history
    rate_48k_s16     input 48000 Hz 16-bit PCM, the same engine; fp32               restarts), record migrations (it travels), prefill refused
    format_16k_alaw  input 16000 Hz A-law: a format alone; fp32                     for the rate, and here for the format
    class_table  classes f32@16000, mulaw@8000, s16@48000, alaw@32000, streams      step (packed input: host, device), resets, set_stream_class
                 with equal and with different channel classes; fp32                and set_stream_channel_classes in mid-run, get / set_state
                                                                                    with the destination's classes set first; export, import
                                                                                    and prefill refused; audited through get_state
    group_same_rate  TrunkGroup of vap + bc + nod at 20 Hz, T = 12 / 15 / 10,       step and step_wire alternating, reset_stream, group
                 16 slots; fp32 and split                                           export / import into other slots (cache yes / no)
    group_mixed  vap 20 Hz leads, nod 10 Hz (R = 2), bc 5 Hz (R = 4), T = 12 / 8    step and step_wire alternating, reset_stream in
                 / 4; dialogue d starts on leader tick d % 4, so phases differ      mid-accumulation, refused export; audited through
                 inside a batch; fp32                                               get_state of every model

Every stepped row is held against the float64 model at 1e-4 and every slot audit (after each chain of operations, every 8 ticks, at the
end) under ``encoder_stages.stage_bound``; on resampled input the history and its started flags exactly and the carry, per channel, within
K . 2^-24 . max sum|h| . max|x| of its class.  The test asserts the number of rows and slot audits the program says.  ``-s`` prints, per
field, the worst err / E32 and err / bound and the operation counts.

In a group every model's row is held against that model's own oracle at its own rate, fed R leader hops per frame counted from the
dialogue's (re)start; on the ticks its phase says no frame is due the row must carry STATUS_NO_FRAME and be zero otherwise, exactly.  An
audit covers every model's window (and cache where records exist) and the leader's LSTM and carry.

Measured on MI355X (worst err / bound per field over all audits; outputs: worst |hip - float64| over all rows; a record, not a threshold):

    profile          path   rows  slot audits  outputs   ring   cache  h      c      carry
    plain_short      fp32   275   524          7.2e-06   0.222  0.214  0.247  0.153  bit-exact
    plain_short      split  275   524          7.8e-06   0.235  0.185  0.279  0.119  bit-exact
    plain_long       fp32   253   443          2.9e-06   0.171  0.152  0.243  0.166  bit-exact
    plain_long       split  253   443          2.6e-06   0.157  0.142  0.246  0.140  bit-exact
    crowd            fp32   2763  679          1.0e-05   0.223  0.198  0.340  0.133  bit-exact
    crowd            split  2763  679          7.3e-06   0.189  0.165  0.303  0.152  bit-exact
    two_engines      mixed  237   215          8.3e-06   0.255  0.167  0.332  0.127  bit-exact
    rate_8k_mulaw    fp32   240   325          1.1e-05   0.279  0.190  0.208  0.104  0.088
    rate_8k_mulaw    split  240   325          8.8e-06   0.298  0.164  0.168  0.147  0.088
    rate_48k_s16     fp32   242   257          7.1e-06   0.262  0.195  0.280  0.112  0.080
    format_16k_alaw  fp32   193   194          7.4e-06   0.355  0.160  0.197  0.114  bit-exact
    class_table      fp32   306   419          1.3e-05   0.295  -      0.216  0.092  0.092 (16 kHz channels bit-exact)
    group_same_rate  fp32   200   145          7.9e-06   0.228  0.176  0.167  0.130  bit-exact
    group_same_rate  split  200   145          7.1e-06   0.201  0.166  0.226  0.110  bit-exact
    group_mixed      fp32   218   378          7.6e-06   0.280  -      0.226  0.123  bit-exact

The bound is 8 x max(E32, 1e-6 max|x|), E32 the fp32 oracle's own distance from float64 on the same block.  No program found a
disagreement with the engine.  Each test takes 0.1 - 0.3 s on the GPU; the float64 truth of a profile (3 - 7 s on the CPU) is computed
once and shared by its paths."""
import json
import time

import pytest

import stream_program as SP

pytestmark = pytest.mark.gpu

_TRUTH: dict = {}
PARAMS = [(name, seed, path) for name, seed in SP.COMMITTED for path in SP.PROFILES[name].paths]


def truth(name, seed):
    if (name, seed) not in _TRUTH:
        t0 = time.time()
        prog = SP.draw(name, seed)
        SP.check_coverage(prog)
        _TRUTH[(name, seed)] = (prog, SP.Truth(prog))
        print(f"STREAM_PROGRAM oracle {name} seed {seed}: {time.time() - t0:.1f} s on the CPU")
    return _TRUTH[(name, seed)]


def make_engines(prog, tr, path):
    from vap_realtime_amd import engine, weights as W
    p = prog.profile
    if p.group:                                                                            # one TrunkGroup; the runner's port closes like an engine
        grp = engine.TrunkGroup({m: W.pack_blob(tr.cpc, tr.gvap[m], m) for m, _, _ in p.group}, {m: hz for m, hz, _ in p.group},
                                {m: (T + 0.5) / hz for m, hz, T in p.group}, max_streams=prog.slots, max_batch=p.max_batch,
                                split_f16=path == "split")
        assert grp.order[0] == p.group[0][0] and grp.T_of == {m: T for m, _, T in p.group}
        return [grp]
    blob = W.pack_blob(tr.cpc, tr.vap, p.mode)
    splits = {"fp32": [False], "split": [True], "mixed": [False, True]}[path]
    assert len(splits) == p.engines
    engs = [engine.Engine(blob, p.hz, p.ctx, max_streams=prog.slots, max_batch=p.max_batch, groups=p.groups, mode=p.mode, split_f16=s,
                          input_hz=p.input_hz, input_format=p.input_format, input_classes=list(p.table) or None) for s in splits]
    assert all(e.T == p.T for e in engs)
    return engs


@pytest.mark.parametrize("name,seed,path", PARAMS, ids=[f"{n}-{s}-{p}" for n, s, p in PARAMS])
def test_random_program_of_state_calls_against_float64(name, seed, path):
    import torch
    prog, tr = truth(name, seed)
    engs = make_engines(prog, tr, path)
    try:
        torch.cuda.synchronize()
        t0 = time.time()
        res = SP.Runner(prog, tr, [SP.GroupPort(e) if prog.profile.group else SP.EnginePort(e) for e in engs]).run()
        seconds = time.time() - t0
    finally:
        for e in engs:
            e.close()
    print("STREAM_PROGRAM " + json.dumps({
        "profile": name, "seed": seed, "path": path, "seconds": round(seconds, 2), "rows": res["rows"], "slot_audits": res["audits"],
        "outputs": float(f"{res['worst_out']:.2e}"),
        "err/E32": {k: round(f["err/E32"], 2) for k, f in res["figures"].items()},
        "err/bound": {k: round(f["err/bound"], 3) for k, f in res["figures"].items()}, "operations": res["counts"]}))
    assert res["rows"] == prog.n_rows, f"{res['rows']} stepped rows compared, the program has {prog.n_rows}"
    assert res["audits"] == prog.n_audits, f"{res['audits']} slot audits made, the program has {prog.n_audits}"
    assert {"ring", "h", "c"} | ({"cache"} if prog.profile.exports else set()) <= set(res["figures"])
