"""The checker of tests/stream_program.py has coverage and detection power, proved on the CPU (what tests/test_prefill_classes.py is for
the prefill classes).

Coverage: ``check_coverage`` holds for every committed (profile, seed) at the length the GPU test runs: every operation legal in the
profile at least three times, the orderings of ``PAIRS`` that the profile can reach, audits of a filling, an exactly full and a slid
window, a slid stream whose rotation differs from its batch neighbours', the four prefill lengths, the crowd's flush of more than 16
resets, in a mixed-rate group resets in mid-accumulation, batches of different phases and rows without a frame, every dialogue in at
least 60 % of the steps.

Detection: the runner drives shortened programs (fewer ticks, the crowd with two extra streams; the operations and chains stay) on
``StandIn`` (a trunk group: ``GroupStandIn``), a slot-level stand-in backed by an oracle.  Backed by the fp32 or the float64 oracle it passes, with every row and every slot
audit counted.  With one seeded fault it is rejected at the first audit or step after the fault took effect, and the message names the
tick, the operation, the slot, the dialogue and the field: backed by the float64 oracle, where the error without the fault is about 0, and
backed by the fp32 oracle, where it is about E32 as an engine's is."""
import re

import pytest

import stream_program as SP

SHORT = {"plain_short": dict(ticks=22), "plain_long": dict(ticks=5), "crowd": dict(ticks=12, extras=2), "two_engines": dict(ticks=10),
         "rate_8k_mulaw": dict(ticks=14), "rate_48k_s16": dict(ticks=8), "format_16k_alaw": dict(ticks=6), "class_table": dict(ticks=14),
         "group_same_rate": dict(ticks=6), "group_mixed": dict(ticks=10)}
# fault -> (profile, seed of the shortened program, the field the message has to name)
FAULT_CASES = {
    "late_reset": ("plain_short", 1, r"n_frames|ring|carry| h | c "),
    "seventeenth_dropped": ("crowd", 1, r"n is|n_frames|outputs"),
    "stale_cache": ("plain_short", 1, r"cache"),
    "cache_not_rotated": ("plain_short", 1, r"cache"),
    "set_state_keeps_head": ("plain_short", 1, r"outputs|ring"),
    "prefill_from_zero_carry": ("plain_short", 1, r"ring"),
    "carry_only_clears_window": ("plain_short", 1, r"n_frames|n is"),
    "bystander_advances": ("plain_short", 1, r" h "),
    "history_survives_reset_carry": ("rate_8k_mulaw", 1, r"resample_hist|resample_started"),
    "history_lost_on_import": ("rate_8k_mulaw", 1, r"resample_hist|resample_started"),
    "carry_survives_class_change": ("class_table", 1, r"carry"),
    "follower_phase_survives_reset": ("group_mixed", 1, r"model (nod|bc): (status|a row without a frame)"),
}
_CACHE: dict = {}


def program(name, seed):
    key = (name, seed)
    if key not in _CACHE:
        prog = SP.draw(name, seed, **SHORT[name])
        _CACHE[key] = (prog, SP.Truth(prog))
    return _CACHE[key]


def run(name, seed, f64=True, fault=None):
    prog, truth = program(name, seed)
    if prog.profile.group:
        ports = [SP.GroupStandIn(truth.g64 if f64 else truth.g32, prog, fault)]
    else:
        ports = [SP.StandIn(truth.o64 if f64 else truth.o32, prog, fault) for _ in range(prog.profile.engines)]
    return prog, ports, SP.Runner(prog, truth, ports)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,seed", SP.COMMITTED, ids=[f"{n}-{s}" for n, s in SP.COMMITTED])
def test_committed_programs_meet_the_coverage_conditions(name, seed):
    prog = SP.draw(name, seed)
    cov = SP.check_coverage(prog)
    assert 40 <= len(prog.ticks) - 1 <= 90
    assert prog.n_rows == sum(len(t.step.members) for t in prog.ticks if t.step) and prog.n_audits == sum(
        len(c.audit) for t in prog.ticks for c in t.chains + t.after)
    print(name, seed, "rows", prog.n_rows, "slot audits", prog.n_audits, "operations", cov["counts"], "orderings", sorted(cov["pairs"]))


def test_every_profile_is_committed_and_the_orderings_are_reached_somewhere():
    assert {n for n, _ in SP.COMMITTED} == set(SP.PROFILES)
    reached = set()
    for name, seed in SP.COMMITTED:
        reached |= SP.coverage(SP.draw(name, seed))["pairs"]
    assert reached == set(SP.PAIRS), sorted(reached)


def test_a_thinned_program_is_refused():
    seed = dict(SP.COMMITTED)
    prog = SP.draw("plain_short", seed["plain_short"])
    cut = prog._replace(ticks=tuple(t._replace(chains=tuple(c for c in t.chains if not c.label.startswith("P0"))) for t in prog.ticks))
    with pytest.raises(AssertionError, match=r"orderings \[12\]"):
        SP.check_coverage(cut)
    with pytest.raises(AssertionError, match="17 resets"):
        crowd = SP.draw("crowd", seed["crowd"])
        SP.check_coverage(crowd._replace(ticks=tuple(
            t._replace(chains=tuple(c for c in t.chains if not c.label.startswith("FLUSH"))) for t in crowd.ticks)))


# ---- detection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [True, False], ids=["float64", "fp32"])
@pytest.mark.parametrize("name", list(SP.PROFILES))
def test_a_clean_stand_in_passes(name, f64):
    prog, _, runner = run(name, 1, f64)
    res = runner.run()
    assert res["rows"] == prog.n_rows and res["audits"] == prog.n_audits, (res["rows"], prog.n_rows, res["audits"], prog.n_audits)
    want = {"ring", "h", "c"} | ({"cache"} if prog.profile.exports else set())             # no cache through get_state
    assert want <= set(res["figures"]), sorted(res["figures"])
    for field, f in res["figures"].items():
        if field == "carry":                                                               # resampled input: held to the resampler's own bound
            assert f["err/bound"] <= 1.0, f
        elif f64:
            # float32 records of float64 values: 2^-24 of a value is 0.0075 of a bound of 8e-6 of the block's largest, and a migrated state
            # continues from its rounded record, a few times per dialogue
            assert f["err/bound"] < 0.05, (field, f)
        else:
            assert f["err/E32"] <= 1.0 + 1e-9 and f["err/bound"] <= 1.0 / 8 + 1e-9, (field, f)
    print(name, "float64" if f64 else "fp32", {k: round(f["err/bound"], 4) for k, f in res["figures"].items()}, f"outputs {res['worst_out']:.2e}")


@pytest.mark.parametrize("f64", [True, False], ids=["float64", "fp32"])
@pytest.mark.parametrize("fault", list(SP.FAULTS))
def test_a_seeded_fault_is_rejected_at_once(fault, f64):
    """On the float64 stand-in the error without the fault is about 0, on the fp32 one about E32, the level an engine has: the fault has to
    stand out of 8 x E32 as well."""
    name, seed, field = FAULT_CASES[fault]
    prog, ports, runner = run(name, seed, f64, fault=fault)
    with pytest.raises(AssertionError) as ex:
        runner.run()
    msg = str(ex.value)
    print(f"{fault}: {msg}")
    marks = [p.fault_mark for p in ports if p.fault_mark is not None]
    assert marks, f"{fault} never took effect in {name} seed {seed}"
    assert ex.value.checkpoint == min(marks), f"{fault} took effect before check {min(marks)} and was rejected at check {ex.value.checkpoint}: {msg}"
    assert re.search(r"tick \d+ after \[[^\]]+\] engine \d+ slot \d+, dialogue (\d+|X)", msg), msg
    assert re.search(field, msg), msg


def test_the_faults_are_the_stand_ins():
    assert set(FAULT_CASES) == set(SP.FAULTS)
    assert all(f'"{f}"' in SP.StandIn.__doc__ for f in SP.FAULTS)
