"""The memory-bounds suite's own ground (no GPU): the margin checker detects what it is there to detect, every kernel of csrc/*.hip is
claimed by a scenario of tests/memory_bounds.py, and the high-slot plan reaches the offsets it is about."""
import numpy as np
import pytest

import memory_bounds as mb


def _buffer(payload_words, margin_words=16):
    w = np.full(payload_words + 2 * margin_words, mb.PATTERN, dtype=np.uint32)
    return w, margin_words


def test_checker_passes_an_untouched_buffer_and_a_written_payload():
    w, m = _buffer(40)
    mb.check_words(w, 40, m)                                                    # nothing written: fine unless the row is promised
    w[m:m + 40] = np.arange(40, dtype=np.float32).view(np.uint32)
    mb.check_words(w, 40, m, defined=True)
    mb.check_words(w.view(np.int32), 40, m, defined=True)                       # int32 words, as a tensor gives them


@pytest.mark.parametrize("at", [0, 15, 16 + 40, 16 + 40 + 15], ids=["first_front", "last_front", "first_back", "last_back"])
def test_checker_detects_one_changed_margin_word(at):
    w, m = _buffer(40)
    w[m:m + 40] = 0
    w[at] ^= 1                                                                  # one bit
    with pytest.raises(AssertionError, match="in front of" if at < m else "behind"):
        mb.check_words(w, 40, m, what="probe")


@pytest.mark.parametrize("at", [0, 17, 39])
def test_checker_detects_one_leftover_payload_word(at):
    w, m = _buffer(40)
    w[m:m + 40] = 0
    w[m + at] = mb.PATTERN
    mb.check_words(w, 40, m)                                                    # the margins are fine
    with pytest.raises(AssertionError, match=f"never written, the first at word {at} of 40"):
        mb.check_words(w, 40, m, defined=True)


def test_checker_refuses_a_buffer_of_another_size():
    w, m = _buffer(40)
    with pytest.raises(AssertionError):
        mb.check_words(w, 41, m)


def test_pattern_is_a_nan_that_arithmetic_does_not_produce():
    f = np.array([mb.PATTERN], dtype=np.uint32).view(np.float32)[0]
    assert np.isnan(f) and mb.PATTERN not in (0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF)


def test_every_kernel_is_claimed_by_a_scenario():
    kernels = mb.kernel_names()
    assert len(kernels) >= 39 and {"input_classes_kernel", "state_import_kernel", "attention_xl_kernel", "gemm_f32_kernel"} <= set(kernels)
    claimed = mb.claims()
    missing = [k for k in kernels if k not in claimed]
    assert not missing, f"kernels without a memory-bounds scenario (tests/memory_bounds.py): {missing}"
    stale = [k for k in claimed if k not in kernels]
    assert not stale, f"claims for kernels that no longer exist: {stale}"
    # what the issue's table names is claimed by a scenario of this suite, not only by the older test
    by_scenario = {k for s in mb.SCENARIOS for k in s.kernels}
    newer = {"input_classes_kernel", "state_export_kernel", "state_import_kernel", "state_ln_kernel", "state_cache_scatter_kernel",
             "trunk_collect_kernel", "out_scatter_kernel", "wire_pack_kernel", "attention_map_kernel", "attention_xl_kernel"}
    assert newer <= by_scenario, sorted(newer - by_scenario)


def test_kernel_scan_sees_a_new_kernel(tmp_path):
    (tmp_path / "a.hip").write_text("template <int X>\n__global__ __launch_bounds__(256, X == 1 ? 2 : 1) void later_kernel(const Args g) {}\n"
                                    "__global__ void plain_kernel(int* p) {}\n")
    assert mb.kernel_names(str(tmp_path)) == ["later_kernel", "plain_kernel"]
    assert "later_kernel" not in mb.claims()


def test_scenario_table_is_well_formed():
    names = [s.name for s in mb.SCENARIOS]
    assert len(set(names)) == len(names)
    assert {s.group for s in mb.SCENARIOS} == set(mb.GROUPS)
    from vap_realtime_amd import engine
    for s in mb.SCENARIOS:
        assert set(s.prof) <= set(engine.PROF_CLASSES.values()), s.name
        assert s.prof or s.proofs, f"{s.name} proves neither a launch nor an output"
    for t in range(6):                                                          # slots 0 and S - 1 on every tick, no batch a multiple of a tile
        ids = mb.batch_ids(mb.S7, t)
        assert 0 in ids and mb.S7 - 1 in ids and len(ids) in (3, 7) and len(set(ids.tolist())) == len(ids)
    assert any((mb.batch_ids(mb.S7, t) != np.arange(mb.S7)[:len(mb.batch_ids(mb.S7, t))]).any() for t in range(3))


def test_high_slot_plan_reaches_the_offsets():
    for row in mb.HIGH_SLOTS:
        T, S = row.T, row.max_streams
        qkv, ring = 2 * T * 768, 2 * T * 256
        assert (S - 1) * qkv > 1 << 32 and (S - 1) * ring * 4 > 1 << 32, row.name   # elements of ring_qkv, bytes of ring
        assert S * T > 2_796_202
        below31, above31, at32 = row.probes[1], row.probes[2], row.probes[3]
        assert below31 * qkv < 1 << 31 <= above31 * qkv and abs(at32 * qkv - (1 << 32)) < qkv, row.name   # the slots next to either edge
        probes, aliases = mb.probe_plan(row)
        assert set(row.probes) <= set(probes) and probes[0] == 0 and probes[-1] == S - 1
        assert aliases and not set(aliases) & set(probes)
        for p in probes:
            if p * qkv >= 1 << 31 and p not in row.probes or p == S - 1:
                assert mb.alias_slots(T, p) and set(mb.alias_slots(T, p)) <= set(aliases), (row.name, p)
        for p in row.probes:                                                    # a table probe whose alias is a probe has a free neighbour
            if set(mb.alias_slots(T, p)) & set(probes):
                assert p + 1 in probes and set(mb.alias_slots(T, p + 1)) <= set(aliases) and mb.alias_slots(T, p + 1), (row.name, p)
    name, S = mb.HIGH_TRUNK
    assert 1 << 31 < (S - 1) * 2 * 250 * 768 < 1 << 32
    assert mb.alias_slots(50, 10) == [] and mb.alias_slots(250, 5631) == [38]   # 5631 * 250 * 2 * 256 * 4 bytes wraps into slot 38
