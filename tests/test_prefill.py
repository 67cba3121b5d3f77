"""vapx_prefill without a GPU: the shape and dtype checks ``Engine.prefill`` makes before it calls the library (against a stub library that
records the call), the chunk plan the engine walks, and the oracle identity the GPU tests (tests/test_prefill_gpu.py) rest on:
``advance`` x F followed by ``step`` is ``step`` x (F + 1)."""
import ctypes as C

import numpy as np
import pytest

from vap_realtime_amd import engine


class _StubLib:
    """What ``Engine.prefill`` needs of libvapx.so: vapx_prefill records its arguments, vapx_last_error answers."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def vapx_prefill(self, h, n, ids, audio, frames, flags, stream):
        ptr = audio.value if isinstance(audio, C.c_void_p) else int(audio)
        self.calls.append({"n": n, "ids": None if ids is None else ids.value, "audio": ptr, "frames": frames, "flags": flags, "stream": stream})
        return self.rc

    def vapx_last_error(self, h):
        return b"stub refusal"

    def vapx_destroy(self, h):
        pass


def _engine(hz=20, rc=0):
    e = engine.Engine.__new__(engine.Engine)                 # no library, no device: only what prefill reads
    e.lib, e._h, e.hop, e.frame_hz = _StubLib(rc), None, 16000 // hz, hz
    return e


def test_prefill_passes_shape_frames_and_flags():
    e = _engine()
    a = np.zeros((3, 2, 5 * 800), np.float32)
    assert e.prefill(a, [9, 2, 6]) == 5
    (c,) = e.lib.calls
    assert (c["n"], c["frames"], c["flags"], c["stream"]) == (3, 5, 0, None)
    assert c["ids"] is not None and c["audio"] % 16 == 0
    assert e.prefill(np.zeros((1, 2, 800), np.float32)) == 1 and e.lib.calls[-1]["ids"] is None


def test_prefill_realigns_a_host_block_that_is_off_by_four_bytes():
    e = _engine()
    raw = engine.aligned_bytes(4 + 2 * 2 * 1600 * 4)
    a = raw[4:].view(np.float32).reshape(2, 2, 1600)
    a[...] = np.arange(a.size, dtype=np.float32).reshape(a.shape)
    assert a.ctypes.data % 16 == 4
    seen = {}
    orig = e.lib.vapx_prefill

    def spy(h, n, ids, audio, frames, flags, stream):
        seen["copy"] = np.ctypeslib.as_array(C.cast(audio, C.POINTER(C.c_float)), (a.size,)).copy()
        return orig(h, n, ids, audio, frames, flags, stream)
    e.lib.vapx_prefill = spy
    assert e.prefill(a) == 2
    assert e.lib.calls[-1]["audio"] % 16 == 0
    np.testing.assert_array_equal(seen["copy"], a.reshape(-1))


@pytest.mark.parametrize("shape", [(3, 800), (3, 1, 800), (3, 2, 0), (3, 2, 799), (3, 2, 1200), (0, 2, 800), (2, 2, 2, 800)])
def test_prefill_refuses_a_wrong_shape_before_the_call(shape):
    e = _engine()
    with pytest.raises(ValueError):
        e.prefill(np.zeros(shape, np.float32))
    assert not e.lib.calls


@pytest.mark.parametrize("dtype", [np.float64, np.int16, np.float16])
def test_prefill_refuses_another_dtype_before_the_call(dtype):
    e = _engine()
    with pytest.raises(TypeError):
        e.prefill(np.zeros((1, 2, 800), dtype))
    assert not e.lib.calls


def test_prefill_refuses_an_id_list_of_another_length_and_reports_the_library_error():
    e = _engine()
    with pytest.raises(ValueError):
        e.prefill(np.zeros((3, 2, 800), np.float32), [1, 2])
    assert not e.lib.calls
    e = _engine(rc=-1)
    with pytest.raises(engine.VapxError, match=r"vapx_prefill failed \(-1\): stub refusal"):
        e.prefill(np.zeros((1, 2, 800), np.float32))


def test_prefill_hop_follows_the_frame_rate():
    e = _engine(hz=50)
    assert e.prefill(np.zeros((2, 2, 7 * 320), np.float32)) == 7
    with pytest.raises(ValueError):
        e.prefill(np.zeros((2, 2, 800), np.float32))         # 2.5 frames at 50 Hz


def test_cpu_torch_tensor_takes_the_host_route():
    import torch
    e = _engine()
    assert e.prefill(torch.zeros(2, 2, 1600)) == 2 and e.lib.calls[-1]["flags"] == 0
    with pytest.raises(TypeError):
        e.prefill(torch.zeros(2, 2, 1600, dtype=torch.float64))


# ---- the chunk plan ---------------------------------------------------------------------------------------------------------------
def test_chunk_plan_of_the_gpu_tests_populations():
    # three streams in an engine of max_batch 8: two frames per chunk, an odd count leaves a remainder
    assert engine.prefill_chunks(8, 3, 5, 50) == [(0, 2, True), (2, 2, True), (4, 1, True)]
    assert engine.prefill_chunks(8, 3, 1, 50) == [(0, 1, True)]
    # nine streams would give floor(8 / 9) = 0: refused (n > max_batch); five give one frame per chunk
    with pytest.raises(ValueError):
        engine.prefill_chunks(8, 9, 5, 50)
    assert engine.prefill_chunks(8, 5, 3, 50) == [(0, 1, True), (1, 1, True), (2, 1, True)]
    assert engine.prefill_chunks(16, 9, 2, 50) == [(0, 1, True), (1, 1, True)]


@pytest.mark.parametrize("max_batch,n,frames,T", [(8, 3, 57, 50), (8, 1, 57, 50), (4096, 1, 250, 250), (4096, 64, 200, 200), (7, 7, 3, 1),
                                                  (8, 3, 257, 250), (5, 2, 11, 3)])
def test_chunk_plan_covers_every_frame_once_and_fills_the_last_window(max_batch, n, frames, T):
    plan = engine.prefill_chunks(max_batch, n, frames, T)
    fc = max(1, max_batch // n)
    assert [f0 for f0, _, _ in plan] == list(range(0, frames, fc))
    assert sum(k for _, k, _ in plan) == frames and all(1 <= k <= fc and n * k <= max_batch for _, k, _ in plan)
    assert all(k == fc for _, k, _ in plan[:-1])
    for f0, k, fills in plan:                                # a chunk fills the ring iff one of its frames is among the last T
        assert fills == any(g >= frames - T for g in range(f0, f0 + k))
    assert plan[-1][2]                                       # the last chunk holds the last frame: it moves the carry and the counter


@pytest.mark.parametrize("bad", [(8, 0, 1, 50), (8, 3, 0, 50), (0, 1, 1, 50), (8, 3, 5, 0)])
def test_chunk_plan_refuses_nonsense(bad):
    with pytest.raises(ValueError):
        engine.prefill_chunks(*bad)


# ---- the oracle identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 4, 7])                     # T = 5: a filling window, a full one, a rotated one
def test_advance_then_step_is_step_all_the_way(F):
    import torch
    from oracle.vap_oracle import ServerFramer, VapOracle
    from vap_realtime_amd import synth, weights as W
    cpc, vap = W.synthetic_weights(5, 20, "vap")
    audio = synth.dialogue_batch([3, 4], 800 * (F + 1))
    o = VapOracle(cpc, vap, 20, 0.25)
    assert o.T == 5
    sa, fa = o.new_state(2), ServerFramer(2, 800)
    sb, fb = o.new_state(2), ServerFramer(2, 800)
    for f in range(F):
        new = audio[:, :, f * 800:(f + 1) * 800]
        o.step(fa.frame(new), sa)
        o.advance(fb.frame(new), sb)
    assert len(sa.ring) == len(sb.ring) == min(F, 5)
    for ra, rb in zip(sa.ring, sb.ring):
        assert torch.equal(ra, rb)
    assert torch.equal(sa.h, sb.h) and torch.equal(sa.c, sb.c)
    new = audio[:, :, F * 800:(F + 1) * 800]
    wa, wb = o.step(fa.frame(new), sa), o.step(fb.frame(new), sb)
    assert set(wa) == set(wb)
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
