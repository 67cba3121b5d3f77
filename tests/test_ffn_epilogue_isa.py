"""ISA-level guard for the row-per-lane epilogues of ffn_block_kernel: the weight fragment is operand A of the
32x32x2 MFMA, so a lane's accumulators are ONE row and groups of four consecutive columns, and every hand-off of the tile (global store,
residual add, LDS park) is a 16-byte access behind one bound test per lane.  The kernel is issue-bound outside its K loops, so a
regression to 4-byte accesses with a guard per row costs time without failing any numerical test.  hipcc cross-compiles without a GPU,
so this runs in the CPU suite; the behavioural checks are tests/test_layer_rows_gpu.py and tests/test_ffn_tiles_gpu.py.

The bounds are those of the column-per-lane kernel this layout replaced (modes 0 / 1 / 2): 216 / 218 / 158 VGPRs and 78 / 93 / 47
s_and_saveexec."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vap-realtime_amd", "csrc")
SRC = os.path.join(CSRC, "fused_blocks.hip")

# mode -> (VGPRs, s_and_saveexec) of the column-per-lane kernel
BEFORE = {0: (216, 78), 1: (218, 93), 2: (158, 47)}


def _mode(sym):
    """ffn_block_kernel<MT, MODE> mangles as _Z16ffn_block_kernelILi<MT>ELi<MODE>EEv...; anything else -> None"""
    m = re.search(r"ffn_block_kernelILi(\d+)ELi(\d+)E", sym)
    return int(m.group(2)) if m else None


@pytest.fixture(scope="module")
def asm_text(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    asm = tmp_path_factory.mktemp("ffn_isa") / "fused_blocks.s"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    "-o", str(asm), SRC], check=True, capture_output=True, timeout=900)
    return asm.read_text()


@pytest.fixture(scope="module")
def kernels(asm_text):
    """mode -> (symbol, body, metadata dict) of every ffn_block_kernel instantiation"""
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):\s*; @.*?$(.*?)s_endpgm", asm_text, re.S | re.M)}
    meta = {}
    for blk in re.split(r"^  - \.agpr_count:", asm_text, flags=re.M)[1:]:   # one amdhsa.kernels entry each (keys are sorted: .agpr_count first)
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+\.(vgpr_count|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk, re.M)}
    out = {}
    for sym, body in bodies.items():
        mode = _mode(sym)
        if mode is not None:
            assert sym in meta, f"no metadata entry for {sym}"
            out[mode] = (sym, body, meta[sym])
    assert sorted(out) == [0, 1, 2], f"ffn_block_kernel instantiations found: {sorted(out)} of {sorted(bodies)[:6]} ..."
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_4_byte_global_access(kernels, mode):
    sym, body, _ = kernels[mode]
    narrow = re.findall(r"\bglobal_(?:store|load)_dword\b", body)
    assert not narrow, f"{sym}: {len(narrow)} 4-byte global accesses; the tile hand-offs are 16 bytes per lane"
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) >= 8, f"{sym}: expected the 16-byte chunk stores"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_no_scratch(kernels, mode):
    sym, body, md = kernels[mode]
    assert not re.findall(r"\bscratch_\w+", body), f"{sym}: scratch instructions"
    assert md["vgpr_spill_count"] == 0, f"{sym}: {md['vgpr_spill_count']} spilled VGPRs"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_registers_not_above_column_per_lane_kernel(kernels, mode):
    sym, _, md = kernels[mode]
    assert md["vgpr_count"] <= BEFORE[mode][0], f"{sym}: {md['vgpr_count']} VGPRs > {BEFORE[mode][0]}"


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_fewer_exec_mask_regions(kernels, mode):
    sym, body, _ = kernels[mode]
    n = len(re.findall(r"\bs_and_saveexec_b64\b", body))
    assert n < BEFORE[mode][1], f"{sym}: {n} s_and_saveexec >= {BEFORE[mode][1]}: a bound test per row is back"
