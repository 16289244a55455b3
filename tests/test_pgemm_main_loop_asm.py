"""CPU (needs hipcc, no GPU): the main loops of the step's six planes products, read from the unit's gfx950 assembly with
tools/main_loop_waits.py.

The ring kernels keep LDS-DMA in flight across their barriers with hand-counted s_waitcnt vmcnt(n). Two things silently undo that
and neither changes a result: an s_waitcnt vmcnt(0) the compiler places inside the loop (in front of a read it takes for one that
may alias the DMA: the builtin transposing read was one, lfi_pgemm.hip pg_frag_tr_asm), and a register spill inside the loop
(scratch loads ride the same counter, and the compiler waits vmcnt(0) for them). Neither may appear between the barriers of the pair
loop of the six instantiations the training step launches."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEP_KERNELS = [
    "gemm_planes16t_kernel<true, false, 4, 2, 0>",          # cond_transform weight gradient
    "gemm_planes16t_kernel<false, false, 2, 4, 0>",         # feature gradient
    "gemm_planes16t_kernel<false, true, 2, 4, 4>",          # dpre
    "gemm_planes16t_kernel<true, false, 2, 4, 0>",          # dW_c
    "gemm_planes16_kernel<false, false, false, 2, 4, 3>",   # cond_transform forward
    "gemm_planes16_kernel<false, false, false, 4, 2, 0>",   # gic
]


@pytest.fixture(scope="module")
def loops():
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    import main_loop_waits
    asm = main_loop_waits.unit_asm(os.path.join(ROOT, "lets_face_it_amd", "csrc", "lfi_pgemm.hip"), [])
    return {name: (lines, flags) for name, lines, flags in main_loop_waits.analyse(asm, "gemm_planes16")}


@pytest.mark.parametrize("kernel", STEP_KERNELS)
def test_pair_loop_has_no_full_drain_and_no_scratch(loops, kernel):
    assert kernel in loops, "not built: %s (have %s)" % (kernel, sorted(loops))
    lines, flags = loops[kernel]
    print(kernel)
    for ln in lines:
        print("   ", ln)
    # a pair is two phases, the loop is unrolled by three: six spans, every one with DMA, MFMAs and a counted wait at its barrier
    assert len(lines) == 6, lines
    for ln in lines:
        assert "DMA" in ln and "M" in ln and "vm(" in ln and ln.endswith("| barrier"), ln
    assert "vmcnt(0)" not in flags, "s_waitcnt vmcnt(0) inside the pair loop of %s" % kernel
    assert "scratch" not in flags, "scratch access inside the pair loop of %s" % kernel


def test_the_tool_sees_the_drain_where_it_is(loops):
    """(the check above is not vacuous: the builtin form of the same loop has the drain, and the tool reports it)"""
    lines, flags = loops["gemm_planes16t_builtin_kernel<true, false, 4, 2, 0>"]
    assert "vmcnt(0)" in flags
    assert sum("vm(0)" in ln for ln in lines) == 6
