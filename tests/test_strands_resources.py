"""Compile-time conditions on the kernels of csrc/awfm_gpu_strands.hip (awfm_strands_kernel.h), cross-compiled for gfx950 like
tests/test_pair_mates_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills, vector
or scalar, or has a private segment; the kernels stay within what DESIGN.md 4u declares -- the 32 lanes a pair and both per-read
instantiations within 128 VGPRs (four waves per SIMD: a workgroup is four waves, four workgroups per CU), the wave per pair
within 256 (two waves per SIMD, two workgroups per CU), the orienting gather within 64 (eight waves per SIMD), none with any
LDS --; and the grids are sized from the constants 4u names."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_strands.hip")


def _constant(name):
    return km.constant(name, "awfm_strands_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("chooseStrandPairsKernel" in name for name in metadata) == 2, list(metadata)
    assert sum("chooseStrandReadsKernel" in name for name in metadata) == 2, list(metadata)
    assert sum("orientReadsKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_kernels_stay_within_the_declared_lds_and_registers(metadata):
    threads, lds = _constant("kStrandThreads"), _constant("kStrandLdsBytes")
    narrow = (_constant("kStrandBlocksPerCU"), _constant("kStrandMaxVgprs"), 128)
    wide = (_constant("kStrandWaveBlocksPerCU"), _constant("kStrandWaveMaxVgprs"), 256)
    seen = 0
    for name, k in metadata.items():
        if "chooseStrand" not in name:
            continue
        per_cu, vgprs, declared = wide if "chooseStrandPairsKernelILi64E" in name else narrow
        assert not k["dynamic"] and k["threads"] == threads == 256, k
        assert k["vgpr"] + k["agpr"] <= vgprs == declared and 512 // vgprs * 4 == per_cu * (threads // 64), (name, k)  # waves per SIMD x 4 SIMDs
        assert k["lds"] == lds == 0, k
        seen += 1
    assert seen == 4
    (name,) = [n for n in metadata if "orientReadsKernel" in n]
    k = metadata[name]
    threads, per_cu, vgprs = (_constant(c) for c in ("kOrientThreads", "kOrientBlocksPerCU", "kOrientMaxVgprs"))
    assert not k["dynamic"] and k["threads"] == threads == 256 and k["lds"] == 0, k
    assert k["vgpr"] + k["agpr"] <= vgprs == 64 and 512 // vgprs * 4 == per_cu * (threads // 64), k


def test_grids_are_sized_from_the_same_numbers():
    unit = open(os.path.join(CSRC, "awfm_gpu_strands.hip")).read()
    assert "perBlock = kStrandThreads / group" in unit
    assert "(uint64_t)g->numCUs * (paired && group == 64u ? kStrandWaveBlocksPerCU : kStrandBlocksPerCU);" in unit
    assert "perBlock = kOrientThreads / 64u" in unit and "(uint64_t)g->numCUs * kOrientBlocksPerCU;" in unit
    kernel = open(os.path.join(CSRC, "awfm_strands_kernel.h")).read()
    assert "__launch_bounds__(kStrandThreads, G == 64 ? 2 : 4) chooseStrandPairsKernel" in kernel
    assert "__launch_bounds__(kStrandThreads, 4) chooseStrandReadsKernel" in kernel and "__launch_bounds__(kOrientThreads, 8)" in kernel


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4u."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "128 VGPRs" in section and "four waves per SIMD" in section and "no LDS" in section
    assert "256 VGPRs" in section and "two waves per SIMD" in section and "64 VGPRs" in section
    for constant in ("kStrandBlocksPerCU", "kStrandWaveBlocksPerCU", "kOrientBlocksPerCU"):
        assert constant in section, constant
