"""Compile-time conditions on the kernels of csrc/awfm_gpu_pair_mates.hip (awfm_pair_mates_kernel.h), cross-compiled for gfx950 like
tests/test_window_scores_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills, vector
or scalar, or has a private segment; both instantiations of the pairing kernel stay within what DESIGN.md 4o declares -- 128
VGPRs (four waves per SIMD: a workgroup is four waves, four workgroups per CU) and no LDS at all --, the reverse complement within
64 VGPRs (eight waves per SIMD) and no LDS; and the grids are sized from the constants 4o names."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_pair_mates.hip")


def _constant(name, header="awfm_pair_mates_kernel.h"):
    return km.constant(name, header)


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("pairMatesKernel" in name for name in metadata) == 2, list(metadata)
    assert sum("reverseComplementKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_kernels_stay_within_the_declared_lds_and_registers(metadata):
    threads, lds, per_cu, vgprs = (_constant(c) for c in ("kPairThreads", "kPairLdsBytes", "kPairBlocksPerCU", "kPairMaxVgprs"))
    for name in [n for n in metadata if "pairMatesKernel" in n]:
        k = metadata[name]
        assert not k["dynamic"] and k["threads"] == threads == 256, k
        assert k["vgpr"] + k["agpr"] <= vgprs == 128 and 512 // vgprs * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
        assert k["lds"] == lds == 0, k
    (name,) = [n for n in metadata if "reverseComplementKernel" in n]
    k = metadata[name]
    threads, per_cu, vgprs = (_constant(c) for c in ("kComplementThreads", "kComplementBlocksPerCU", "kComplementMaxVgprs"))
    assert not k["dynamic"] and k["threads"] == threads == 256 and k["lds"] == 0, k
    assert k["vgpr"] + k["agpr"] <= vgprs == 64 and 512 // vgprs * 4 == per_cu * (threads // 64), k


def test_grids_are_sized_from_the_same_numbers():
    unit = open(os.path.join(CSRC, "awfm_gpu_pair_mates.hip")).read()
    assert "perBlock = kPairThreads / group" in unit and "(uint64_t)g->numCUs * kPairBlocksPerCU;" in unit
    assert "perBlock = kComplementThreads / 64u" in unit and "(uint64_t)g->numCUs * kComplementBlocksPerCU;" in unit
    kernel = open(os.path.join(CSRC, "awfm_pair_mates_kernel.h")).read()
    assert "__launch_bounds__(kPairThreads, 4)" in kernel and "__launch_bounds__(kComplementThreads, 8)" in kernel


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4o."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "128 VGPRs" in section and "four waves per SIMD" in section and "no LDS" in section
    assert "kPairBlocksPerCU" in section and "kComplementBlocksPerCU" in section and "64 VGPRs" in section
