"""Compile-time conditions on the kernels of csrc/awfm_gpu_align.hip (awfm_align_kernel.h), cross-compiled for gfx950 like
tests/test_verify_chains_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills,
vector or scalar, or has a private segment, and the three instantiations of the alignment kernel stay within what DESIGN.md 4k
declares -- 128 VGPRs (four waves per SIMD: a workgroup is four waves, four workgroups per CU; the arguments are kept in vector
registers so that no scalar register spills) and kAlignLdsBytes of static LDS (the staging words of the sixteen groups of 16
lanes and the amino letter table: LDS never limits the occupancy).  The grid and the trace arena are sized from the same
waves per CU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_VGPRS = 128


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_align.hip")


def _constant(name, header="awfm_align_kernel.h"):
    return km.constant(name, header)


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("alignChainsKernel" in name for name in metadata) == 3, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_alignment_stays_within_the_declared_lds_and_registers(metadata, group):
    (name,) = [n for n in metadata if "alignChainsKernelILi%dE" % group in n]
    k = metadata[name]
    threads, lds, per_cu = _constant("kAlignThreads"), _constant("kAlignLdsBytes"), _constant("kAlignBlocksPerCU")
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] <= ALIGN_VGPRS and 512 // ALIGN_VGPRS * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
    groups, words = threads // group, _constant("kVerifyGroupWords", "awfm_band_kernel.h")
    assert groups * words * 4 <= k["lds"] <= groups * words * 4 + 64 and k["lds"] <= lds, (k, lds)
    assert per_cu * lds <= 160 * 1024


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4k."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert f"{ALIGN_VGPRS} VGPRs" in section and f"{_constant('kAlignLdsBytes')} bytes" in section and "four waves per SIMD" in section
