"""Compile-time conditions on the kernels of csrc/awfm_gpu_score_affine.hip (awfm_score_affine_kernel.h), cross-compiled for gfx950
like tests/test_align_affine_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills,
vector or scalar, or has a private segment, and the three instantiations of the slot scoring kernel stay within what DESIGN.md
4m declares -- 72 VGPRs (seven waves per SIMD: a workgroup is four waves, seven workgroups per CU; the parameters stay in the
argument segment and are loaded where they are used, so that neither scalar nor vector registers hold them for the kernel's
whole life) and kScoreLdsBytes of static LDS (the staging words of the sixteen groups of 16 lanes, the amino letter table and
the slot words of the four waves: LDS never limits the occupancy).  The grid is sized from the same waves per CU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_VGPRS = 72


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_score_affine.hip")


def _constant(name, header="awfm_score_affine_kernel.h"):
    return km.constant(name, header)


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("scoreChainsAffineKernel" in name for name in metadata) == 3, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_slot_scoring_stays_within_the_declared_lds_and_registers(metadata, group):
    (name,) = [n for n in metadata if "scoreChainsAffineKernelILi%dE" % group in n]
    k = metadata[name]
    threads, lds, per_cu = _constant("kScoreThreads"), _constant("kScoreLdsBytes"), _constant("kScoreBlocksPerCU")
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] <= SCORE_VGPRS and 512 // SCORE_VGPRS * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
    groups, words = threads // group, _constant("kVerifyGroupWords", "awfm_band_kernel.h")
    slot_bytes = (threads // 64) * _constant("kScoreSlotWords") * 4
    assert groups * words * 4 + slot_bytes <= k["lds"] <= groups * words * 4 + slot_bytes + 64 and k["lds"] <= lds, (k, lds)
    assert per_cu * lds <= 160 * 1024


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4m."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert f"{SCORE_VGPRS} VGPRs" in section and f"{_constant('kScoreLdsBytes')} bytes" in section and "seven waves per SIMD" in section
