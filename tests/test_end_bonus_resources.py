"""Compile-time conditions on the kernels of csrc/awfm_gpu_score_ends.hip and csrc/awfm_gpu_align_ends.hip
(awfm_end_bonus_kernel.h), cross-compiled for gfx950 like tests/test_matrix_scores_resources.py (no GPU needed), from the code
object's metadata alone: no kernel of either unit spills, vector or scalar, or has a private segment; each unit has exactly its
three instantiations and none of the siblings'; and they stay within what DESIGN.md 4s declares -- the matrix siblings' registers
(72 VGPRs for the score kernel: seven waves per SIMD; 128 for the alignment kernel: four) and the matrix siblings' static LDS: the
bonus is one more word of the launch's arguments and costs no LDS."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_VGPRS, ALIGN_VGPRS = 72, 128
MATRIX_LDS = 21 * 32  # kMatrixLdsBytes: AWFM_MATRIX_CLASSES rows of kMatrixStride bytes


@pytest.fixture(scope="module")
def score_metadata():
    return km.metadata("awfm_gpu_score_ends.hip")


@pytest.fixture(scope="module")
def align_metadata():
    return km.metadata("awfm_gpu_align_ends.hip")


def test_no_kernel_of_either_unit_spills_or_uses_scratch(score_metadata, align_metadata):
    assert sum("scoreChainsEndBonusKernel" in name for name in score_metadata) == 3, list(score_metadata)
    assert sum("alignChainsEndBonusKernel" in name for name in align_metadata) == 3, list(align_metadata)
    for name in list(score_metadata) + list(align_metadata):  # the siblings' kernels stay in their own units
        assert "AffineKernel" not in name and "MatrixKernel" not in name, name
    for name, k in list(score_metadata.items()) + list(align_metadata.items()):
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_the_score_kernel_stays_within_the_declared_lds_and_registers(score_metadata, group):
    (name,) = [n for n in score_metadata if "scoreChainsEndBonusKernelILi%dE" % group in n]
    k = score_metadata[name]
    threads, lds, per_cu = (km.constant(c, "awfm_score_affine_kernel.h") for c in ("kScoreThreads", "kScoreLdsBytes", "kScoreBlocksPerCU"))
    assert km.constant("kMatrixStride", "awfm_band_kernel.h") == 32 and MATRIX_LDS == 672
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] <= SCORE_VGPRS and 512 // SCORE_VGPRS * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
    groups, words = threads // group, km.constant("kVerifyGroupWords", "awfm_band_kernel.h")
    slot_words = km.constant("kScoreSlotWords", "awfm_score_affine_kernel.h")
    own = groups * words * 4 + (threads // 64) * slot_words * 4 + MATRIX_LDS
    assert own <= k["lds"] <= own + 64 and k["lds"] <= lds + MATRIX_LDS, (k, lds)
    assert per_cu * (lds + MATRIX_LDS) <= 160 * 1024


@pytest.mark.parametrize("group", [16, 32, 64])
def test_the_alignment_kernel_stays_within_the_declared_lds_and_registers(align_metadata, group):
    (name,) = [n for n in align_metadata if "alignChainsEndBonusKernelILi%dE" % group in n]
    k = align_metadata[name]
    threads, lds, per_cu = (km.constant(c, "awfm_align_affine_kernel.h") for c in ("kAffineThreads", "kAffineLdsBytes", "kAffineBlocksPerCU"))
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] <= ALIGN_VGPRS and 512 // ALIGN_VGPRS * 4 == per_cu * (threads // 64), k
    groups, words = threads // group, km.constant("kVerifyGroupWords", "awfm_band_kernel.h")
    own = groups * words * 4 + MATRIX_LDS
    assert own <= k["lds"] <= own + 64 and k["lds"] <= lds + MATRIX_LDS, (k, lds)
    assert per_cu * (lds + MATRIX_LDS) <= 160 * 1024


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4s."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    score_lds = km.constant("kScoreLdsBytes", "awfm_score_affine_kernel.h") + MATRIX_LDS
    align_lds = km.constant("kAffineLdsBytes", "awfm_align_affine_kernel.h") + MATRIX_LDS
    assert f"{SCORE_VGPRS} VGPRs" in section and f"{ALIGN_VGPRS} VGPRs" in section
    assert f"{score_lds} bytes" in section and f"{align_lds} bytes" in section
