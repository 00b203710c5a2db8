"""Compile-time conditions on the kernels of csrc/awfm_gpu_verify.hip (awfm_verify_kernel.h), cross-compiled for gfx950 like
tests/test_read_chains_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills or has
a private segment, and the verification kernels stay within what DESIGN.md 4j declares -- 80 VGPRs (six waves per SIMD: a
workgroup is four waves with a read each, six workgroups per CU; the slot arrays' addresses are kept in vector registers so
that no scalar register spills) and kVerifyLdsBytes of static LDS (the staging words of the sixteen groups of 16 lanes and the
amino letter table: LDS never limits the occupancy); the recall kernel uses no LDS and at most 64 VGPRs."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERIFY_VGPRS, WINDOW_VGPRS = 80, 64


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_verify.hip")


def _constant(name, header="awfm_verify_kernel.h"):
    return km.constant(name, header)


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("verifyChainsKernel" in name for name in metadata) == 3 and sum("textWindowsKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_verification_stays_within_the_declared_lds_and_registers(metadata, group):
    (name,) = [n for n in metadata if "verifyChainsKernelILi%dE" % group in n]
    k = metadata[name]
    threads, lds, per_cu = _constant("kVerifyThreads"), _constant("kVerifyLdsBytes"), _constant("kVerifyBlocksPerCU")
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] <= VERIFY_VGPRS and 512 // VERIFY_VGPRS * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
    groups = threads // group
    assert groups * _constant("kVerifyGroupWords", "awfm_band_kernel.h") * 4 <= k["lds"] <= groups * _constant("kVerifyGroupWords", "awfm_band_kernel.h") * 4 + 64 and k["lds"] <= lds, (k, lds)
    assert per_cu * lds <= 160 * 1024


def test_recall_uses_no_lds(metadata):
    (name,) = [n for n in metadata if "textWindowsKernel" in n]
    k = metadata[name]
    assert k["lds"] == 0 and not k["dynamic"] and k["vgpr"] <= WINDOW_VGPRS and k["threads"] == _constant("kWindowThreads"), k
