"""Compile-time conditions on the kernels of csrc/awfm_gpu_sam.hip (awfm_sam_kernel.h), cross-compiled for gfx950 like
tests/test_longest_match_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills, vector
or scalar, or has a private segment; the write kernel has exactly a tile of kSamTileWords words per wave of static LDS -- the
8192 bytes DESIGN.md 4t names -- and the lengths kernel none; both stay within kSamMaxVgprs; and the launcher allocates nothing,
waits for nothing and scans with the library's scan."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_sam.hip")


def _constant(name):
    return km.constant(name, "awfm_sam_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("samLengthsKernel" in name for name in metadata) == 1, list(metadata)
    assert sum("samWriteKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():  # (and the kernels awfm_device.h brings into every unit)
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_kernels_stay_within_the_declared_lds_and_registers(metadata):
    threads, tile, words, lds, vgprs, fields = (_constant(c) for c in ("kSamThreads", "kSamTileBytes", "kSamTileWords", "kSamLdsBytes", "kSamMaxVgprs",
                                                                       "kSamFields"))
    assert threads == 256 and tile == 2048 and words * 4 == tile and lds == (threads // 64) * words * 4 == 8192
    assert vgprs == 64 and 512 // vgprs == 8 and 8 * 4 // (threads // 64) * lds <= 160 * 1024  # eight waves a SIMD, and the LDS allows them
    assert fields == 15 and fields < 16  # the prefix sum over the fields runs over sixteen lanes
    for name, k in [(n, k) for n, k in metadata.items() if "samLengthsKernel" in n or "samWriteKernel" in n]:
        want = lds if "samWriteKernel" in name else 0
        assert not k["dynamic"] and k["threads"] == threads and k["lds"] == want, (name, k)
        assert k["vgpr"] + k["agpr"] <= vgprs, (name, k)


def test_launcher_allocates_nothing_waits_for_nothing_and_uses_the_librarys_scan():
    unit = open(os.path.join(CSRC, "awfm_gpu_sam.hip")).read()
    assert "hipMalloc" not in unit and "Synchronize" not in unit  # no allocation, no host wait
    assert "awfmGpuScanCounts(" in unit and "awfmGpuScanScratchBytes(numReads)" in unit  # the library's scan, not a second one
    assert 'awfmGpuDiag("sam_tier")' in unit  # the diagnostics key, no new environment variable
    assert "getenv" not in unit


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4t."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "kSamTileBytes" in section and "2048 bytes" in section and "kSamLdsBytes" in section and "8192 bytes" in section
    assert "kSamMaxVgprs" in section and "64 VGPRs" in section and "kSamThreads" in section and "no spill" in section
