"""Compile-time conditions on the kernels of csrc/awfm_gpu_strings.hip (awfm_strings_kernel.h), cross-compiled for gfx950 like
tests/test_insert_size_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills, vector
or scalar, or has a private segment; the write kernels have exactly a tile of kStringsTileWords words per wave of static LDS --
the 32784 bytes DESIGN.md 4q names -- and the lengths kernels none; all four stay within kStringsMaxVgprs; and the launcher sizes
grid and tiers from the constants 4q names."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
CU_LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_strings.hip")


def _constant(name):
    return km.constant(name, "awfm_strings_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("stringLengthsKernel" in name for name in metadata) == 2, list(metadata)  # 16-byte and dword loads of the rows
    assert sum("stringWriteKernel" in name for name in metadata) == 2, list(metadata)
    for name, k in metadata.items():  # (and the kernels awfm_device.h brings into every unit)
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_kernels_stay_within_the_declared_lds_and_registers(metadata):
    threads, tile, words, lds, vgprs = (_constant(c) for c in ("kStringsThreads", "kStringsTileBytes", "kStringsTileWords", "kStringsLdsBytes",
                                                               "kStringsMaxVgprs"))
    assert threads == 256 and tile == 8192 and words * 4 >= tile + 3 and lds == (threads // 64) * words * 4 == 32784
    assert 4 * lds <= CU_LDS_BYTES < 5 * lds and vgprs == 128 and 4 * (threads // 64) // 4 <= 512 // vgprs  # four workgroups a CU by LDS: four waves a SIMD
    for name, k in [(n, k) for n, k in metadata.items() if "stringLengthsKernel" in n or "stringWriteKernel" in n]:
        want = lds if "stringWriteKernel" in name else 0
        assert not k["dynamic"] and k["threads"] == threads and k["lds"] == want, (name, k)
        assert k["vgpr"] + k["agpr"] <= vgprs, (name, k)


def test_launcher_uses_the_same_numbers():
    unit = open(os.path.join(CSRC, "awfm_gpu_strings.hip")).read()
    assert "(numReads + kStringsThreads - 1u) / kStringsThreads" in unit and "block(kStringsThreads)" in unit
    assert "maxOps % 4u == 0u && ((uintptr_t)dIn->ops & 15u) == 0u" in unit and 'awfmGpuDiag("strings_tier")' in unit
    assert "awfmGpuScanCounts(" in unit and "awfmGpuScanScratchBytes(numReads)" in unit  # the library's scan, not a second one
    kernel = open(os.path.join(CSRC, "awfm_strings_kernel.h")).read()
    assert kernel.count("__launch_bounds__(kStringsThreads)") == 2 and "bytes > kStringsTileBytes || p.direct" in kernel
    assert "tiles[kStringsThreads / 64u][kStringsTileWords]" in kernel


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4q."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "kStringsTileBytes" in section and "8192 bytes" in section and "kStringsLdsBytes" in section and "32784 bytes" in section
    assert "kStringsMaxVgprs" in section and "128 VGPRs" in section and "kStringsThreads" in section and "no spill" in section
