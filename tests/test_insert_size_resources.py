"""Compile-time conditions on the kernels of csrc/awfm_gpu_insert.hip (awfm_insert_kernel.h), cross-compiled for gfx950 like
tests/test_pair_mates_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills, vector or
scalar, or has a private segment; the histogram kernel's LDS tier has exactly kInsertLdsBins 32-bit counters of static LDS -- the
32768 bytes DESIGN.md 4p names -- and its global tier none; both stay within 64 VGPRs, as does the interval kernel, whose one
workgroup of 1024 threads has the 400 bytes of LDS 4p names; and the grid is sized from the constants 4p names."""
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
    return km.metadata("awfm_gpu_insert.hip")


def _constant(name):
    return km.constant(name, "awfm_insert_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("insertHistogramKernel" in name for name in metadata) == 2, list(metadata)
    assert sum("insertIntervalKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_kernels_stay_within_the_declared_lds_and_registers(metadata):
    threads, bins, lds, per_cu, vgprs = (_constant(c) for c in ("kInsertThreads", "kInsertLdsBins", "kInsertLdsBytes", "kInsertBlocksPerCU",
                                                                "kInsertMaxVgprs"))
    assert bins == 8192 and lds == bins * 4 == 32768 and per_cu * lds <= CU_LDS_BYTES
    assert vgprs == 64 and per_cu * (threads // 64) <= 512 // vgprs * 4  # the grid's waves per CU fit the registers
    tiers = {"ILb1E": lds, "ILb0E": 0}  # the template argument in the mangled name: the LDS tier, the global tier
    for name in [n for n in metadata if "insertHistogramKernel" in n]:
        k = metadata[name]
        (want,) = [size for tag, size in tiers.items() if tag in name]
        assert not k["dynamic"] and k["threads"] == threads == 256 and k["lds"] == want, (name, k)
        assert k["vgpr"] + k["agpr"] <= vgprs, (name, k)
    (name,) = [n for n in metadata if "insertIntervalKernel" in n]
    k = metadata[name]
    threads, lds, vgprs = (_constant(c) for c in ("kIntervalThreads", "kIntervalLdsBytes", "kIntervalMaxVgprs"))
    assert not k["dynamic"] and k["threads"] == threads == 1024 and k["lds"] == lds == 400, k
    assert k["vgpr"] + k["agpr"] <= vgprs == 64 and 65536 // threads == 64, k  # (the longest chunk a thread sums: 64 bins)


def test_grid_is_sized_from_the_same_numbers():
    unit = open(os.path.join(CSRC, "awfm_gpu_insert.hip")).read()
    assert "(numPairs + kInsertPairsPerBlock - 1u) / kInsertPairsPerBlock;" in unit and "(uint64_t)g->numCUs * kInsertBlocksPerCU;" in unit
    assert "dim3(1), dim3(kIntervalThreads)" in unit and "p.bins <= kInsertLdsBins" in unit
    kernel = open(os.path.join(CSRC, "awfm_insert_kernel.h")).read()
    assert "__launch_bounds__(kInsertThreads)" in kernel and "__launch_bounds__(kIntervalThreads)" in kernel
    assert _constant("kInsertPairsPerBlock") == 4096


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4p."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "kInsertLdsBins" in section and "8192 bins" in section and "32768 bytes" in section and "64 VGPRs" in section
    assert "kInsertBlocksPerCU" in section and "kInsertPairsPerBlock" in section and "4096 pairs" in section
    assert "kIntervalThreads" in section and "1024 threads" in section and "400 bytes" in section and "no spill" in section
