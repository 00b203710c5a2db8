"""Compile-time conditions on the kernel of csrc/awfm_gpu_window_affine.hip (awfm_window_affine_kernel.h), cross-compiled for gfx950
like tests/test_score_chains_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills,
vector or scalar, or has a private segment, and the window scoring kernel -- one kernel that holds the three instantiations of
its row, 4, 8 and 12 columns a lane, behind a wave-uniform switch -- stays within what DESIGN.md 4n declares: 128 VGPRs (four
waves per SIMD: a workgroup is four waves, four workgroups per CU) and kWinAffLdsBytes of static LDS (per wave 64 boundary entries
and 64 read words, and the amino letter table: LDS never limits the occupancy).  The grid and the scratch are sized from the same
waves per CU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_window_affine.hip")


def _constant(name, header="awfm_window_affine_kernel.h"):
    return km.constant(name, header)


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum("scoreWindowsAffineKernel" in name for name in metadata) == 1, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


def test_window_scoring_stays_within_the_declared_lds_and_registers(metadata):
    (name,) = [n for n in metadata if "scoreWindowsAffineKernel" in n]
    k = metadata[name]
    threads, lds, per_cu, vgprs = (_constant(c) for c in ("kWinAffThreads", "kWinAffLdsBytes", "kWinAffBlocksPerCU", "kWinAffMaxVgprs"))
    assert not k["dynamic"] and k["threads"] == threads == 256, k
    assert k["vgpr"] + k["agpr"] <= vgprs == 128 and 512 // vgprs * 4 == per_cu * (threads // 64), k  # waves per SIMD x 4 SIMDs = the grid's waves per CU
    waves = threads // 64
    assert k["lds"] == lds == waves * 64 * (_constant("kWinAffEntryBytes") + 4) + 32, (k, lds)
    assert per_cu * lds <= 160 * 1024


def test_grid_and_scratch_are_sized_from_the_same_numbers():
    unit = open(os.path.join(CSRC, "awfm_gpu_window_affine.hip")).read()
    assert "g->numCUs * kWinAffBlocksPerCU * (kWinAffThreads / 64u)" in unit      # the arena's waves
    assert "(uint64_t)g->numCUs * kWinAffBlocksPerCU;" in unit                      # the grid's resident workgroups
    assert "windowGridWaves(g) * 2ull * kWinAffEntryBytes * maxLength" in unit
    kernel = open(os.path.join(CSRC, "awfm_window_affine_kernel.h")).read()
    assert "__launch_bounds__(kWinAffThreads, 4)" in kernel and _constant("kWinAffMaxQ") == 12


def test_design_declares_these_numbers():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 4n."):]
    section = section[:section.index("\n## ") if "\n## " in section else len(section)]
    assert "128 VGPRs" in section and f"{_constant('kWinAffLdsBytes')} bytes" in section and "four waves per SIMD" in section
