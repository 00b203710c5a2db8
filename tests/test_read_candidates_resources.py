"""Compile-time conditions on the kernels of awfmGpuReadCandidates (csrc/awfm_candidates_kernel.h), cross-compiled for gfx950
like tests/test_local_positions_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills
or has a private segment, and the two tiers stay within the LDS and the registers that DESIGN.md 4h declares -- the wave tier
4.5 KB of LDS and 64 VGPRs (workgroups of one wave, eight per SIMD), the workgroup tier 58 KB (<= 80 KB: two workgroups per CU)
and 128 VGPRs (its two workgroups of eight waves are four waves per SIMD)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

DECLARED = {"readCandidatesWaveKernel": {"lds": "kCandidatesWaveLdsBytes", "lds_at_most": 8 * 1024, "vgpr": 64, "threads": "kCandidatesWaveThreads"},
            "readCandidatesGroupKernel": {"lds": "kCandidatesGroupLdsBytes", "lds_at_most": 80 * 1024, "vgpr": 128, "threads": "kCandidatesGroupThreads"}}


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_candidates.hip")


def _constant(name):
    return km.constant(name, "awfm_candidates_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum(any(k in name for k in DECLARED) for name in metadata) == 2, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("kernel", sorted(DECLARED))
def test_tiers_stay_within_the_declared_lds_and_registers(metadata, kernel):
    (name,) = [n for n in metadata if kernel in n]
    declared, k = DECLARED[kernel], metadata[name]
    lds = _constant(declared["lds"])
    assert k["lds"] <= lds <= declared["lds_at_most"], (k, lds)  # all of it static: the kernels are launched without dynamic LDS
    assert k["vgpr"] <= declared["vgpr"], k
    assert k["threads"] == _constant(declared["threads"]), k
    entry = _constant("kCandidatesEntryBytes")
    limit = _constant("kCandidatesWaveLimit" if "Wave" in kernel else "kCandidatesGroupLimit")
    assert limit * entry <= k["lds"] <= limit * entry + 1024, (k, limit, entry)  # the kept hits, and a few words of slots
