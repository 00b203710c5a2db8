"""Compile-time conditions on the kernels of awfmGpuReadChains (csrc/awfm_chains_kernel.h), cross-compiled for gfx950 like
tests/test_read_candidates_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills or
has a private segment, and the two tiers stay within the LDS and the registers that DESIGN.md 4i declares -- the wave tier
5.25 KB of static LDS and 64 VGPRs (workgroups of one wave, eight per SIMD), the workgroup tier 65 KB of dynamic LDS on top of a
few static words (<= 80 KB in all: two workgroups per CU) and 128 VGPRs (its two workgroups of eight waves are four waves per
SIMD)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_metadata_common as km  # noqa: E402

DECLARED = {"readChainsWaveKernel": {"lds": "kChainsWaveLdsBytes", "lds_at_most": 8 * 1024, "vgpr": 64, "threads": "kChainsWaveThreads", "dynamic": False},
            "readChainsGroupKernel": {"lds": "kChainsGroupLdsBytes", "lds_at_most": 80 * 1024, "vgpr": 128, "threads": "kChainsGroupThreads", "dynamic": True}}


@pytest.fixture(scope="module")
def metadata():
    return km.metadata("awfm_gpu_chains.hip")


def _constant(name):
    return km.constant(name, "awfm_chains_kernel.h")


def test_no_kernel_of_the_unit_spills_or_uses_scratch(metadata):
    assert sum(any(k in name for k in DECLARED) for name in metadata) == 2, list(metadata)
    for name, k in metadata.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)


@pytest.mark.parametrize("kernel", sorted(DECLARED))
def test_tiers_stay_within_the_declared_lds_and_registers(metadata, kernel):
    (name,) = [n for n in metadata if kernel in n]
    declared, k = DECLARED[kernel], metadata[name]
    lds = _constant(declared["lds"])
    entry = _constant("kChainsEntryBytes")
    limit = _constant("kChainsWaveLimit" if "Wave" in kernel else "kChainsGroupLimit")
    assert k["dynamic"] == declared["dynamic"], k
    assert k["vgpr"] <= declared["vgpr"], k
    assert k["threads"] == _constant(declared["threads"]), k
    assert limit * entry <= lds <= limit * entry + 1280, (lds, limit, entry)  # the anchors, and a few words of slots
    if declared["dynamic"]:  # what the launch asks for on top of the kernel's static words: two workgroups share a CU's 160 KB
        assert k["lds"] <= 1024 and k["lds"] + lds <= declared["lds_at_most"] and 2 * (k["lds"] + lds) <= 160 * 1024, (k, lds)
    else:  # all of it static: the kernel is launched without dynamic LDS
        assert limit * entry <= k["lds"] <= lds <= declared["lds_at_most"], (k, lds)
