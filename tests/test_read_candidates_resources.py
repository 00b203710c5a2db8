"""Compile-time conditions on the kernels of awfmGpuReadCandidates (csrc/awfm_candidates_kernel.h), cross-compiled for gfx950
like tests/test_local_positions_resources.py (no GPU needed), from the code object's metadata alone: no kernel of the unit spills
or has a private segment, and the two tiers stay within the LDS and the registers that DESIGN.md 4h declares -- the wave tier
4.5 KB of LDS and 64 VGPRs (workgroups of one wave, eight per SIMD), the workgroup tier 58 KB (<= 80 KB: two workgroups per CU)
and 128 VGPRs (its two workgroups of eight waves are four waves per SIMD)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

DECLARED = {"readCandidatesWaveKernel": {"lds": "kCandidatesWaveLdsBytes", "lds_at_most": 8 * 1024, "vgpr": 64, "threads": "kCandidatesWaveThreads"},
            "readCandidatesGroupKernel": {"lds": "kCandidatesGroupLdsBytes", "lds_at_most": 80 * 1024, "vgpr": 128, "threads": "kCandidatesGroupThreads"}}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "awfm_gpu_candidates.s"
    subprocess.check_call([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "-Wno-unused-function", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "awfm_gpu_candidates.hip")], stderr=subprocess.DEVNULL)
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.max_flat_workgroup_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", out.read_text()):
        meta[m.group(3)] = {"lds": int(m.group(1)), "threads": int(m.group(2)), "scratch": int(m.group(4)), "sgpr_spill": int(m.group(5)),
                            "vgpr": int(m.group(6)), "spill": int(m.group(7))}
    return meta


def _constant(name):
    header = open(os.path.join(CSRC, "awfm_candidates_kernel.h")).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", header).group(1))


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
