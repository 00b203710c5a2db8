"""Compile-time conditions on oneSubstitutionKernel (csrc/awfm_subst_kernel.h), cross-compiled for gfx950 like
tests/test_longest_match_resources.py (no GPU needed): no instantiation spills a vector or scalar register or uses scratch, and
each keeps the vector registers of the occupancy DESIGN.md 4g declares for it (512 registers per SIMD lane, allocated in eights:
80 -> 6 waves per SIMD, 96 -> 5, 128 -> 4); the static LDS is a few KB, so that LDS does not limit the workgroups per CU below
what the registers allow."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# <AMINO, NARROW, TABLES> -> most vector registers: the waves per SIMD DESIGN.md 4g declares
PLANNED = {
    "ILb0ELb1ELb0EE": 80,   # nucleotide, 32-bit positions, the plain path: 6 waves
    "ILb0ELb0ELb0EE": 80,   # ... 64-bit positions: 6 waves
    "ILb0ELb1ELb1EE": 96,   # table gathers, 32-bit positions: 5 waves (the uniform values that live in vector registers)
    "ILb0ELb0ELb1EE": 128,  # table gathers, 64-bit positions: 4 waves
    "ILb1ELb1ELb0EE": 80,   # amino: 6 waves
    "ILb1ELb0ELb0EE": 80,
}


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "awfm_gpu_subst.s"
    subprocess.check_call([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "-Wno-unused-function", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "awfm_gpu_subst.hip")])
    return out.read_text()


def _metadata(text):
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text):
        meta[m.group(2)] = {"lds": int(m.group(1)), "scratch": int(m.group(3)), "sgpr_spill": int(m.group(4)),
                            "vgpr": int(m.group(5)), "spill": int(m.group(6))}
    return meta


def _body(text, symbol):
    start = text.index("\n" + symbol + ":")
    return text[start:text.index(".Lfunc_end", start)]


def test_every_instantiation_spills_nothing_and_keeps_its_occupancy(assembly):
    everything = _metadata(assembly)
    # tests/test_kernel_resources.py and tests/test_longest_match_resources.py match their kernels' symbols by name
    assert all("searchKernel" not in n and "walkKernel" not in n for n in everything)
    kernels = {n: v for n, v in everything.items() if "oneSubstitutionKernel" in n}
    found = {}
    for name, k in kernels.items():
        key = name[name.index("KernelILb") + len("Kernel"):][:14]
        found[key] = name
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= PLANNED[key], (name, k)
        assert k["lds"] <= 8 * 1024, (name, k)
        body = _body(assembly, name)
        assert "scratch_" not in body and "v_writelane" not in body, name
    assert sorted(found) == sorted(PLANNED), sorted(found)
    fill = [v for n, v in everything.items() if "oneSubstitutionFillKernel" in n]
    assert len(fill) == 1 and fill[0]["spill"] == 0 and fill[0]["sgpr_spill"] == 0 and fill[0]["scratch"] == 0
