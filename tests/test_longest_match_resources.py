"""Compile-time conditions on longestMatchKernel (csrc/awfm_match_kernel.h), cross-compiled for gfx950 like
tests/test_kernel_resources.py (no GPU needed): no instantiation spills a vector or scalar register or uses scratch, and each
keeps the vector registers of the occupancy DESIGN.md 4f plans for it (512 registers per SIMD lane, allocated in eights:
64 -> 8 waves per SIMD, 80 -> 6, 96 -> 5); the static LDS is a few KB, so that LDS does not limit the workgroups per CU
(one wave per SIMD each) below what the registers allow."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# <AMINO, NARROW, PAIR> -> most vector registers: the waves per SIMD the kernel is planned at
PLANNED = {
    "ILb0ELb1ELb0EE": 64,  # nucleotide, 32-bit positions, single steps: 8 waves
    "ILb0ELb0ELb0EE": 80,  # ... 64-bit positions: 6 waves
    "ILb0ELb1ELb1EE": 80,  # pair steps, 32-bit positions (a GRCh38-sized image): 6 waves, what searchKernel's pair instantiation has
    "ILb0ELb0ELb1EE": 96,  # pair steps, 64-bit positions: 5 waves
    "ILb1ELb1ELb0EE": 96,  # amino: 5 waves
    "ILb1ELb0ELb0EE": 96,
}


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "awfm_gpu_match.s"
    subprocess.check_call([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "-Wno-unused-function", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "awfm_gpu_match.hip")], stderr=subprocess.DEVNULL)
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
    kernels = {n: v for n, v in _metadata(assembly).items() if "longestMatchKernel" in n}
    assert all("searchKernel" not in n for n in kernels)  # tests/test_kernel_resources.py matches that kernel's symbols by name
    found = {}
    for name, k in kernels.items():
        key = name[name.index("KernelILb") + len("Kernel"):][:14]
        found[key] = name
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= PLANNED[key], (name, k)
        assert k["lds"] <= 8 * 1024, (name, k)  # with the 12 KB of pair bases of a GRCh38-sized image: six workgroups (6 waves per SIMD) in 120 of the CU's 160 KB
        body = _body(assembly, name)
        assert "scratch_" not in body and "v_writelane" not in body, name
    assert sorted(found) == sorted(PLANNED), sorted(found)
