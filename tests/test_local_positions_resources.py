"""Compile-time conditions on the two lookups of the mapping kernel (csrc/awfm_records_kernel.h), cross-compiled for gfx950
like tests/test_kernel_resources.py (no GPU needed): neither spills nor uses scratch; the LDS lookup's static plus largest
dynamic LDS leaves two workgroups per CU (<= 80 KB of the CU's 160 KB) and its table reads are LDS reads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("isa") / "awfm_gpu_records.s"
    subprocess.check_call([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, "-Wno-unused-function", "-S", "--cuda-device-only", "-o", str(out),
                           os.path.join(CSRC, "awfm_gpu_records.hip")], stderr=subprocess.DEVNULL)
    return out.read_text()


def _metadata(text):
    meta = {}
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                         r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                         r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text):
        meta[m.group(2)] = {"lds": int(m.group(1)), "scratch": int(m.group(3)), "sgpr_spill": int(m.group(4)),
                            "vgpr": int(m.group(5)), "spill": int(m.group(6))}
    return meta


def _constant(name):
    header = open(os.path.join(CSRC, "awfm_records_kernel.h")).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", header).group(1))


def _body(text, symbol):
    """the instructions of one kernel"""
    start = text.index("\n" + symbol + ":")
    return text[start:text.index(".Lfunc_end", start)]


def test_both_lookups_spill_nothing_and_use_no_scratch(assembly):
    meta = _metadata(assembly)
    kernels = {n: v for n, v in meta.items() if "localPositionsKernel" in n}
    assert sorted(n[n.index("KernelILb"):][:12] for n in kernels) == ["KernelILb0EE", "KernelILb1EE"], list(kernels)
    for name, k in kernels.items():
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k)
        assert k["vgpr"] <= 64, (name, k)  # 512-thread workgroups at full occupancy
    for name in kernels:
        assert "scratch_" not in _body(assembly, name), name


def test_lds_lookup_leaves_two_workgroups_per_cu(assembly):
    meta = _metadata(assembly)
    (name,) = [n for n in meta if "localPositionsKernelILb1EE" in n]
    dynamic = _constant("kRecordLdsMaxRecords") * 8 + (_constant("kRecordLdsMaxBuckets") + 1) * 4
    assert meta[name]["lds"] + dynamic <= 80 * 1024, (meta[name], dynamic)
    body = _body(assembly, name)
    assert "ds_read_b64" in body  # the 8-byte ends come out of LDS in one read each
    (other,) = [n for n in meta if "localPositionsKernelILb0EE" in n]
    assert "ds_read" not in _body(assembly, other)
