"""What the *_resources.py tests share: a unit of csrc/ cross-compiled to gfx950 assembly (no GPU needed) and the resource
numbers of every kernel in it, read from the code object's metadata."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

_KERNEL = re.compile(r"- \.agpr_count:\s+(\d+)\n\s+\.args:\n((?:.*\n)*?)\s+\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.max_flat_workgroup_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                     r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?"
                     r"\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)")


def metadata(source):
    """source: a .hip file of csrc/ -> {kernel name: {lds, dynamic, threads, scratch, sgpr_spill, vgpr, agpr, spill}}"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, os.path.splitext(source)[0] + ".s")
        subprocess.check_call([HIPCC, "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-I" + CSRC, "-Wno-unused-function", "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, source)],
                              stderr=subprocess.DEVNULL)
        text = open(out).read()
    return {m.group(5): {"agpr": int(m.group(1)), "dynamic": "hidden_dynamic_lds_size" in m.group(2), "lds": int(m.group(3)),
                         "threads": int(m.group(4)), "scratch": int(m.group(6)), "sgpr_spill": int(m.group(7)), "vgpr": int(m.group(8)),
                         "spill": int(m.group(9))} for m in _KERNEL.finditer(text)}


def constant(name, header):
    """the value of `constexpr unsigned name = N;` in that header of csrc/"""
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", text).group(1))
