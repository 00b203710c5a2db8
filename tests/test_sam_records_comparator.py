"""scripts/sam_records_comparator.c is the side scripts/sam_records_timing.py measures awfmGpuSamRecords against: the snprintf loop at
the end of examples/read_sam.c on several threads.  It must write real SAM lines, or the comparison is worth nothing: on an
unpaired batch without names, qualities, mapping qualities, second scores and flags, whose unaligned reads are those without a
score, its lines are the host twin's byte for byte, for 1 and for 5 threads.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_records_common as sm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 512


class NameTable(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("chars", C.c_void_p), ("numRecords", C.c_uint64)]


class ComparatorInputs(C.Structure):
    _fields_ = [("readChars", C.c_void_p), ("readOffsets", C.c_void_p), ("sequences", C.c_void_p), ("slots", C.c_void_p), ("scores", C.c_void_p),
                ("editDistances", C.c_void_p), ("textBegins", C.c_void_p), ("cigarOffsets", C.c_void_p), ("cigarChars", C.c_void_p),
                ("mdOffsets", C.c_void_p), ("mdChars", C.c_void_p), ("numReads", C.c_uint64), ("maxCandidates", C.c_uint32), ("lookup", C.c_void_p),
                ("lookupUser", C.c_void_p), ("out", C.c_void_p), ("stride", C.c_uint64), ("written", C.c_void_p), ("firstRead", C.c_void_p)]


def test_comparator_writes_the_host_twins_lines(awfm, tmp_path):
    so = str(tmp_path / "sam_records_comparator.so")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-pthread",
                           os.path.join(ROOT, "scripts", "sam_records_comparator.c"), "-o", so])
    lib = C.CDLL(so)
    lib.samComparator.argtypes, lib.samComparator.restype = [C.POINTER(ComparatorInputs), C.c_uint], C.c_int
    rng = np.random.default_rng(5)
    reads = [sm.read(rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(rng.integers(1, 160))).tobytes(), score=int(rng.integers(0, 4)) * 40,
                     nm=int(rng.integers(0, 9)), slot=int(rng.integers(0, 2)), records=(int(rng.integers(0, 4)), int(rng.integers(0, 4))),
                     begin=int(rng.integers(0, 1 << 33)), cigar=b"" if r % 7 == 0 else b"%dM" % r, md=b"" if r % 5 == 0 else b"%dA0" % r)
             for r in range(301)]
    batch = sm.Batch(reads, without=("names", "qualities", "mappingQualities", "secondScores", "baseFlags", "properPairs"))
    want = sm.lines_of(batch)
    twin = awfm.sam_records_host(batch.arrays, max_candidates=batch.C)
    assert awfm.strings_of(twin["lineOffsets"], twin["lineChars"]) == want and 0 < twin["numUnaligned"] < batch.n
    a = {name: np.ascontiguousarray(v) for name, v in batch.arrays.items() if v is not None}
    table = NameTable(a["recordNameOffsets"].ctypes.data, a["recordNameChars"].ctypes.data, len(sm.RECORD_NAMES))
    for threads in (1, 5):
        out, written, first = np.zeros(batch.n * STRIDE, np.uint8), np.zeros(threads, np.uint64), np.zeros(threads, np.uint64)
        inputs = ComparatorInputs(*(a[name].ctypes.data for name in ("readChars", "readOffsets", "sequences", "slots", "scores", "editDistances",
                                                                      "textBegins", "cigarOffsets", "cigarChars", "mdOffsets", "mdChars")),
                                  batch.n, batch.C, C.cast(lib.samComparatorTableLookup, C.c_void_p).value, C.addressof(table), out.ctypes.data, STRIDE,
                                  written.ctypes.data, first.ctypes.data)
        assert lib.samComparator(C.byref(inputs), threads) == 1
        got = b"".join(out[int(first[t]) * STRIDE:int(first[t]) * STRIDE + int(written[t])].tobytes() for t in range(threads))
        assert got == b"".join(want), threads
