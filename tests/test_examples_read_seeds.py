"""examples/read_seeds.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
FASTA -> index -> awfmGpuLongestSuffixMatches over the windows ending at every s-th position of every read -> hit offsets ->
awfmGpuLocate -> awfmGpuLocalPositions -> `read:end:length:header:offset` per occurrence.  Without a GPU it must fail loudly; on
the GPU its lines must be what the host gives: awfmLongestSuffixMatches, the host's own locate of every row of the range,
awfmLocalPositions and the headers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import longest_match_common as lm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP, MIN_LENGTH, CAP = 4, 14, 64


def _compile(tmp_path):
    exe = str(tmp_path / "read_seeds")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_seeds.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _inputs(tmp_path):
    """records from a seed; reads = pieces of 100-150 characters of the longer records with 5 % substitutions, some random ones"""
    lengths = lp.record_lengths(43, count=200, longest=1500)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    rng = np.random.default_rng(6)
    long_enough = [r for r in records if len(r) >= 200]
    reads = []
    for i in range(120):
        m = int(rng.integers(100, 151))
        if i % 10 == 9:
            reads.append(lm.random_text(rng, m, lm.DNA))
            continue
        r = long_enough[int(rng.integers(0, len(long_enough)))]
        at = int(rng.integers(0, len(r) - m + 1))
        reads.append(lm.mutate(rng, r[at:at + m], lm.DNA, 0.05))
    reads.append(lm.random_text(rng, 70000, lm.DNA))  # longer than any line buffer: still one read
    reads.append(b"acg")  # shorter than a step: no window
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    return fa, reads


def test_read_seeds_example_compiles_and_fails_loudly_without_a_gpu(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    exe = _compile(tmp_path)  # against the two public headers, warnings as errors
    if _lib.lib().awfmGpuDeviceCount() > 0:
        return  # what it prints on a GPU is the next test's
    _inputs(tmp_path)
    out = subprocess.run([exe, "records.fa", "reads.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "no CPU search path" in out.stderr and out.stdout == ""


@pytest.mark.gpu
def test_read_seeds_example_prints_what_the_host_twin_finds(awfm, require_gpu, tmp_path):
    from avxwindowfmindex_amd import _lib
    fa, reads = _inputs(tmp_path)
    out = subprocess.run([_compile(tmp_path), "records.fa", "reads.txt", str(STEP), str(MIN_LENGTH), str(CAP)], cwd=tmp_path,
                         capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    chars = np.frombuffer(b"".join(reads), np.uint8)
    read_at = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    windows = [(r, e) for r, read in enumerate(reads) for e in range(STEP, len(read) + 1, STEP)]
    starts = np.array([read_at[r] + max(e - CAP, 0) for r, e in windows], np.uint64)
    ends = np.array([read_at[r] + e for r, e in windows], np.uint64)
    lengths, ranges, counts = awfm.longest_suffix_matches_host(ix, chars, starts, ends, min_length=MIN_LENGTH)
    L = _lib.lib()
    want, illegal = [], 0
    for (r, e), length, (sp, ep), count in zip(windows, lengths, ranges, counts):
        if count == 0:
            continue
        ok = C.c_int(0)
        rows = np.array([L.awFmFindDatabaseHitPositionSingle(ix.ptr, int(p), C.byref(ok)) for p in range(int(sp), int(ep) + 1)], np.uint64)
        seq, local, bad = awfm.local_positions_host(ix, rows)
        illegal += bad
        for s, p in zip(seq, local):
            where = b"*" if s == lp.ILLEGAL else ix.header(int(s))
            want.append(b"%d:%d:%d:%s:%d" % (r, e, int(length), where, int(p)))
    assert len(want) > 500 and (lengths[counts > 0] >= MIN_LENGTH).all() and (counts == 0).any()
    assert out.stdout.split(b"\n")[:-1] == want
    assert f"reads {len(reads)} windows {len(windows)} occurrences {len(want)} illegal {illegal}".encode() in out.stderr
    ix.dealloc()
