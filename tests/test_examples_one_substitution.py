"""examples/kmer_neighbours.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
FASTA -> index -> awfmGpuOneSubstitutionSearch over a list of k-mers -> hit offsets -> awfmGpuLocate -> awfmGpuLocalPositions ->
`kmer:edit:header:offset` per occurrence.  Without a GPU it must fail loudly; on the GPU its lines must be what the host gives:
awfmOneSubstitutionSearch, the host's own locate of every row of every record's range, awfmLocalPositions and the headers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import longest_match_common as lm  # noqa: E402
import one_substitution_common as osc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "kmer_neighbours")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "kmer_neighbours.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _inputs(tmp_path):
    """records from a seed; k-mers of 12..40 characters: pieces of the records, most with one substitution, and some random ones"""
    lengths = lp.record_lengths(44, count=150, longest=1200)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 14)
    rng = np.random.default_rng(8)
    long_enough = [r for r in records if len(r) >= 100]
    kmers = []
    for i in range(600):
        m = int(rng.integers(12, 41))
        if i % 10 == 9:
            kmers.append(lm.random_text(rng, m, lm.DNA))
            continue
        r = long_enough[int(rng.integers(0, len(long_enough)))]
        at = int(rng.integers(0, len(r) - m + 1))
        piece = bytearray(r[at:at + m])
        if i % 10 < 7:
            p = int(rng.integers(0, m))
            piece[p] = [c for c in lm.DNA if c != piece[p]][int(rng.integers(0, 3))]
        kmers.append(bytes(piece))
    (tmp_path / "kmers.txt").write_bytes(b"\n".join(kmers) + b"\n")
    return fa, kmers


def test_kmer_neighbours_example_compiles_and_fails_loudly_without_a_gpu(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    exe = _compile(tmp_path)  # against the two public headers, warnings as errors
    if _lib.lib().awfmGpuDeviceCount() > 0:
        return  # what it prints on a GPU is the next test's
    _inputs(tmp_path)
    out = subprocess.run([exe, "records.fa", "kmers.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "no CPU search path" in out.stderr and out.stdout == ""


@pytest.mark.gpu
def test_kmer_neighbours_example_prints_what_the_host_twin_finds(awfm, require_gpu, tmp_path):
    from avxwindowfmindex_amd import _lib
    fa, kmers = _inputs(tmp_path)
    out = subprocess.run([_compile(tmp_path), "records.fa", "kmers.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    chars, offsets = osc.pack(kmers)
    queries, edits, ranges, total, variants, occurrences = awfm.one_substitution_search_host(ix, chars, offsets)
    L = _lib.lib()
    want, illegal = [], 0
    for q, edit, (sp, ep) in zip(queries, edits, ranges):
        ok = C.c_int(0)
        rows = np.array([L.awFmFindDatabaseHitPositionSingle(ix.ptr, int(p), C.byref(ok)) for p in range(int(sp), int(ep) + 1)], np.uint64)
        seq, local, bad = awfm.local_positions_host(ix, rows)
        illegal += bad
        # (a nucleotide index: the letter index in the edit's low five bits is 0..3)
        name = b"=" if edit == osc.EDIT_NONE else b"%d%c" % (int(edit) >> 5, lm.DNA[int(edit) & 3])
        for s, p in zip(seq, local):
            where = b"*" if s == lp.ILLEGAL else ix.header(int(s))
            want.append(b"%d:%s:%s:%d" % (int(q), name, where, int(p)))
    assert len(want) > 400 and (edits != osc.EDIT_NONE).sum() > 300 and (variants == 0).any()
    assert out.stdout.split(b"\n")[:-1] == want
    assert f"kmers {len(kmers)} records {total} occurrences {len(want)} illegal {illegal}".encode() in out.stderr
    ix.dealloc()
