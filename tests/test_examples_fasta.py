"""examples/kmer_locate_fasta.c is a C program written against the two public headers only (include/AwFmIndex.h,
include/awfm_gpu.h): FASTA -> index -> awfmGpuLocateHostLocal -> `kmer <tab> header:offset` per hit.  Without a GPU it must
fail loudly; on the GPU its lines must be what the host mapping (awfmGpuLocateHost + awfmLocalPositions + the headers) gives."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "kmer_locate_fasta")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "kmer_locate_fasta.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _inputs(tmp_path):
    lengths = lp.record_lengths(41, count=300, longest=900)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 12)
    rng = np.random.default_rng(4)
    long_enough = [r for r in records if len(r) >= 12]
    kmers = []
    for i in range(400):
        r = long_enough[int(rng.integers(0, len(long_enough)))]
        length = int(rng.integers(6, 13))
        at = int(rng.integers(0, len(r) - length + 1))
        kmers.append(r[at:at + length] if i % 4 else lp.DNA_LETTERS[rng.integers(0, 4, length)].tobytes())
    kmers.append(b"n")  # an ambiguity letter: it hits every record's terminator
    (tmp_path / "kmers.txt").write_bytes(b"\n".join(kmers) + b"\n")
    return fa, lengths, kmers


def test_fasta_example_fails_loudly_without_a_gpu(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    if _lib.lib().awfmGpuDeviceCount() > 0:
        pytest.skip("a GPU is present")
    _inputs(tmp_path)
    out = subprocess.run([_compile(tmp_path), "records.fa", "kmers.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "no CPU search path" in out.stderr and out.stdout == ""


@pytest.mark.gpu
def test_fasta_example_prints_the_host_mapping(awfm, require_gpu, tmp_path):
    fa, lengths, kmers = _inputs(tmp_path)
    out = subprocess.run([_compile(tmp_path), "records.fa", "kmers.txt"], cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    g = awfm.GpuIndex(ix)
    chars = np.frombuffer(b"".join(kmers), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in kmers])]).astype(np.uint64)
    _, hit_off, pos = g.locate_host(chars, offsets=offsets)
    seq, local, illegal = awfm.local_positions_host(ix, pos)
    want = []
    for i, kmer in enumerate(kmers):
        for h in range(int(hit_off[i]), int(hit_off[i + 1])):
            where = b"*" if seq[h] == lp.ILLEGAL else ix.header(int(seq[h]))
            want.append(kmer + b"\t" + where + b":" + str(int(local[h])).encode())
    assert illegal == len(lengths) and len(want) > 300  # `n` hits the terminators, all of them illegal positions
    assert out.stdout.split(b"\n")[:-1] == want
    assert f"hits {len(want)} illegal {illegal} records {len(lengths)}".encode() in out.stderr
    g.destroy()
    ix.dealloc()
