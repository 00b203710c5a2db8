"""examples/read_verified.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_verified.c plus awfmGpuIndexSetText and awfmGpuVerifyChains, fed with the arrays of the candidate and the chain call as they
are -> `read:header:begin:end:score:distance` per read with a verified chain.  Without a GPU it must fail loudly; on the GPU its
lines must be what the host gives: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates, awfmReadChains and
awfmVerifyChains."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 2, 2, 4, 32, 2


def _compile(tmp_path):
    exe = str(tmp_path / "read_verified")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_verified.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _inputs(tmp_path):
    lengths = lp.record_lengths(43, count=200, longest=1500)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records)
    reads.append(b"acg")  # shorter than a step: a read without seeds
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    return fa, reads, planted, records


def test_read_verified_example_compiles_and_fails_loudly_without_a_gpu(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    exe = _compile(tmp_path)  # against the two public headers, warnings as errors
    if _lib.lib().awfmGpuDeviceCount() > 0:
        return  # what it prints on a GPU is the next test's
    _inputs(tmp_path)
    out = subprocess.run([exe, "records.fa", "reads.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert out.returncode == 3 and "no CPU search path" in out.stderr and out.stdout == ""


@pytest.mark.gpu
def test_read_verified_example_prints_what_the_host_twin_finds(awfm, require_gpu, tmp_path):
    fa, reads, planted, records = _inputs(tmp_path)
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY), str(vc.E2E_W), str(vc.E2E_X)]
    out = subprocess.run([_compile(tmp_path), "records.fa", "reads.txt"] + args, cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    inst = rc.host_pipeline(awfm, ix, reads)
    case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=MIN_VOTES)
    got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=BAND, lookback=LOOKBACK, gap_penalty=GAP_PENALTY)
    text, ends = vc.text_of(records)
    slots = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads])))
    verified = vc.Case(b"".join(reads), offsets, slots, text.tobytes(), ends).host(awfm, vc.E2E_W, vc.E2E_X)
    want = []
    for r in range(len(reads)):
        j = int(verified["bestSlots"][r])
        if j == vc.NO_SLOT:
            continue
        begin = int(got["chainReadBegins"][r, j]) + int(got["chainBeginDiagonals"][r, j])
        end = int(got["chainReadEnds"][r, j]) + int(got["chainEndDiagonals"][r, j])
        want.append(b"%d:%s:%d:%d:%d:%d" % (r, ix.header(int(case.sequences[r, j])), begin, end, int(got["chainScores"][r, j]),
                                            int(verified["editDistances"][r, j])))
    assert len(want) >= sum(p is not None for p in planted)
    assert out.stdout.split(b"\n")[:-1] == want
    assert (f"reads {len(reads)} windows {inst.num_seeds} occurrences {inst.num_hits} verified {len(want)} overflowed 0 unverified 0".encode()
            in out.stderr)
    ix.dealloc()
