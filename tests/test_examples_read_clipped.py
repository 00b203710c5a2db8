"""examples/read_clipped.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_aligned.c with awfmAlignChainsAffine / awfmGpuAlignChainsAffine in place of the unit-cost stage, fed with verification's
bestSlots as they are -> one line `read <tab> header <tab> pos <tab> score <tab> CIGAR <tab> NM` per read.  It runs the host twins
and, where there is a GPU, the device calls as well (and then refuses to print when the two differ); its lines must be what the
Python API gives on the same FASTA file: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates,
awfmReadChains, awfmVerifyChains and awfmAlignChainsAffine, printed with cigar_of."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY, MAX_OPS, SCORING = 2, 2, 4, 32, 2, 9, (2, 4, 4, 2)


def _compile(tmp_path):
    exe = str(tmp_path / "read_clipped")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_clipped.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_clipped_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    lengths = lp.record_lengths(43, count=60, longest=900)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records, count=24)
    reads.append(b"acg")  # shorter than a step: a read without seeds
    record, at = next(p for p in planted if p is not None)[:2]
    reads.append(b"nnnnn" + records[record][at + 5:at + 100] + b"nnnnnnn")  # clipped at both ends
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY),
            str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in SCORING]
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
    aligned = awfm.align_chains_affine_host(b"".join(reads), offsets, slots, verified["bestSlots"], text.tobytes(), ends, band_pad=vc.E2E_W,
                                            max_drift=vc.E2E_X, scoring=SCORING, max_ops=MAX_OPS)
    want, num_aligned = [], 0
    for r in range(len(reads)):
        score = int(aligned["scores"][r])
        if score == 0 or score >= af.TOO_LONG:
            want.append(b"%d\t*\t0\t0\t*\t0" % r)
            continue
        k = int(aligned["numOps"][r])
        script = awfm.cigar_of(aligned["ops"][r][:k]) if 0 < k <= MAX_OPS else "*"
        want.append(b"%d\t%s\t%d\t%d\t%s\t%d" % (r, ix.header(int(case.sequences[r, int(verified["bestSlots"][r])])), int(aligned["textBegins"][r]), score,
                                                 script.encode(), int(aligned["editDistances"][r])))
        num_aligned += 1
    assert num_aligned >= sum(p is not None for p in planted) + 1 and want[-2].endswith(b"\t*\t0\t0\t*\t0")
    assert 0 < aligned["numTruncated"] < num_aligned  # both kinds of line: a script, and * for a row that did not hold it
    assert want[-1].split(b"\t")[2:] == [b"%d" % (at + 5), b"%d" % (95 * SCORING[0]), b"5S95=7S", b"0"], want[-1]
    assert out.stdout.split(b"\n")[:-1] == want
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert (f"reads {len(reads)} windows {inst.num_seeds} aligned {num_aligned} unaligned {aligned['numUnaligned']} "
            f"truncated {aligned['numTruncated']} on the {side}").encode() in out.stderr
    assert awfm.cigar_of([5 << 4 | 4, 3 << 4 | 7, 1 << 4 | 8, 2 << 4 | 1, 1 << 4 | 2]) == "5S3=1X2I1D"  # S is printed, the others as before
    ix.dealloc()
