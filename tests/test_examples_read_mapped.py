"""examples/read_mapped.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_clipped.c's path with awfmScoreChainsAffine / awfmGpuScoreChainsAffine between chains and affine alignment, whose bestSlots
the alignment takes as they are -> one line `read:header:textBegin:MAPQ:score:secondScore:CIGAR` per read.  It runs the host twins
and, where there is a GPU, the device calls as well (and then refuses to print when the two differ); its lines must be what the
Python API gives on the same FASTA file: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates,
awfmReadChains, awfmScoreChainsAffine and awfmAlignChainsAffine, printed with cigar_of."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY, MAX_OPS, SCORING, MIN_SCORE, CAP = 2, 2, 4, 32, 2, 9, (2, 4, 4, 2), 40, 60


def _compile(tmp_path):
    exe = str(tmp_path / "read_mapped")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_mapped.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_mapped_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    lengths = lp.record_lengths(43, count=60, longest=900)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records, count=24)
    record, at = next(p for p in planted if p is not None)[:2]
    # the record of the first planted read once more at the file's end: that read and its neighbours map twice, at mapq 0
    with open(fa, "ab") as f:
        f.write(b">copy\n" + records[record] + b"\n")
    records = records + [records[record]]
    reads.append(b"acg")  # shorter than a step: a read without seeds
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY),
            str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in SCORING] + [str(MIN_SCORE), str(CAP)]
    out = subprocess.run([_compile(tmp_path), "records.fa", "reads.txt"] + args, cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    inst = rc.host_pipeline(awfm, ix, reads)
    case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=MIN_VOTES)
    got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=BAND, lookback=LOOKBACK, gap_penalty=GAP_PENALTY)
    text, ends = vc.text_of(records)
    slots = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads])))
    scored = awfm.score_chains_affine_host(b"".join(reads), offsets, slots, text.tobytes(), ends, band_pad=vc.E2E_W, max_drift=vc.E2E_X, scoring=SCORING,
                                           min_score=MIN_SCORE, mapq_cap=CAP)
    aligned = awfm.align_chains_affine_host(b"".join(reads), offsets, slots, scored["bestSlots"], text.tobytes(), ends, band_pad=vc.E2E_W,
                                            max_drift=vc.E2E_X, scoring=SCORING, max_ops=MAX_OPS)
    want, num_aligned, qualities = [], 0, []
    for r in range(len(reads)):
        best = int(scored["bestSlots"][r])
        if best == sc.NO_SLOT:
            want.append(b"%d:*:0:0:0:0:*" % r)
            continue
        assert int(aligned["scores"][r]) == int(scored["bestScores"][r])
        k = int(aligned["numOps"][r])
        script = awfm.cigar_of(aligned["ops"][r][:k]) if 0 < k <= MAX_OPS else "*"
        want.append(b"%d:%s:%d:%d:%d:%d:%s" % (r, ix.header(int(case.sequences[r, best])), int(aligned["textBegins"][r]), int(scored["mappingQualities"][r]),
                                               int(scored["bestScores"][r]), int(scored["secondScores"][r]), script.encode()))
        qualities.append(int(scored["mappingQualities"][r]))
        num_aligned += 1
    assert num_aligned >= sum(p is not None for p in planted) and want[-1] == b"%d:*:0:0:0:0:*" % (len(reads) - 1)
    assert 0 in qualities and CAP in qualities  # reads of the record that stands in the file twice, and reads with one locus
    assert 0 < aligned["numTruncated"] < num_aligned  # both kinds of line: a script, and * for a row that did not hold it
    assert out.stdout.split(b"\n")[:-1] == want
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert (f"reads {len(reads)} windows {inst.num_seeds} mapped {scored['numMapped']} aligned {num_aligned} "
            f"truncated {aligned['numTruncated']} on the {side}").encode() in out.stderr
    ix.dealloc()
