"""examples/read_unclipped.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_sam.c's pipeline with awfmScoreChainsEndBonus / awfmGpuScoreChainsEndBonus for the best slot and the mapping quality and
awfmAlignChainsEndBonus / awfmGpuAlignChainsEndBonus for the script, run under B = 0 and under B = 5 -> awfmAlignmentStrings /
awfmGpuAlignmentStrings -> two SAM-shaped lines per read.  It runs the host twins and, where there is a GPU, the device calls as
well (and then refuses to print when the two differ, strings included); its lines must be what the Python API gives on the same
FASTA file and reads: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates, awfmReadChains, the two end-bonus
twins and alignment_strings_host.  Reads with a substitution two characters from an end are clipped in the first line and whole
in the second."""
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
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY, MAX_OPS, SCORING, BONUS = 2, 2, 4, 32, 2, 9, (1, 4, 6, 1), 5
OTHER = {ord("a"): b"c", ord("c"): b"g", ord("g"): b"t", ord("t"): b"a"}


def compile_example(tmp_path):
    exe = str(tmp_path / "read_unclipped")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_unclipped.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def make_inputs(tmp_path):
    """records.fa and reads.txt in tmp_path -> (records, reads, the number of the first read made by hand)"""
    lengths = lp.record_lengths(43, count=60, longest=900)
    records = lp.write_fasta(str(tmp_path / "records.fa"), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records, count=24)
    record, at = next(p for p in planted if p is not None)[:2]
    exact = records[record][at:at + 100]
    by_hand = len(reads)
    reads.append(exact[:97] + OTHER[exact[97]] + exact[98:])  # a substitution two characters from the end: 2 + B > 4 keeps it
    reads.append(exact[:2] + OTHER[exact[2]] + exact[3:])  # and from the start
    reads.append(exact[:95] + OTHER[exact[95]] + exact[96:])  # four characters from the end: 4 + 0 = 4 is a tie, clipped without the bonus
    reads.append(b"nnnnn" + exact[5:] + b"nnnnnnn")  # five and seven characters that match nothing: clipped under either
    reads.append(b"acg")  # shorter than a step: a read without seeds
    (tmp_path / "reads.txt").write_bytes(b"\n".join(reads) + b"\n")
    return records, reads, by_hand


def run_example(tmp_path):
    if not (tmp_path / "reads.txt").exists():
        make_inputs(tmp_path)
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY),
            str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in SCORING] + [str(BONUS)]
    return subprocess.run([compile_example(tmp_path), "records.fa", "reads.txt"] + args, cwd=tmp_path, capture_output=True, timeout=300)


def expected_lines(awfm, tmp_path):
    """the lines by the Python API's host calls -> (lines, per bonus the alignment call's outputs, reads, the first read made by hand)"""
    records, reads, by_hand = make_inputs(tmp_path)
    ix = awfm.create_index_from_fasta(str(tmp_path / "records.fa"), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "check.awfmi"))
    inst = rc.host_pipeline(awfm, ix, reads)
    case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=MIN_VOTES)
    got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=BAND, lookback=LOOKBACK, gap_penalty=GAP_PENALTY)
    text, ends = vc.text_of(records)
    slots = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
    offsets = np.concatenate(([0], np.cumsum([len(r) for r in reads])))
    chars = b"".join(reads)
    matrix = awfm.matrix_scoring_uniform(awfm.AwFmAlphabetDna, SCORING)
    per_bonus = []
    for bonus in (0, BONUS):
        scored = awfm.score_chains_end_bonus_host(chars, offsets, slots, text.tobytes(), matrix, bonus, ends, band_pad=vc.E2E_W, max_drift=vc.E2E_X,
                                                  min_score=1, mapq_cap=60)
        aligned = awfm.align_chains_end_bonus_host(chars, offsets, slots, scored["bestSlots"], text.tobytes(), matrix, bonus, ends, band_pad=vc.E2E_W,
                                                   max_drift=vc.E2E_X, max_ops=MAX_OPS)
        strings = awfm.alignment_strings_host(case.sequences, scored["bestSlots"], aligned["textBegins"], aligned["numOps"], aligned["ops"],
                                              text.tobytes(), ends)
        cigars, mds = awfm.strings_of(strings["cigarOffsets"], strings["cigarChars"]), awfm.strings_of(strings["mdOffsets"], strings["mdChars"])
        lines = []
        for r, read in enumerate(reads):
            score = int(aligned["scores"][r])
            if score == 0 or score >= af.TOO_LONG:
                lines.append(b"%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*\teb:i:%d" % (r, read, bonus))
                continue
            assert score == int(scored["bestScores"][r])  # the alignment of the best slot has the best slot's score
            line = b"%d\t0\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tAS:i:%d" % (
                r, ix.header(int(case.sequences[r, int(scored["bestSlots"][r])])), int(aligned["textBegins"][r]) + 1, int(scored["mappingQualities"][r]),
                cigars[r] or b"*", read, int(aligned["editDistances"][r]), score)
            lines.append(line + (b"\tMD:Z:" + mds[r] if mds[r] else b"") + b"\teb:i:%d" % bonus)
        per_bonus.append((lines, aligned))
    ix.dealloc()
    want = [line for pair in zip(per_bonus[0][0], per_bonus[1][0]) for line in pair]
    return want, [aligned for _, aligned in per_bonus], reads, by_hand


def test_read_unclipped_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    want, (plain, bonus), reads, h = expected_lines(awfm, tmp_path)
    out = run_example(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split(b"\n")[:-1] == want

    def fields(r, k):
        return want[2 * r + k].split(b"\t")

    # two characters from the end: 97=3S and score 97 without the bonus; whole, one X, 97 + 5 - 4 + 2 + 5 with it
    assert fields(h, 0)[5] == b"97=3S" and fields(h, 0)[11:13] == [b"NM:i:0", b"AS:i:97"] and fields(h, 0)[-1] == b"eb:i:0"
    assert fields(h, 1)[5] == b"97=1X2=" and fields(h, 1)[11:13] == [b"NM:i:1", b"AS:i:105"] and fields(h, 1)[-1] == b"eb:i:5"
    assert fields(h, 1)[13].startswith(b"MD:Z:97") and fields(h, 1)[13].endswith(b"2")
    assert fields(h + 1, 0)[5] == b"3S97=" and fields(h + 1, 1)[5] == b"2=1X97=" and int(fields(h + 1, 1)[3]) == int(fields(h + 1, 0)[3]) - 3
    # four characters from the end: the tie goes to the clip without the bonus
    assert fields(h + 2, 0)[5] == b"95=5S" and fields(h + 2, 1)[5] == b"95=1X4="
    # letters that match nothing stay clipped; the read's middle reaches no end and earns nothing
    assert fields(h + 3, 0)[5] == fields(h + 3, 1)[5] == b"5S95=7S" and fields(h + 3, 0)[12] == fields(h + 3, 1)[12] == b"AS:i:95"
    assert fields(h + 4, 0)[1] == fields(h + 4, 1)[1] == b"4"
    gained = [r for r in range(len(reads)) if 0 < plain["scores"][r] < af.TOO_LONG and bonus["editDistances"][r] > plain["editDistances"][r]]
    assert set(range(h, h + 3)) <= set(gained)
    edits = sum(int(bonus["editDistances"][r]) - int(plain["editDistances"][r]) for r in gained)
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert f"with bonus {BONUS}: {len(gained)} reads gained {edits} edits; on the {side}".encode() in out.stderr, out.stderr
