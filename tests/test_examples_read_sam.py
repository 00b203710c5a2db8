"""examples/read_sam.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
read_clipped.c's pipeline, then awfmAlignmentStrings / awfmGpuAlignmentStrings on the alignment's arrays as they are -> one
SAM-shaped line per read, `read FLAG header POS 255 CIGAR * 0 0 read * NM:i: AS:i: MD:Z:`.  It runs the host twins and, where there
is a GPU, the device calls as well (and then refuses to print when the two differ, strings included); its lines must be what the
Python API gives on the same FASTA file and reads: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates,
awfmReadChains, awfmVerifyChains, awfmAlignChainsAffine and alignment_strings_host with the classic CIGAR."""
import os
import re
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
    exe = str(tmp_path / "read_sam")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_sam.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_sam_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    lengths = lp.record_lengths(43, count=60, longest=900)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records, count=24)
    record, at = next(p for p in planted if p is not None)[:2]
    reads.append(records[record][at:at + 50] + records[record][at + 53:at + 110])  # three text characters deleted: one run of D
    reads.append(b"acg")  # shorter than a step: a read without seeds
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
    strings = awfm.alignment_strings_host(case.sequences, verified["bestSlots"], aligned["textBegins"], aligned["numOps"], aligned["ops"], text.tobytes(),
                                          ends, classic=True)
    cigars = awfm.strings_of(strings["cigarOffsets"], strings["cigarChars"])
    mds = awfm.strings_of(strings["mdOffsets"], strings["mdChars"])
    want, num_aligned = [], 0
    for r, read in enumerate(reads):
        score = int(aligned["scores"][r])
        if score == 0 or score >= af.TOO_LONG:
            want.append(b"%d\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*" % (r, read))
            assert cigars[r] == mds[r] == b""
            continue
        k = int(aligned["numOps"][r])
        assert (cigars[r] != b"") == (mds[r] != b"") == (0 < k <= MAX_OPS)
        line = b"%d\t0\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tAS:i:%d" % (
            r, ix.header(int(case.sequences[r, int(verified["bestSlots"][r])])), int(aligned["textBegins"][r]) + 1, cigars[r] or b"*", read,
            int(aligned["editDistances"][r]), score)
        want.append(line + (b"\tMD:Z:" + mds[r] if mds[r] else b""))
        if k <= MAX_OPS:  # the classic CIGAR is the script with '=' and X merged
            merged = re.sub(r"(\d+)[=X]((\d+)[=X])*", lambda m: str(sum(int(v) for v in re.findall(r"\d+", m.group(0)))) + "M", awfm.cigar_of(aligned["ops"][r][:k]))
            assert cigars[r] == merged.encode() and re.fullmatch(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", mds[r])
        num_aligned += 1
    assert num_aligned >= sum(p is not None for p in planted) + 1 and want[-2].split(b"\t")[1:3] == [b"4", b"*"]  # one is unaligned
    assert 0 < aligned["numTruncated"] == strings["numSkipped"] < num_aligned  # both kinds of line: strings, and * for a row that did not hold its script
    assert want[-1].split(b"\t")[3:6] == [b"%d" % (at + 5 + 1), b"255", b"5S95M7S"] and want[-1].endswith(b"\tNM:i:0\tAS:i:%d\tMD:Z:95" % (95 * SCORING[0]))  # one clips
    scripts = [awfm.cigar_of(aligned["ops"][r][:int(aligned["numOps"][r])]) for r in range(len(reads)) if 0 < int(aligned["numOps"][r]) <= MAX_OPS]
    assert any("X" in s for s in scripts) and any("D" in s for s in scripts)  # one line has an X, one a D
    assert any(re.search(rb"MD:Z:[0-9]+[A-Z][0-9]", line) for line in want) and any(re.search(rb"MD:Z:[0-9A-Z]*\^[A-Z]+[0-9]", line) for line in want)
    assert out.stdout.split(b"\n")[:-1] == want
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert (f"reads {len(reads)} windows {inst.num_seeds} aligned {num_aligned} unaligned {aligned['numUnaligned']} "
            f"truncated {aligned['numTruncated']} skipped {strings['numSkipped']} overflow 0 on the {side}").encode() in out.stderr
    ix.dealloc()
