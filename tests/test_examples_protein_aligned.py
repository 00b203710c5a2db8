"""examples/protein_aligned.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h):
an amino FASTA file, peptide queries and a substitution matrix file -> seeds, candidates and chains as in examples/read_sam.c ->
awfmScoreChainsMatrix / awfmGpuScoreChainsMatrix for the best slot and the mapping quality -> awfmAlignChainsMatrix /
awfmGpuAlignChainsMatrix -> awfmAlignmentStrings / awfmGpuAlignmentStrings -> one line per query.  It is fed the hand-written
matrix, FASTA file and peptides of tests/golden/ (this repository's own data, no published matrix).  It runs the host twins and,
where there is a GPU, the device calls as well (and then refuses to print when the two differ); its lines must be what the
Python API gives on the same files: the host's pipeline (tests/read_candidates_common.py), awfmReadCandidates, awfmReadChains,
awfmMatrixScoringFromText, the two matrix twins and awfmAlignmentStrings."""
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import matrix_scores_common as mx  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402
import verify_chains_common as vc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY, MAX_OPS, GAPS = 2, 2, 4, 32, 1, 16, (11, 1)


def compile_example(tmp_path):
    exe = str(tmp_path / "protein_aligned")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "protein_aligned.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd", "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def run_example(tmp_path):
    args = [str(rc.E2E_STEP), str(rc.E2E_MIN_LENGTH), str(rc.E2E_CAP), str(rc.E2E_MAX_HITS), str(BAND), str(MIN_VOTES), str(LOOKBACK), str(GAP_PENALTY),
            str(vc.E2E_W), str(vc.E2E_X), str(MAX_OPS)] + [str(v) for v in GAPS]
    files = [os.path.join(GOLDEN, name) for name in ("proteins.fa", "peptides.txt", "protein_matrix.txt")]
    return subprocess.run([compile_example(tmp_path)] + files + args, cwd=tmp_path, capture_output=True, timeout=300)


def expected_lines(awfm, tmp_path):
    """the lines by the Python API's host calls, and the number of aligned queries"""
    records, name = [], None
    for line in open(os.path.join(GOLDEN, "proteins.fa"), "rb").read().split(b"\n"):
        if line.startswith(b">"):
            records.append(b"")
        elif line:
            records[-1] += line
    queries = [q for q in open(os.path.join(GOLDEN, "peptides.txt"), "rb").read().split(b"\n") if q]
    matrix = awfm.matrix_scoring_from_text(open(os.path.join(GOLDEN, "protein_matrix.txt"), "rb").read(), awfm.AwFmAlphabetAmino, *GAPS)
    ix = awfm.create_index_from_fasta(os.path.join(GOLDEN, "proteins.fa"), awfm.AwFmAlphabetAmino, 8, 3, file_src=str(tmp_path / "check.awfmi"))
    inst = rc.host_pipeline(awfm, ix, queries)
    case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=MIN_VOTES)
    got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=BAND, lookback=LOOKBACK, gap_penalty=GAP_PENALTY)
    text, ends = vc.text_of(records)
    slots = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
    offsets = np.concatenate(([0], np.cumsum([len(q) for q in queries])))
    chars = b"".join(queries)
    scored = awfm.score_chains_matrix_host(chars, offsets, slots, text.tobytes(), matrix, ends, awfm.AwFmAlphabetAmino, band_pad=vc.E2E_W,
                                           max_drift=vc.E2E_X, min_score=1, mapq_cap=60)
    aligned = awfm.align_chains_matrix_host(chars, offsets, slots, scored["bestSlots"], text.tobytes(), matrix, ends, awfm.AwFmAlphabetAmino,
                                            band_pad=vc.E2E_W, max_drift=vc.E2E_X, max_ops=MAX_OPS)
    strings = awfm.alignment_strings_host(case.sequences, scored["bestSlots"], aligned["textBegins"], aligned["numOps"], aligned["ops"], text.tobytes(),
                                          ends, awfm.AwFmAlphabetAmino)
    cigars, mds = awfm.strings_of(strings["cigarOffsets"], strings["cigarChars"]), awfm.strings_of(strings["mdOffsets"], strings["mdChars"])
    want, num_aligned = [], 0
    for r in range(len(queries)):
        score = int(aligned["scores"][r])
        if score == 0 or score >= af.TOO_LONG:
            want.append(b"%d\t*\t0\t0\t0\t*\t0\t*" % r)
            continue
        assert score == int(scored["bestScores"][r])  # the alignment of the best slot has the best slot's score
        want.append(b"%d\t%s\t%d\t%d\t%d\t%s\t%d\t%s" % (r, ix.header(int(case.sequences[r, int(scored["bestSlots"][r])])), int(aligned["textBegins"][r]) + 1, score,
                                                       int(scored["mappingQualities"][r]), cigars[r] or b"*", int(aligned["editDistances"][r]), mds[r] or b"*"))
        num_aligned += 1
    # the scripts re-scored from the text with the parsed matrix give the scores: X columns that score among them
    values = mx.Matrix(awfm.matrix_values(matrix), *GAPS)
    check = mx.Case(chars, offsets, slots, scored["bestSlots"], text.tobytes(), ends, af.AMINO)
    assert mx.assert_scripts_replay(check, aligned, vc.E2E_W, vc.E2E_X, values, MAX_OPS) == num_aligned
    ix.dealloc()
    return want, num_aligned, len(queries), inst.num_seeds, aligned


def test_protein_aligned_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    out = run_example(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    want, num_aligned, num_queries, num_seeds, aligned = expected_lines(awfm, tmp_path)
    assert out.stdout.split(b"\n")[:-1] == want
    assert num_aligned == 6 and want[-1].endswith(b"\t*\t0\t0\t0\t*\t0\t*") and want[-2].endswith(b"\t*\t0\t0\t0\t*\t0\t*")
    assert want[3].split(b"\t")[1] == b"repeat region" and want[3].split(b"\t")[5].startswith(b"5S9=1X") and want[3].split(b"\t")[5].endswith(b"4S")
    assert any(b"D" in line.split(b"\t")[5] for line in want[:6]) and any(b"I" in line.split(b"\t")[5] for line in want[:6])
    side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
    assert (f"queries {num_queries} windows {num_seeds} aligned {num_aligned} unaligned {aligned['numUnaligned']} "
            f"truncated {aligned['numTruncated']}").encode() in out.stderr and f"on the {side}".encode() in out.stderr
    bad = tmp_path / "bad_matrix.txt"
    bad.write_text("A R\nA 1 2\n")
    files = [os.path.join(GOLDEN, "proteins.fa"), os.path.join(GOLDEN, "peptides.txt"), str(bad)]
    refused = subprocess.run([str(tmp_path / "protein_aligned")] + files, cwd=tmp_path, capture_output=True, timeout=60)
    assert refused.returncode == 2 and b"is no amino substitution matrix: -9" in refused.stderr
