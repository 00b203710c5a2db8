"""examples/read_strands.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h): a FASTA
file indexed on ONE strand, FR pairs as sequenced from both strands, one batch of 2R rows (awfmReverseComplementReads, ALL, into the
second half), the path of read_mapped.c to chains with three slots in a table of stride four, slot scores, strand choice
(awfmChooseStrands), window scores on the windows it names, slot scores and strand choice again, orient (awfmOrientReads), affine
alignment with strandSlots, the classic strings and SAM records -> the header and one SAM line per read.  A few of its lines are
held to literals written out by hand -- a proper pair from the reverse strand with FLAG 83 / 163 and one from the forward
strand with 99 / 147, each with its POS, PNEXT and signed TLEN --, and all of them to what the Python API gives on the same files:
the loop of tests/strands_common.py EndToEnd through the host twins, which tests/test_strands.py holds to the planted pairs."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_candidates_common as rc  # noqa: E402
import strands_common as st  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "read_strands")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_strands.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def _arguments(E):
    return [E["min_insert"], E["max_insert"], rc.E2E_STEP, rc.E2E_MIN_LENGTH, rc.E2E_CAP, rc.E2E_MAX_HITS, E["band"], E["min_votes"], E["lookback"],
            E["gap_penalty"], 8, 15, E["max_ops"], *E["scoring"], E["min_score"], E["unpaired_penalty"], E["window_pad"], E["mapq_cap"]]


def test_read_strands_example_prints_what_the_python_api_finds(awfm, tmp_path):
    e = st.EndToEnd(awfm, tmp_path)
    try:
        reads = [bytes(e.sequenced[int(a):int(b)]) for a, b in zip(e.read_offsets[:-1], e.read_offsets[1:])]
        (tmp_path / "pairs.txt").write_bytes(b"".join(r + b"\n" for r in reads))
        out = subprocess.run([_compile(tmp_path), "one_strand.fa", "pairs.txt"] + [str(v) for v in _arguments(st.E2E)], cwd=tmp_path,
                             capture_output=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        e.qualities[:] = ord("I")  # the pairs file has no qualities: the program prints a constant one
        got = e.host_loop(awfm)
        e.check(got)
        assert out.stdout == awfm.sam_header(e.ix) + bytes(got["sam"]["lineChars"])
        kinds = [plan["kind"] for plan in e.plan]
        assert b"reads 192 on the reverse strand 96 proper pairs %d " % (len(kinds) - kinds.count("far")) in out.stderr, out.stderr
    finally:
        e.close()


def test_a_pair_from_each_strand_by_hand(awfm, tmp_path):
    """One record of 400 characters, written out here.  Pair 0 comes from the forward strand: mate 1 is the text at 0-based 20,
    mate 2 the reverse complement of the text at 240, 30 characters each, so the fragment is [20, 270): POS 21 and 241, TLEN
    +-250, FLAG 99 = 1 + 2 + 32 + 64 and 147 = 1 + 2 + 16 + 128.  Pair 1 comes from the reverse strand: mate 1 is the reverse
    complement of the text at 330, mate 2 the text at 100: POS 331 and 101, TLEN -+260, FLAG 83 = 1 + 2 + 16 + 64 and 163 = 1 + 2 +
    32 + 128; SEQ of a read on the reverse strand is the text's, not the read's as sequenced."""
    import numpy as np
    rng = np.random.default_rng(5)
    text = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, 400)].tobytes()
    (tmp_path / "one.fa").write_bytes(b">chrT hand made\n" + b"".join(text[j:j + 60] + b"\n" for j in range(0, 400, 60)))
    reads = [text[20:50], st.mirrored(text[240:270]), st.mirrored(text[330:360]), text[100:130]]
    (tmp_path / "pairs.txt").write_bytes(b"".join(r + b"\n" for r in reads))
    out = subprocess.run([_compile(tmp_path), "one.fa", "pairs.txt", "200", "300", "2", "12", "64", "16", "2", "2", "32", "1", "8", "15", "32", "1", "4",
                          "6", "1", "20", "17", "20", "60"], cwd=tmp_path, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split(b"\n")
    assert lines[0] == b"@HD\tVN:1.6\tSO:unknown" and lines[1] == b"@SQ\tSN:chrT\tLN:400" and lines[6] == b"" and len(lines) == 7
    quality = b"I" * 30
    tags = b"NM:i:0\tAS:i:30\tXS:i:0\tMD:Z:30"
    assert lines[2] == b"\t".join([b"0", b"99", b"chrT", b"21", b"60", b"30M", b"=", b"241", b"250", text[20:50], quality, tags])
    assert lines[3] == b"\t".join([b"0", b"147", b"chrT", b"241", b"60", b"30M", b"=", b"21", b"-250", text[240:270], quality, tags])
    assert lines[4] == b"\t".join([b"1", b"83", b"chrT", b"331", b"60", b"30M", b"=", b"101", b"-260", text[330:360], quality, tags])
    assert lines[5] == b"\t".join([b"1", b"163", b"chrT", b"101", b"60", b"30M", b"=", b"331", b"260", text[100:130], quality, tags])
