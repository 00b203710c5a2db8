"""examples/read_pairs.c is a C program written against the two public headers only (include/AwFmIndex.h, include/awfm_gpu.h): the
reads of a pairs file, mate 2 as sequenced, onto one strand (awfmReverseComplementReads), the path of read_mapped.c to chains
with three slots in a table of stride four, slot scores, pairing (awfmPairMates), window scores on the windows the pairing names,
slot scores and pairing again, affine alignment with pairSlots -> one line `pair proper T MAPQ1 pos1 CIGAR1 MAPQ2 pos2 CIGAR2` per
pair.  It runs the host twins and, where there is a GPU, the device calls as well (and then refuses to print when the two
differ); its lines must be what the Python API gives on the same files: the loop of tests/pair_mates_common.py EndToEnd through
the host twins, which tests/test_pair_mates.py holds to the planted pairs."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_mates_common as pm  # noqa: E402
import read_candidates_common as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "read_pairs")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_pairs.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_pairs_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    e = pm.EndToEnd(awfm, tmp_path)
    try:
        reads = [bytes(e.sequenced[int(a):int(b)]) for a, b in zip(e.offsets[:-1], e.offsets[1:])]
        (tmp_path / "pairs.txt").write_bytes(b"".join(r + b"\n" for r in reads))
        E = pm.E2E
        args = [E["min_insert"], E["max_insert"], rc.E2E_STEP, rc.E2E_MIN_LENGTH, rc.E2E_CAP, rc.E2E_MAX_HITS, E["band"], E["min_votes"], E["lookback"],
                E["gap_penalty"], 8, 15, E["max_ops"], *E["scoring"], E["min_score"], E["unpaired_penalty"], E["window_pad"], E["mapq_cap"]]
        out = subprocess.run([_compile(tmp_path), "strands.fa", "pairs.txt"] + [str(v) for v in args], cwd=tmp_path, capture_output=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        first, second, aligned = e.loop(pm.HostSide(awfm, e))
        e.check(first, second, aligned)
        placed = awfm.score_windows_affine(e.chars, e.offsets, first["windowSequences"], first["windowBegins"], first["windowEnds"], e.text, e.ends,
                                           scoring=E["scoring"], min_score=E["min_score"], outputs=["numFound"], threads=16)

        def mate(r):
            if not 0 < int(aligned["scores"][r]) < pm.TOO_LONG:
                return b"\t0\t*\t*"
            k = int(aligned["numOps"][r])
            script = awfm.cigar_of(aligned["ops"][r][:k]).encode() if 0 < k <= E["max_ops"] else b"*"
            sequence = int(e.final_slots["sequences"][r, int(second["pairSlots"][r])])
            return b"\t%d\t%s:%d\t%s" % (int(second["mappingQualities"][r]), e.ix.header(sequence), int(aligned["textBegins"][r]), script)

        want = [b"%d\t%d\t%d" % (p, int(second["properPairs"][p]), int(second["templateLengths"][p])) + mate(2 * p) + mate(2 * p + 1)
                for p in range(E["pairs"])]
        # what the lines of the planted pairs say: a plain pair is two exact reads 400 apart, a rescued mate carries its nine substitutions
        for p, (s, at, mate_at, kind) in enumerate(e.plan):
            fields = want[p].split(b"\t")
            assert fields[4] == b"%s:%d" % (e.ix.header(s), at) and fields[5] == b"100=", want[p]
            if kind == "plain":
                assert fields[1:4] == [b"1", b"400", b"60"] and fields[6:] == [b"60", b"%s:%d" % (e.ix.header(s), mate_at), b"100="], want[p]
            elif kind == "rescued":
                assert fields[1:3] == [b"1", b"400"] and fields[7] == b"%s:%d" % (e.ix.header(s), mate_at), want[p]
                assert fields[8] == b"5=1X10=1X10=1X10=1X10=1X10=1X10=1X10=1X10=1X6=", want[p]
            else:
                assert fields[1:3] == [b"0", b"0"] and fields[7] == b"%s:%d" % (e.ix.header(s), mate_at), want[p]
        assert out.stdout.split(b"\n")[:-1] == want
        side = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
        summary = (f"pairs {E['pairs']} windows {2 * E['pairs'] * (E['length'] // rc.E2E_STEP)} proper {second['numProper']} rescue windows left "
                   f"{second['numWindows']} found in windows {placed['numFound']} aligned {2 * E['pairs']} on the {side}")
        assert summary.encode() in out.stderr, out.stderr
    finally:
        e.close()
