"""examples/read_pairs_estimated.c is a C program written against the two public headers only (include/AwFmIndex.h,
include/awfm_gpu.h): the loop of examples/read_pairs.c with no insert interval on the command line -- after the first slot scores
the histogram of template lengths over a wide range (awfmInsertHistogram), the interval from its quartiles (awfmInsertInterval),
and both pairings with it -> the estimate on stderr and one line `pair proper T MAPQ1 pos1 CIGAR1 MAPQ2 pos2 CIGAR2` per pair.  It
compiles with -Wall -Wextra -Werror, runs the host twins and, where there is a GPU, the device calls as well (and then refuses to
print when the two differ); its lines and its estimate must be what the Python API gives on the same files: the loop of
tests/insert_size_common.py EstimatingHostSide, which tests/test_insert_size.py holds to the planted pairs."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import insert_size_common as ic  # noqa: E402
import pair_mates_common as pm  # noqa: E402
import read_candidates_common as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(tmp_path):
    exe = str(tmp_path / "read_pairs_estimated")
    lib_dir = os.path.join(ROOT, "avxwindowfmindex_amd")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "examples", "read_pairs_estimated.c"),
                           "-I" + os.path.join(ROOT, "include"), "-L" + lib_dir, "-lawfmindex_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def test_read_pairs_estimated_example_prints_what_the_python_api_finds(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    e = pm.EndToEnd(awfm, tmp_path)
    try:
        reads = [bytes(e.sequenced[int(a):int(b)]) for a, b in zip(e.offsets[:-1], e.offsets[1:])]
        (tmp_path / "pairs.txt").write_bytes(b"".join(r + b"\n" for r in reads))
        E, I = pm.E2E, ic.E2E_INSERT
        assert I["min_score"] == E["min_score"]  # (the program has one minScore)
        args = [I["low_template"], I["high_template"], I["fallback_min"], I["fallback_max"], rc.E2E_STEP, rc.E2E_MIN_LENGTH, rc.E2E_CAP, rc.E2E_MAX_HITS,
                E["band"], E["min_votes"], E["lookback"], E["gap_penalty"], 8, 15, E["max_ops"], *E["scoring"], E["min_score"], E["unpaired_penalty"],
                E["window_pad"], E["mapq_cap"], I["min_quality"], I["spread"], I["min_samples"]]
        out = subprocess.run([_compile(tmp_path), "strands.fa", "pairs.txt"] + [str(v) for v in args], cwd=tmp_path, capture_output=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        side = ic.EstimatingHostSide(awfm, e)
        first, second, aligned = e.loop(side)
        ic.check_end_to_end(e, side.estimate, second, aligned)
        t = side.estimate
        estimate = (f"insert estimate: valid {t['valid']} interval {t['minInsert']} {t['maxInsert']} quartiles {t['quartiles'][0]} {t['quartiles'][1]} "
                    f"{t['quartiles'][2]} mean {t['mean']} samples {t['numSamples']} outside {t['numOutside']}\n")
        assert estimate.encode() in out.stderr, out.stderr
        assert "valid 1 interval 384 416 quartiles 400 400 400 mean 400" in estimate  # the planted library

        def mate(r):
            if not 0 < int(aligned["scores"][r]) < pm.TOO_LONG:
                return b"\t0\t*\t*"
            k = int(aligned["numOps"][r])
            script = awfm.cigar_of(aligned["ops"][r][:k]).encode() if 0 < k <= E["max_ops"] else b"*"
            sequence = int(e.final_slots["sequences"][r, int(second["pairSlots"][r])])
            return b"\t%d\t%s:%d\t%s" % (int(second["mappingQualities"][r]), e.ix.header(sequence), int(aligned["textBegins"][r]), script)

        want = [b"%d\t%d\t%d" % (p, int(second["properPairs"][p]), int(second["templateLengths"][p])) + mate(2 * p) + mate(2 * p + 1)
                for p in range(E["pairs"])]
        for p, (s, at, mate_at, kind) in enumerate(e.plan):  # what the lines of the planted pairs say
            fields = want[p].split(b"\t")
            assert fields[4] == b"%s:%d" % (e.ix.header(s), at) and fields[5] == b"100=", want[p]
            assert fields[1:3] == ([b"0", b"0"] if kind == "far" else [b"1", b"400"]) and fields[7] == b"%s:%d" % (e.ix.header(s), mate_at), want[p]
        assert out.stdout.split(b"\n")[:-1] == want
        side_name = "device" if _lib.lib().awfmGpuDeviceCount() > 0 else "host"
        assert f"proper {second['numProper']} rescue windows left {second['numWindows']}".encode() in out.stderr, out.stderr
        assert f"on the {side_name}".encode() in out.stderr, out.stderr
    finally:
        e.close()
