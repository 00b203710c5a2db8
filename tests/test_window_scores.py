"""awfmScoreWindowsAffine (include/awfm_gpu.h "window scores", csrc/awfm_window_affine.c), the host twin and checker of
awfmGpuScoreWindowsAffine: against the plain-Python restatement of tests/window_scores_common.py (the begin cell by the walk back,
which pins the twin's forward origins) on random batches in both alphabets under the five scorings, on the edge list with
hand-computed values, on the limits of width and length, on ties of the origin rule, through awfmAlignChainsAffine on the slots
it writes, and as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import window_scores_common as ws  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
PLANTED_SEED = 5


@pytest.mark.parametrize("alphabet", [ws.DNA, ws.AMINO], ids=["dna", "amino"])
@pytest.mark.parametrize("scoring", ws.SCORINGS, ids=[str(s) for s in ws.SCORINGS])
def test_random_batches_equal_the_python_restatement(awfm, alphabet, scoring):
    """reads planted with edits in windows that may cut them, some not looked at, malformed or clipped at a record's end"""
    case = ws.random_case(3 + alphabet, 80, alphabet)
    want = case.expected(scoring, min_score=5, stride=4, column=1, unscored_before=5, found_before=7)
    got = case.host(awfm, scoring, min_score=5, stride=4, column=1, unscored_before=5, found_before=7, fill=0x5A, threads=3)
    ws.assert_equal(got, want, what=str(scoring))
    kinds = set(int(v) for v in got["scores"] if v >= ws.TOO_LONG)
    assert {ws.NONE, ws.MALFORMED} <= kinds and (got["scores"] < ws.TOO_LONG).sum() > 40 and got["numFound"] > 7


def test_edge_list_by_hand_computed_values(awfm):
    b = ws.edge_builder()
    case = b.case()
    got = case.host(awfm, unscored_before=3, found_before=1)
    b.check(got)
    ws.assert_equal(got, case.expected(unscored_before=3, found_before=1))
    assert got["numUnscored"] == 3 + 2 and got["numFound"] == 1 + sum(1 for v in b.values if 0 < v[0] < ws.TOO_LONG)
    for skew in (1, 2, 3):  # the reads further into the buffer
        ws.assert_equal(b.case(skew).host(awfm, unscored_before=3, found_before=1), got, what=f"skew {skew}")
    # the slot of a found read, and the unused slot of the others
    r = b.names.index("clips at both ends of the read")
    assert [int(got[f][r, 0]) for f in vc.SLOT_FIELDS] == [4, 1, 2, 14, 2, 2]
    for r, value in enumerate(b.values):
        if not 0 < value[0] < ws.TOO_LONG:
            assert [int(got[f][r, 0]) for f in vc.SLOT_FIELDS] == [ws.UNUSED, 0, 0, 0, 0, 0], b.names[r]


def test_a_read_not_looked_at_keeps_its_slot_and_every_stride_and_column(awfm):
    b = ws.edge_builder()
    case = b.case()
    skipped = [r for r in range(case.num_reads) if case.sequences[r] == ws.UNUSED]
    assert skipped and 0 < skipped[0] < case.num_reads - 1  # between two that are looked at
    for stride in (1, 4, 16):
        for column in range(stride):
            slots = {name: np.full((case.num_reads, stride), 0x5A5A5A5A, dtype) for name, dtype in ws.SLOT_OUTPUTS.items()}
            got = case.host(awfm, stride=stride, column=column, slots=slots)
            ws.assert_equal(got, case.expected(stride=stride, column=column, slots=slots), what=f"{stride} {column}")
            for name in vc.SLOT_FIELDS:  # the guard pattern: the skipped read's element and every other column
                assert (got[name][skipped, :] == 0x5A5A5A5A).all() and (np.delete(got[name], column, axis=1) == 0x5A5A5A5A).all()
                assert (np.delete(got[name][:, column], skipped) != 0x5A5A5A5A).all()
    for stride, column in ((0, 0), (17, 0), (1, 1), (4, 4), (16, 16), (2 ** 32 - 1, 0)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, stride=stride, column=column)
        assert e.value.rc == awfm.AwFmIllegalPositionError, (stride, column)


def test_scorings_and_other_arguments_are_refused_and_zero_reads_touch_nothing(awfm):
    case = ws.edge_builder().case()
    for scoring in ((1, 0, 0, 1), (255, 255, 255, 255), (1, 255, 0, 255), (255, 0, 255, 1)):
        ws.assert_equal(case.host(awfm, scoring), case.expected(scoring), what=str(scoring))
    for scoring in ((0, 4, 6, 1), (256, 4, 6, 1), (1, 256, 6, 1), (1, 4, 256, 1), (1, 4, 6, 0), (1, 4, 6, 256), (2 ** 32 - 1,) * 4):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, scoring)
        assert e.value.rc == awfm.AwFmIllegalPositionError, scoring
    lib = awfm._lib.lib()
    costs = awfm.align_scoring()
    import ctypes as C
    assert lib.awfmScoreWindowsAffine(None, 0, None, 0, 0, 99, None, 0, None, 0, 2, None, 1) == awfm.AwFmSuccess  # numReads == 0 touches nothing
    win, out = awfm.window_inputs(0, 0, 0, 0, 0, 0), awfm.window_score_outputs()
    assert lib.awfmScoreWindowsAffine(C.byref(win), 1, C.byref(costs), 0, 1, 0, None, 0, None, 0, 2, C.byref(out), 1) == -4  # AwFmNullPtrError
    assert lib.awfmScoreWindowsAffine(None, 1, C.byref(costs), 0, 1, 0, None, 0, None, 0, 2, C.byref(out), 1) == -4  # AwFmNullPtrError


def test_min_score_at_the_score_and_one_above_it(awfm):
    b = ws.edge_builder()
    case = b.case()
    r = b.names.index("clips at both ends of the read")  # score 12
    for min_score, found in ((12, True), (13, False), (0, True), (2 ** 32 - 1, False)):
        got = case.host(awfm, min_score=min_score)
        ws.assert_equal(got, case.expected(min_score=min_score), what=str(min_score))
        assert int(got["scores"][r]) == 12 and int(got["readBegins"][r]) == 2  # the per-read outputs do not depend on it
        assert (int(got["chainAnchors"][r, 0]) == 1) == found and (int(got["sequences"][r, 0]) == 4) == found
        assert got["numFound"] == sum(1 for v in b.values if max(min_score, 1) <= v[0] < ws.TOO_LONG)


def test_every_output_null_in_turn_and_alone_and_both_counters_are_added_to(awfm):
    case = ws.edge_builder().case()
    want = case.expected(unscored_before=11, found_before=13)
    names = list(ws.READ_OUTPUTS) + list(vc.SLOT_FIELDS) + list(ws.COUNTERS)
    for missing in names:
        for outputs in ([n for n in names if n != missing], [missing]):
            got = case.host(awfm, outputs=outputs, unscored_before=11, found_before=13)
            assert sorted(got) == sorted(outputs)
            ws.assert_equal(got, want, names=outputs, what=str(outputs))


def test_the_limits_of_width_and_length(awfm):
    """W = 4096 and 4097 after clipping, n = 4096 and 4097: the last accepted and the first refused (a read longer than its window
    begins with the record's first characters: the whole window matches)"""
    for n, W, value in ((60, 4096, 60), (60, 4097, ws.TOO_WIDE), (4096, 300, 300), (4097, 300, ws.TOO_LONG)):
        case = ws.wide_case(n, W)
        got = case.host(awfm)
        ws.assert_equal(got, case.expected(), what=f"n={n} W={W}")
        assert int(got["scores"][0]) == value and got["numUnscored"] == (value >= ws.TOO_LONG)
    # 4097 before clipping, 4096 after it: accepted
    case = ws.wide_case(60, 4096)
    L = int(case.ends[1] - case.ends[0] - 1)
    case.begins[0], case.window_ends[0] = L - 4096, L + 1
    assert int(case.host(awfm)["scores"][0]) < ws.TOO_LONG
    ws.assert_equal(case.host(awfm), case.expected())
    # too wide comes before too long
    assert int(ws.wide_case(4097, 4097).host(awfm)["scores"][0]) == ws.TOO_WIDE


def test_inverted_and_overlong_read_offsets_and_a_record_that_leaves_the_text(awfm):
    b = ws.edge_builder()
    base = b.case()
    o = [int(v) for v in base.offsets]
    inverted = ws.Case(base.reads, b.windows, base.text, base.ends, offsets=[o[1], o[0]] + o[2:])
    got = inverted.host(awfm)
    ws.assert_equal(got, inverted.expected())
    assert int(got["scores"][0]) == ws.MALFORMED and int(got["scores"][1]) == 10
    beyond = ws.Case(base.reads, b.windows, base.text, base.ends, num_read_chars=o[-1] - 1)
    got = beyond.host(awfm)
    ws.assert_equal(got, beyond.expected())
    assert int(got["scores"][-1]) == ws.MALFORMED and int(got["scores"][0]) == 10
    ends = base.ends.copy()
    ends[-1] = base.text.size + 1  # the last record leaves the text
    leaving = ws.Case(base.reads, b.windows, base.text, ends)
    got = leaving.host(awfm)
    ws.assert_equal(got, leaving.expected())
    assert (got["scores"][leaving.sequences == len(ends) - 1] == ws.MALFORMED).all()


def test_the_two_ties_of_the_origin_rule_by_hand_computed_values(awfm):
    """a cell where M = F = E = H (the origin follows M) and a gap where opening and extending tie (opened): one hand-worked read
    each (ws.tie_builder); the restatement's walk reports that it met exactly that tie"""
    b = ws.tie_builder()
    case = b.case()
    got = case.host(awfm, ws.TIE_SCORING)
    b.check(got)
    ws.assert_equal(got, case.expected(ws.TIE_SCORING))
    for r, kind in enumerate(("MFE", "opened")):
        ties = set()
        S, E = case.record(r)
        ws.window_local(case.reads[r], bytes(case.text[S:E]), ws.TIE_SCORING, ties=ties)
        assert kind in ties, (kind, ties)


def test_random_two_letter_reads_under_scorings_full_of_ties_follow_the_walk(awfm):
    """short reads over two letters under four scorings with cheap gaps, where ties of both kinds abound: the twin's forward
    origins equal the walk back on every one of them, whatever the reads are"""
    rng = np.random.default_rng(2)
    reads, windows, records = [], [], []
    for k in range(400):
        records.append(bytes(rng.choice(np.frombuffer(b"ac", np.uint8), 14)))
        reads.append(bytes(rng.choice(np.frombuffer(b"ac", np.uint8), 9)))
        windows.append((k, 0, 14))
    text, ends = ws.text_of(records)
    case = ws.Case(reads, windows, text, ends)
    for scoring in ((1, 1, 0, 1), (1, 0, 0, 1), (2, 1, 1, 1), ws.TIE_SCORING):
        ws.assert_equal(case.host(awfm, scoring), case.expected(scoring), what=str(scoring))


def test_planted_reads_through_affine_alignment_on_the_written_slots(awfm):
    """200 planted reads of 150 characters (up to 8 % substitutions, up to two gaps of 1..3) in windows of 600: the slot goes into
    awfmAlignChainsAffine with w = 8, x = 15, which returns this call's score, begin and end and a script that replays to it for
    every read whose restated path lies in the band.  Seed 5 leaves 0 of 200 reads out of the comparison (at most 2 % may be)."""
    case = ws.planted_case(PLANTED_SEED)
    got = case.host(awfm, min_score=30, threads=4)
    ws.assert_equal(got, case.expected(min_score=30))
    assert got["numFound"] == case.num_reads and got["numUnscored"] == 0
    slots = {name: got[name] for name in vc.SLOT_FIELDS}
    aligned = awfm.align_chains_affine_host(case.read_chars, case.offsets, slots, np.zeros(case.num_reads, np.uint32), case.text, case.ends,
                                            band_pad=8, max_drift=15, max_ops=32)
    left_out = 0
    for r in range(case.num_reads):
        R = case.reads[r]
        b, e = int(case.begins[r]), int(case.window_ends[r])
        T = bytes(case.text[b:e])
        score, lowest, highest, runs = ws.unbanded_local(R, T)
        assert score == int(got["scores"][r])
        bD, eD = int(got["chainBeginDiagonals"][r, 0]) - b, int(got["chainEndDiagonals"][r, 0]) - b
        assert int(aligned["scores"][r]) <= score or int(aligned["scores"][r]) >= ws.TOO_LONG
        if abs(eD - bD) > 15 or lowest < min(bD, eD) - 8 or highest > max(bD, eD) + 8:
            left_out += 1
            continue
        for name in ("scores", "readBegins", "readEnds", "textBegins", "textEnds"):
            assert int(aligned[name][r]) == int(got[name][r]), (r, name)
        script = af.runs_of(aligned["ops"][r], int(aligned["numOps"][r]))
        chars, span, replayed, _ = ws.replay(script, R, bytes(case.text), int(aligned["textBegins"][r]))
        assert chars == len(R) and replayed == score and span == int(got["textEnds"][r]) - int(got["textBegins"][r])
    assert left_out * 50 <= case.num_reads, left_out


SANITIZER_MAIN = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "awfm_gpu.h"
static void *block(FILE *f, size_t bytes) { /* a heap block of exactly its size: the sanitizer sees every read outside it */
  void *p = malloc(bytes ? bytes : 1);
  if (bytes && fread(p, 1, bytes, f) != bytes) exit(2);
  return p;
}
int main(int argc, char **argv) {
  FILE *f = argc < 2 ? NULL : fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h[16];
  if (fread(h, 8, 16, f) != 16) return 2;
  const uint64_t numReads = h[0], stride = h[1], sizeChars = h[2], textLength = h[4], numRecords = h[5], n = numReads * stride;
  struct AwFmWindowInputs in = {0};
  in.numReadChars = h[3];
  in.readChars = block(f, sizeChars);
  in.readOffsets = block(f, (numReads + 1) * 8);
  in.windowSequences = block(f, numReads * 4);
  in.windowBegins = block(f, numReads * 8);
  in.windowEnds = block(f, numReads * 8);
  const uint8_t *text = block(f, textLength);
  const uint64_t *ends = numRecords ? block(f, numRecords * 8) : NULL;
  uint64_t unscored = h[9], found = h[9] + 1;
  const struct AwFmAlignScoring scoring = {(uint32_t)h[12], (uint32_t)h[13], (uint32_t)h[14], (uint32_t)h[15]};
  struct AwFmWindowOutputs out = {malloc(numReads * 4), malloc(numReads * 4), malloc(numReads * 4), malloc(numReads * 8), malloc(numReads * 8),
                                  calloc(n, 4), calloc(n, 4), calloc(n, 4), calloc(n, 4), calloc(n, 8), calloc(n, 8), &unscored, &found};
  if (awfmScoreWindowsAffine(&in, numReads, &scoring, (uint32_t)h[11], (uint32_t)stride, (uint32_t)h[6], text, textLength, ends, numRecords,
                             (int)h[8], &out, (unsigned)h[10]) != AwFmSuccess)
    return 3;
  fwrite(out.scores, 4, numReads, stdout);
  fwrite(out.readBegins, 4, numReads, stdout);
  fwrite(out.readEnds, 4, numReads, stdout);
  fwrite(out.textBegins, 8, numReads, stdout);
  fwrite(out.textEnds, 8, numReads, stdout);
  fwrite(out.sequences, 4, n, stdout);
  fwrite(out.chainAnchors, 4, n, stdout);
  fwrite(out.chainReadBegins, 4, n, stdout);
  fwrite(out.chainReadEnds, 4, n, stdout);
  fwrite(out.chainBeginDiagonals, 8, n, stdout);
  fwrite(out.chainEndDiagonals, 8, n, stdout);
  fwrite(&unscored, 8, 1, stdout);
  fwrite(&found, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twin indexes the read buffer and the text by offsets and windows its caller supplies: awfm_window_affine.c, the letter
    tables and the thread pool, compiled with a stand-alone main under -fsanitize=address,undefined and run as a program on the
    edge list (skewed, too), on windows of the largest width, on a record that ends at the text's last byte and on random batches
    spread over four threads, every array in a heap block of exactly its size"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "window_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_window_affine.c"), os.path.join(CSRC, "awfm_letters.c"), os.path.join(CSRC, "awfm_threads.c"),
                           "-o", exe])
    tail = ws.wide_case(40, 96)
    tail.text, tail.window_ends[0] = tail.text[:-1], 1 << 50  # the last record without its terminator, the window clipped at its end
    cases = [("edge", ws.edge_builder().case(), 1, 0, 2, 0, ws.DEFAULT), ("edge-skewed", ws.edge_builder().case(3), 4, 3, 1, 11, ws.DEFAULT),
             ("widest", ws.wide_case(70, 4096), 1, 0, 1, 0, (2, 4, 4, 2)), ("wider", ws.wide_case(70, 4097), 16, 15, 1, 0, ws.DEFAULT),
             ("tail", tail, 1, 0, 1, 0, ws.DEFAULT),
             ("random", ws.random_case(8, 300, max_length=80, clipped=0.3), 4, 1, 4, 5, (255, 255, 255, 255)),
             ("free", ws.random_case(7, 200, max_length=80), 2, 1, 4, 0, (1, 0, 0, 1)),
             ("amino", ws.random_case(9, 100, ws.AMINO, clipped=0.3), 16, 9, 4, 3, (1, 1, 0, 1))]
    for name, case, stride, column, threads, min_score, scoring in cases:
        header = np.array([case.num_reads, stride, case.read_chars.size, case.num_read_chars, case.text.size, len(case.ends), column, 0,
                           case.alphabet, 6, threads, min_score, *scoring], np.uint64)
        arrays = [header, case.read_chars, case.offsets, case.sequences, case.begins, case.window_ends, case.text, case.ends]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        zeros = {f: np.zeros((case.num_reads, stride), d) for f, d in ws.SLOT_OUTPUTS.items()}
        want = case.host(awfm, scoring, min_score=min_score, stride=stride, column=column, slots=zeros, unscored_before=6, found_before=7)
        n, at, got = case.num_reads, 0, {}
        for field, dtype, count in ([(f, d, n) for f, d in ws.READ_OUTPUTS.items()] + [(f, d, n * stride) for f, d in ws.SLOT_OUTPUTS.items()] +
                                    [("numUnscored", np.uint64, 1), ("numFound", np.uint64, 1)]):
            got[field] = np.frombuffer(run.stdout, dtype, count, at)
            at += count * np.dtype(dtype).itemsize
        for field in ws.SLOT_OUTPUTS:
            got[field] = got[field].reshape(n, stride)
        got["numUnscored"], got["numFound"] = int(got["numUnscored"][0]), int(got["numFound"][0])
        ws.assert_equal(got, want, what=name)
