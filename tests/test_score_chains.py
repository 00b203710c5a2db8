"""awfmScoreChainsAffine (include/awfm_gpu.h "slot scores and mapping quality", csrc/awfm_score_affine.c), the host twin and
checker of awfmGpuScoreChainsAffine: against a plain-Python restatement (tests/align_affine_common.py's `local` per slot, the five
per-read rules over Python integers) on random batches, against awfmAlignChainsAffine slot by slot and on its own best slots, on
the edge list of the per-read rules with hand-computed values, on the planted reads of the end-to-end test, and as a stand-alone
program under AddressSanitizer and UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
from test_align_affine import long_affine_case, long_expected  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
BATCHES = [(alphabet, C, w, x, scoring)
           for k, (width, (w, x)) in enumerate(sorted(af.BAND_SHAPES.items()))
           for alphabet, C, scoring in [((af.DNA, af.AMINO)[k % 2], (1, 4, 16)[k % 3], af.SCORINGS[k % 5]),
                                        ((af.AMINO, af.DNA)[k % 2], (4, 16, 1)[k % 3], af.SCORINGS[(k + 2) % 5])]]


def batch(alphabet, C, w, x):
    return sc.random_case(17 * C + w + x, 30 if C < 16 else 16, C, alphabet, max_length=40 + 2 * w, broken=0.08, hanging=0.3)


@pytest.mark.parametrize("alphabet,C,w,x,scoring", BATCHES)
def test_random_batches_equal_the_python_restatement_and_the_affine_call(awfm, alphabet, C, w, x, scoring):
    """every band shape of ac.BAND_SHAPES in both alphabets with C = 1, 4 and 16 under the five scorings; unused, malformed,
    too wide and hanging slots among them"""
    case = batch(alphabet, C, w, x)
    want = case.expected_scores(w, x, scoring, min_score=3, cap=60, unscored_before=5, mapped_before=7)
    got = case.score(awfm, w, x, scoring, min_score=3, cap=60, unscored_before=5, mapped_before=7, fill=0x5A, threads=3)
    sc.assert_equal(got, want, what=f"C={C} w={w} x={x} {scoring}")
    # slot by slot what awfmAlignChainsAffine gives with slots[:] = j
    sc.assert_equal(got, case.by_the_affine_call(awfm, w, x, scoring), what="against awfmAlignChainsAffine")
    # and on the new call's best slots the existing call returns the best scores
    case.chosen = got["bestSlots"]
    aligned = case.host(awfm, w, x, scoring, max_ops=1, outputs=["scores"])
    mapped = got["bestSlots"] != sc.NO_SLOT
    assert np.array_equal(aligned["scores"][mapped], got["bestScores"][mapped]) and (aligned["scores"][~mapped] == sc.NONE).all()
    assert got["numMapped"] == 7 + int(mapped.sum())


def test_the_batches_hold_every_kind_of_slot(awfm):
    kinds, hanging, seconds = set(), 0, 0
    for alphabet, C, w, x, scoring in BATCHES[::3]:
        case = batch(alphabet, C, w, x)
        got = case.score(awfm, w, x, scoring)
        kinds |= set(int(v) for v in got["slotScores"].ravel() if v >= sc.TOO_LONG)
        seconds += int((got["secondSlots"] != sc.NO_SLOT).sum())
        for j in range(C):
            case.chosen = np.full(case.num_reads, j, np.uint32)
            hanging += sum(sc.ac.Case.status(case, r, w, x) == sc.ac.OVERHANG for r in range(case.num_reads))
    assert {sc.NONE, sc.MALFORMED, sc.TOO_WIDE} <= kinds and hanging >= 5 and seconds >= 5


def test_a_band_of_65_diagonals_bad_caps_scorings_and_other_arguments_are_refused(awfm):
    case = sc.rules_builder().case()
    for kw in (dict(w=32, x=0), dict(w=0, x=64), dict(w=31, x=2), dict(w=2 ** 31, x=2 ** 31), dict(w=8, x=15, cap=255), dict(w=8, x=15, cap=2 ** 32 - 1)):
        with pytest.raises(awfm.AwFmError) as e:
            case.score(awfm, **kw)
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    assert (case.score(awfm, 8, 15, cap=0)["mappingQualities"] == 0).all()
    assert int(case.score(awfm, 8, 15, cap=254)["mappingQualities"].max()) == 254
    assert case.score(awfm, 0, 63)["slotScores"].shape == (case.num_reads, 4)
    for min_score in (0, 1, 2 ** 32 - 1):  # any value
        case.score(awfm, 8, 15, min_score=min_score)
    # every scoring bound and one beyond
    for scoring in ((1, 0, 0, 1), (255, 255, 255, 255), (1, 255, 0, 255), (255, 0, 255, 1)):
        case.score(awfm, 8, 15, scoring)
    for scoring in ((0, 4, 6, 1), (256, 4, 6, 1), (1, 256, 6, 1), (1, 4, 256, 1), (1, 4, 6, 0), (1, 4, 6, 256), (2 ** 32 - 1,) * 4):
        with pytest.raises(awfm.AwFmError) as e:
            case.score(awfm, 8, 15, scoring)
        assert e.value.rc == awfm.AwFmIllegalPositionError, scoring
    lib = awfm._lib.lib()
    costs = awfm.align_scoring()
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmScoreChainsAffine(empty, 0, 4, 8, 15, None, 0, 255, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmScoreChainsAffine(empty, 1, 4, 8, 15, costs, 0, 60, None, 0, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == -4  # AwFmNullPtrError
    slots = {name: np.zeros((1, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
    text = (case.text.ctypes.data, case.text.size)
    assert lib.awfmScoreChainsAffine(vin, 1, 1, 8, 15, None, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == -4  # no scoring
    assert lib.awfmScoreChainsAffine(vin, 1, 1, 8, 15, costs, 0, 60, *text, None, 0, af.DNA, None, 1) == -4  # no outputs
    assert lib.awfmScoreChainsAffine(vin, 1, 1, 8, 15, costs, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == awfm.AwFmSuccess
    for C in (0, 17):
        assert lib.awfmScoreChainsAffine(vin, 1, C, 8, 15, costs, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == awfm.AwFmIllegalPositionError


@pytest.mark.parametrize("C", [4, 1, 16])
def test_edge_list_of_the_read_rules_by_hand_computed_values(awfm, C):
    b = sc.rules_builder(C)
    case = b.case()
    got = case.score(awfm, 8, 15, unscored_before=9, mapped_before=2, fill=0xC3)
    b.check(got)
    assert got["numUnscored"] == 9 + b.unscored() and got["numMapped"] == 2 + b.mapped()
    assert b.mapped() >= (10 if C > 1 else 1) and (b.unscored() == 2) == (C > 1)
    sc.assert_equal(got, case.expected_scores(8, 15, unscored_before=9, mapped_before=2), what="restatement")
    r = b.names.index("one slot: second is 0 and mapq = cap")
    assert (int(got["slotReadEnds"][r, 0]), int(got["slotTextEnds"][r, 0])) == (100, 110)
    if C > 1:
        r = b.names.index("a duplicate: diagonals 10 and 12 of one sequence give one end cell")
        assert got["slotReadEnds"][r, :2].tolist() == [100, 100] and got["slotTextEnds"][r, :2].tolist() == [110, 110]
        r = b.names.index("best 100, second 37")
        assert (int(got["slotReadEnds"][r, 1]), int(got["slotTextEnds"][r, 1]), int(got["mappingQualities"][r])) == (57, 77, 37)
    for skew in (1, 2, 3):  # the same reads further into their buffer
        sc.assert_equal(b.case(skew).score(awfm, 8, 15, unscored_before=9, mapped_before=2), got, what=f"skew {skew}")


def test_min_score_at_the_best_score_one_above_it_and_above_the_second(awfm):
    b = sc.rules_builder()
    case = b.case()
    plain = case.score(awfm, 8, 15)
    at = case.score(awfm, 8, 15, min_score=100, mapped_before=11)
    r = b.names.index("best 100, second 37")
    d = b.names.index("a duplicate plus a true second")
    assert [int(at[f][r]) for f in sc.READ_OUTPUTS] == [0, 100, sc.NO_SLOT, 0, 60]  # the best counts, the second lies below and is ignored
    assert [int(at[f][d]) for f in sc.READ_OUTPUTS] == [0, 100, sc.NO_SLOT, 0, 60]
    assert np.array_equal(at["bestSlots"], plain["bestSlots"]) and at["numMapped"] == 11 + plain["numMapped"]
    assert np.array_equal(at["slotScores"], plain["slotScores"])  # minScore changes no slot's own outputs
    for min_score in (37, 38):
        got = case.score(awfm, 8, 15, min_score=min_score)
        assert [int(got[f][r]) for f in sc.READ_OUTPUTS] == ([0, 100, 1, 37, 37] if min_score == 37 else [0, 100, sc.NO_SLOT, 0, 60])
        sc.assert_equal(got, case.expected_scores(8, 15, min_score=min_score))
    above = case.score(awfm, 8, 15, min_score=101, mapped_before=11)
    assert (above["bestSlots"] == sc.NO_SLOT).all() and (above["secondSlots"] == sc.NO_SLOT).all() and above["numMapped"] == 11
    assert not above["bestScores"].any() and not above["secondScores"].any() and not above["mappingQualities"].any()
    assert above["numUnscored"] == plain["numUnscored"]


def test_best_100_second_37_under_other_caps(awfm):
    b = sc.rules_builder()
    r = b.names.index("best 100, second 37")
    for cap, quality in ((60, 37), (0, 0), (254, 160), (1, 0), (100, 63)):
        got = b.case().score(awfm, 8, 15, cap=cap)
        assert int(got["mappingQualities"][r]) == quality and int(got["mappingQualities"][b.names.index("one slot: second is 0 and mapq = cap")]) == cap


def test_every_output_null_in_turn_and_both_counters_are_added_to(awfm):
    case = sc.random_case(3, 50, 4, hanging=0.2)
    want = case.score(awfm, 2, 3)
    assert want["numUnscored"] > 0 and want["numMapped"] > 0
    for missing in sc.ALL_OUTPUTS:
        for outputs in ([n for n in sc.ALL_OUTPUTS if n != missing], [missing]):
            got = case.score(awfm, 2, 3, outputs=outputs, fill=0xC3)
            assert sorted(got) == sorted(outputs)
            sc.assert_equal(got, want, names=outputs, what=str(outputs))
    got = case.score(awfm, 2, 3, unscored_before=2 ** 40, mapped_before=2 ** 41)
    assert got["numUnscored"] == 2 ** 40 + want["numUnscored"] and got["numMapped"] == 2 ** 41 + want["numMapped"]


def long_scored_case(n=af.MAX_LENGTH, C=1):
    """long_case's two reads (n characters and n + 1) with their one slot C times"""
    case = long_affine_case(n)
    slots = {name: np.repeat(a, C, axis=1) for name, a in case.slots.items()}
    return sc.Case(case.read_chars.tobytes(), case.offsets, slots, [0, 0], case.text.tobytes(), case.ends)


def test_a_read_of_two_to_the_sixteen_characters_and_one_more(awfm):
    n = af.MAX_LENGTH
    score, _, read_end, _, text_end, _ = long_expected(n)
    got = long_scored_case().score(awfm, 8, 15)
    assert got["slotScores"].tolist() == [[score], [sc.TOO_LONG]] and got["slotReadEnds"].tolist() == [[read_end], [0]]
    assert got["slotTextEnds"].tolist() == [[text_end], [0]] and got["numUnscored"] == 1 and got["numMapped"] == 1
    assert got["bestSlots"].tolist() == [0, sc.NO_SLOT] and got["bestScores"].tolist() == [score, 0] and got["mappingQualities"].tolist() == [60, 0]
    got = long_scored_case().score(awfm, 8, 15, (255, 255, 255, 255), cap=254)  # the largest score there is: 254 * best fits 32 bits
    assert got["bestScores"].tolist() == [255 * (n - 3 - 2 - 2), 0] and got["mappingQualities"].tolist() == [254, 0]


def test_the_planted_reads_of_the_end_to_end_test_by_the_host_twins_alone(awfm, tmp_path):
    """the conditions tests/test_gpu_score_chains.py puts on EVERY planted read of its end-to-end test, met by the host's pipeline
    and the host twin on the same FASTA file, reads and parameters: the own record is best, a decoy that has a slot is the
    strictly smaller second with mapq > 0, the reads of the duplicated record meet their copy at mapq 0; and awfmAlignChainsAffine
    on these best slots returns the best scores"""
    case, records, planted, decoy_of, copies = sc.e2e_host_case(awfm, str(tmp_path))
    got = case.score(awfm, vc.E2E_W, vc.E2E_X, cap=sc.E2E_CAP)
    decoys_met, copies_met = sc.assert_planted_reads_mapped(case, got, planted, decoy_of, copies)
    print("planted", sum(p is not None for p in planted), "decoys", len(decoy_of), "met", decoys_met, "copies met", copies_met)
    assert decoys_met >= len(decoy_of) // 2 and copies_met >= 1
    case.chosen = got["bestSlots"]
    aligned = case.host(awfm, vc.E2E_W, vc.E2E_X, max_ops=32)
    mapped = got["bestSlots"] != sc.NO_SLOT
    assert np.array_equal(aligned["scores"][mapped], got["bestScores"][mapped]) and np.array_equal(aligned["readEnds"][mapped], got["slotReadEnds"][mapped, got["bestSlots"][mapped]])


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
  const uint64_t numReads = h[0], slots = h[1], sizeChars = h[2], textLength = h[4], numRecords = h[5], n = numReads * slots;
  struct AwFmVerifyInputs in = {0};
  in.numReadChars = h[3];
  in.readChars = block(f, sizeChars);
  in.readOffsets = block(f, (numReads + 1) * 8);
  in.sequences = block(f, n * 4);
  in.chainAnchors = block(f, n * 4);
  in.chainReadBegins = block(f, n * 4);
  in.chainReadEnds = block(f, n * 4);
  in.chainBeginDiagonals = block(f, n * 8);
  in.chainEndDiagonals = block(f, n * 8);
  const uint8_t *text = block(f, textLength);
  const uint64_t *ends = numRecords ? block(f, numRecords * 8) : NULL;
  uint64_t unscored = h[9], mapped = h[9] + 1;
  const struct AwFmAlignScoring scoring = {(uint32_t)h[12], (uint32_t)h[13], (uint32_t)h[14], (uint32_t)h[15]};
  struct AwFmSlotScoreOutputs out = {malloc(n * 4), malloc(n * 4), malloc(n * 8), malloc(numReads * 4), malloc(numReads * 4),
                                     malloc(numReads * 4), malloc(numReads * 4), malloc(numReads), &unscored, &mapped};
  if (awfmScoreChainsAffine(&in, numReads, (uint32_t)slots, (uint32_t)h[6], (uint32_t)h[7], &scoring, (uint32_t)h[11], 60, text, textLength,
                            ends, numRecords, (int)h[8], &out, (unsigned)h[10]) != AwFmSuccess)
    return 3;
  fwrite(out.slotScores, 4, n, stdout);
  fwrite(out.slotReadEnds, 4, n, stdout);
  fwrite(out.slotTextEnds, 8, n, stdout);
  fwrite(out.bestSlots, 4, numReads, stdout);
  fwrite(out.bestScores, 4, numReads, stdout);
  fwrite(out.secondSlots, 4, numReads, stdout);
  fwrite(out.secondScores, 4, numReads, stdout);
  fwrite(out.mappingQualities, 1, numReads, stdout);
  fwrite(&unscored, 8, 1, stdout);
  fwrite(&mapped, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twin indexes the read buffer and the text by offsets and diagonals its caller supplies: awfm_score_affine.c, the letter
    tables and the thread pool, compiled with a stand-alone main under -fsanitize=address,undefined and run as a program on the
    rule list, on the affine edge lists (every malformed shape and every overhang in them), on a tail that ends at the text's
    last byte and on random batches spread over four threads, every array in a heap block of exactly its size"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "score_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_score_affine.c"), os.path.join(CSRC, "awfm_letters.c"), os.path.join(CSRC, "awfm_threads.c"),
                           "-o", exe])
    cases = [("rules", sc.rules_builder().case(), 8, 15, 2, 0, af.DEFAULT), ("rules-16", sc.rules_builder(16).case(3), 8, 15, 1, 38, af.DEFAULT),
             ("edge", sc.as_scored(af.edge_builder(2, 3).case()), 2, 3, 2, 0, af.DEFAULT),
             ("edge-wide", sc.as_scored(af.edge_builder(24, 15).case(3)), 24, 15, 1, 2, af.DEFAULT),
             ("outside", sc.as_scored(af.outside_builder().case(1)), 0, 0, 1, 0, af.DEFAULT),
             ("tail", sc.as_scored(af.tail_case(113).case()), 2, 3, 1, 0, (2, 4, 4, 2)),
             ("random", sc.random_case(8, 400, 4, max_length=80, hanging=0.3), 4, 7, 4, 5, (255, 255, 255, 255)),
             ("narrow", sc.random_case(7, 200, 4, max_length=80, hanging=0.5), 0, 0, 4, 0, (1, 0, 0, 1)),
             ("amino", sc.random_case(9, 100, 16, af.AMINO, hanging=0.3), 8, 15, 4, 3, (1, 1, 0, 1))]
    for name, case, w, x, threads, min_score, scoring in cases:
        header = np.array([case.num_reads, case.C, case.read_chars.size, case.num_read_chars, case.text.size, len(case.ends), w, x, case.alphabet,
                           6, threads, min_score, *scoring], np.uint64)
        arrays = [header, case.read_chars, case.offsets] + [case.slots[f] for f in vc.SLOT_FIELDS] + [case.text, case.ends]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        want = case.score(awfm, w, x, scoring, min_score=min_score, unscored_before=6, mapped_before=7)
        n, at, got = case.num_reads, 0, {}
        for field, dtype, count in ([(f, d, n * case.C) for f, d in sc.SLOT_OUTPUTS.items()] + [(f, d, n) for f, d in sc.READ_OUTPUTS.items()] +
                                    [("numUnscored", np.uint64, 1), ("numMapped", np.uint64, 1)]):
            got[field] = np.frombuffer(run.stdout, dtype, count, at)
            at += count * np.dtype(dtype).itemsize
        for field in sc.SLOT_OUTPUTS:
            got[field] = got[field].reshape(n, case.C)
        got["numUnscored"], got["numMapped"] = int(got["numUnscored"][0]), int(got["numMapped"][0])
        sc.assert_equal(got, want, what=name)
