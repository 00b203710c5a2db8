"""awfmAlignChainsAffine (include/awfm_gpu.h "affine alignment", csrc/awfm_align_affine.c), the host twin and checker of
awfmGpuAlignChainsAffine: against a plain-Python restatement of the definition (dicts of cells, exact integers, the tie and state
rules as written) on random batches, on the edge list with hand-computed values, by replaying every script (the invariants the
header states), against an unbanded local Gotoh pass on planted reads, and as a stand-alone program under AddressSanitizer and
UBSan."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import verify_chains_common as vc  # noqa: E402
from test_align_chains import long_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")
ALL_OUTPUTS = list(af.READ_OUTPUTS) + ["ops"] + list(af.COUNTERS)


@pytest.mark.parametrize("alphabet,C,w,x,scoring", [
    (af.DNA, 4, 0, 0, af.DEFAULT), (af.AMINO, 1, 7, 0, (2, 4, 4, 2)), (af.DNA, 16, 7, 1, (1, 1, 0, 1)), (af.AMINO, 4, 8, 0, (255, 255, 255, 255)),
    (af.DNA, 1, 15, 0, (1, 0, 0, 1)), (af.DNA, 4, 15, 1, af.DEFAULT), (af.AMINO, 16, 16, 0, af.DEFAULT), (af.DNA, 4, 31, 0, (2, 4, 4, 2)),
    (af.AMINO, 1, 31, 1, (1, 1, 0, 1)), (af.DNA, 4, 2, 3, (255, 255, 255, 255)), (af.AMINO, 4, 2, 3, (1, 0, 0, 1)), (af.DNA, 1, 8, 15, af.DEFAULT)])
def test_random_batches_equal_the_python_restatement_and_replay(awfm, alphabet, C, w, x, scoring):
    """band widths 1, 15, 16, 17, 31, 32, 33, 63, 64, 8 and 32 under the five scorings; some slots unused, some malformed, some
    whose band hangs over a record end or (w = 0) lies outside the record"""
    case = af.random_case(13 * C + w + x, 40 if C < 16 else 30, C, alphabet, max_length=40 + 2 * w, broken=0.08, hanging=0.3)
    max_ops = 12
    want = case.expected(w, x, scoring, max_ops, unaligned_before=5, truncated_before=7)
    got = case.host(awfm, w, x, scoring, max_ops, unaligned_before=5, truncated_before=7, fill=0x5A, threads=3)
    af.assert_equal(got, want, what=f"C={C} w={w} x={x} {scoring}", fill=0x5A)
    kinds = set(int(v) for v in want["scores"] if v >= af.TOO_LONG)
    assert {af.NONE, af.MALFORMED} <= kinds and want["numUnaligned"] > 5
    hanging = sum(ac.Case.status(case, r, w, x) == ac.OVERHANG for r in range(case.num_reads))
    assert hanging >= 2  # reads chain alignment refuses
    assert af.assert_scripts_replay(case, got, w, x, scoring, max_ops) >= 4  # (with x = 0 every read with an indel in its chain is too wide)


def test_a_band_of_65_diagonals_scorings_and_other_arguments_out_of_range_are_refused(awfm):
    case = af.edge_builder(2, 3).case()
    for kw in (dict(w=32, x=0), dict(w=0, x=64), dict(w=31, x=2), dict(w=2 ** 31, x=2 ** 31), dict(w=2, x=3, max_ops=0),
               dict(w=2, x=3, max_ops=af.MAX_OPS + 1)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, **kw)
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    assert case.host(awfm, 0, 63, max_ops=af.MAX_OPS)["ops"].shape == (case.num_reads, af.MAX_OPS)
    # every scoring bound and one beyond
    for scoring in ((1, 0, 0, 1), (255, 255, 255, 255), (1, 255, 0, 255), (255, 0, 255, 1)):
        case.host(awfm, 2, 3, scoring)
    for scoring in ((0, 4, 6, 1), (256, 4, 6, 1), (1, 256, 6, 1), (1, 4, 256, 1), (1, 4, 6, 0), (1, 4, 6, 256), (2 ** 32 - 1,) * 4):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, 2, 3, scoring)
        assert e.value.rc == awfm.AwFmIllegalPositionError, scoring
    lib = awfm._lib.lib()
    costs = awfm.align_scoring()
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmAlignChainsAffine(empty, None, 0, 4, 2, 3, None, 8, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmAlignChainsAffine(empty, None, 1, 4, 2, 3, costs, 8, None, 0, None, 0, af.DNA, awfm.affine_outputs(), 1) == -4  # AwFmNullPtrError
    slots = {name: np.zeros((1, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
    text = (case.text.ctypes.data, case.text.size)
    assert lib.awfmAlignChainsAffine(vin, None, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == -4  # no slots
    assert lib.awfmAlignChainsAffine(vin, case.chosen.ctypes.data, 1, 1, 2, 3, None, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == -4  # no scoring
    assert lib.awfmAlignChainsAffine(vin, case.chosen.ctypes.data, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, None, 1) == -4  # no outputs
    assert lib.awfmAlignChainsAffine(vin, case.chosen.ctypes.data, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == awfm.AwFmSuccess
    for C in (0, 17):
        rc = lib.awfmAlignChainsAffine(vin, case.chosen.ctypes.data, 1, C, 2, 3, costs, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1)
        assert rc == awfm.AwFmIllegalPositionError


@pytest.mark.parametrize("w,x", [(2, 3), (8, 15), (3, 4), (24, 15)])
def test_edge_list_by_hand_computed_values(awfm, w, x):
    b = af.edge_builder(w, x)
    case = b.case()
    got = case.host(awfm, w, x, max_ops=8, unaligned_before=9, truncated_before=2, fill=0xC3)
    b.check(got, 8)
    assert got["numUnaligned"] == 9 + b.unaligned() and got["numTruncated"] == 2
    af.assert_equal(got, case.expected(w, x, max_ops=8, unaligned_before=9, truncated_before=2), what="restatement", fill=0xC3)
    assert af.assert_scripts_replay(case, got, w, x, af.DEFAULT, 8) >= 25
    for skew in (1, 2, 3):  # the same reads further into their buffer
        af.assert_equal(b.case(skew).host(awfm, w, x, max_ops=8, unaligned_before=9, truncated_before=2), got, what=f"skew {skew}")


def test_bands_outside_the_record_unit_gap_costs_and_what_chain_alignment_does_with_the_same_reads(awfm):
    b = af.outside_builder()
    got = b.case().host(awfm, 0, 0, max_ops=8)
    b.check(got, 8)
    af.assert_equal(got, b.case().expected(0, 0, max_ops=8))
    assert got["numUnaligned"] == 0
    b = af.unit_builder()
    got = b.case().host(awfm, 2, 3, (1, 1, 0, 1), max_ops=8)
    b.check(got, 8)
    af.assert_equal(got, b.case().expected(2, 3, (1, 1, 0, 1), max_ops=8))
    # the same reads under chain alignment: the two-gap read gets two separate 1-gaps there, the overhanging ones nothing
    b = af.edge_builder(2, 3)
    case = b.case()
    unit = ac.Case.host(case, awfm, 2, 3, max_ops=8)
    r = b.names.index("one 2-gap where unit costs take two 1-gaps")
    runs = ac.runs_of(unit["ops"][r], int(unit["numOps"][r]))
    assert int(unit["editDistances"][r]) == 2 and [run for run, op in runs if op == ac.OP_D] == [1, 1], ac.cigar(runs)
    refused = [name for name, d in zip(b.names, unit["editDistances"]) if d == ac.OVERHANG]
    assert sorted(refused) == ["3 characters over the record's first character", "3 characters over the record's last character"]


def test_one_sequence_without_a_record_table_and_the_amino_alphabet(awfm):
    slots = {name: np.array([[v]], vc.SLOT_DTYPES[name]) for name, v in zip(vc.SLOT_FIELDS, (0, 1, 0, 4, 2, 2))}

    def call(read, text, alphabet, w=1, x=1):
        got = af.Case(read, [0, 4], slots, [0], text, None, alphabet).host(awfm, w, x)
        return (int(got["scores"][0]), int(got["readBegins"][0]), int(got["readEnds"][0]), int(got["textBegins"][0]), int(got["textEnds"][0]),
                af.cigar(af.runs_of(got["ops"][0], int(got["numOps"][0]))))

    # x matches nothing, not even itself: 2 - 4 < 0, and the d behind it is worth 1 < 2; case is ignored
    assert call(b"ARXD", b"mkarxdmk", af.AMINO) == (2, 0, 2, 2, 4, "2=2S")
    assert call(b"ARND", b"mkarndmk", af.AMINO) == (4, 0, 4, 2, 6, "4=")
    assert call(b"acgt", b"ttACGTtt", af.DNA, 0, 0) == (4, 0, 4, 2, 6, "4=")
    slots["sequences"][0, 0] = 1
    assert call(b"ARXD", b"mkarxdmk", af.AMINO)[0] == af.MALFORMED


def test_max_ops_exactly_the_number_of_runs_and_one_less(awfm):
    """guard words around every row: a row is written up to its runs or, truncated, nowhere outside itself"""
    b = af.edge_builder(2, 3)
    case = b.case()
    full = case.host(awfm, 2, 3, max_ops=8)
    most = int(full["numOps"].max())
    assert most == 4 and full["numTruncated"] == 0  # 20=2D1X20=
    lib, costs = awfm._lib.lib(), awfm.align_scoring()
    for max_ops in (most, most - 1):
        n = case.num_reads
        # the rows of ops as the middle third of rows three times as wide: the words on either side of a row are its guards
        wide = np.full((n, 3 * max_ops), 0xA5A5A5A5, np.uint32)
        rows = {name: np.full(n + 2, 0xA5, dtype) for name, dtype in af.READ_OUTPUTS.items()}
        counters = np.array([0xA5A5, 4, 6, 0xA5A5], np.uint64)
        for r in range(n):  # a read at a time, so that every row lies between words of its own
            one = af.Case(case.read(r), [0, len(case.read(r))], {name: case.slots[name][r:r + 1] for name in vc.SLOT_FIELDS}, case.chosen[r:r + 1],
                          case.text.tobytes(), case.ends)
            vin = awfm.verify_inputs(one.read_chars.ctypes.data if one.read_chars.size else counters.ctypes.data, one.num_read_chars,
                                     one.offsets.ctypes.data, **{name: a.ctypes.data for name, a in one.slots.items()})
            out = awfm.affine_outputs(ops=wide[r, max_ops:].ctypes.data, numUnaligned=counters[1:].ctypes.data, numTruncated=counters[2:].ctypes.data,
                                      **{name: a[r + 1:].ctypes.data for name, a in rows.items()})
            assert lib.awfmAlignChainsAffine(vin, one.chosen.ctypes.data, 1, 1, 2, 3, costs, max_ops, one.text.ctypes.data, one.text.size,
                                             one.ends.ctypes.data, len(one.ends), af.DNA, out, 1) == awfm.AwFmSuccess
        assert (wide[:, :max_ops] == 0xA5A5A5A5).all() and (wide[:, 2 * max_ops:] == 0xA5A5A5A5).all()
        truncated = full["numOps"] > max_ops
        assert counters.tolist() == [0xA5A5, 4 + full["numUnaligned"], 6 + int(truncated.sum()), 0xA5A5] and truncated.sum() == (max_ops < most)
        for name, a in rows.items():
            assert np.array_equal(a[1:-1], full[name]) and a[0] == a[-1] == 0xA5, name
        for r in range(n):
            k = int(full["numOps"][r])
            if k <= max_ops:
                assert np.array_equal(wide[r, max_ops:max_ops + k], full["ops"][r, :k]) and (wide[r, max_ops + k:2 * max_ops] == 0xA5A5A5A5).all(), r


def test_every_output_null_in_turn_and_both_counters_are_added_to(awfm):
    case = af.random_case(3, 50, 4, hanging=0.2)
    want = case.host(awfm, 2, 3, max_ops=3)
    assert want["numUnaligned"] > 0 and want["numTruncated"] > 0
    for missing in ALL_OUTPUTS:
        for outputs in ([n for n in ALL_OUTPUTS if n != missing], [missing]):
            got = case.host(awfm, 2, 3, max_ops=3, outputs=outputs, fill=0xC3)
            assert sorted(got) == sorted(outputs)
            if "ops" not in outputs or "numOps" in outputs:
                af.assert_equal(got, want, names=outputs, what=str(outputs))
            else:
                af.assert_equal(dict(got, numOps=want["numOps"]), want, names=outputs, what=str(outputs))
    got = case.host(awfm, 2, 3, max_ops=3, unaligned_before=2 ** 40, truncated_before=2 ** 41)
    assert got["numUnaligned"] == 2 ** 40 + want["numUnaligned"] and got["numTruncated"] == 2 ** 41 + want["numTruncated"]


def test_read_offsets_that_are_inverted_or_leave_the_buffer(awfm):
    b = af.Builder([b"gatcctgaagtcatgc"])
    for k in range(4):
        b.add(f"read {k}", b"gatcctgaagtcatgc"[4 * k:4 * k + 4], 0, 4 * k, 4 * k, None)
    case = b.case()
    case.offsets = np.array([0, 4, 3, 12, 17], np.uint64)  # read 1 inverted, read 2 nine characters long, read 3 beyond the 16
    got = case.host(awfm, 2, 3)
    assert got["scores"].tolist() == [4, af.MALFORMED, int(case.expected(2, 3)["scores"][2]), af.MALFORMED] and got["numUnaligned"] == 2
    af.assert_equal(got, case.expected(2, 3))
    case.num_read_chars = 11  # now read 2 leaves it too
    assert case.host(awfm, 2, 3)["scores"].tolist() == [4, af.MALFORMED, af.MALFORMED, af.MALFORMED]


@pytest.mark.parametrize("length", range(96, 112))
def test_last_record_ending_at_the_texts_last_byte(awfm, length):
    b = af.tail_case(length)
    got = b.case().host(awfm, 2, 3)
    b.check(got, 32)


def long_affine_case(n=af.MAX_LENGTH):
    return af.as_affine(long_case(n))


def long_expected(n):
    """long_case's first read: n characters on diagonal 20 with substitutions at 0, 1000, n / 2, n - 2 and n - 1: the first and the
    last two are clipped, the other two are kept -> (score, readBegin, readEnd, textBegin, textEnd, cigar)"""
    return n - 3 - 2 - 8, 1, n - 2, 21, 20 + n - 2, f"1S999=1X{n // 2 - 1001}=1X{n - 3 - n // 2}=2S"


def test_too_long_at_two_to_the_sixteen_and_one_more(awfm):
    n = af.MAX_LENGTH
    for scoring, score in ((af.DEFAULT, long_expected(n)[0]), ((255, 255, 255, 255), 255 * (n - 3 - 2 - 2))):
        got = long_affine_case().host(awfm, 8, 15, scoring)
        assert got["scores"].tolist() == [score, af.TOO_LONG] and got["numUnaligned"] == 1 and got["numTruncated"] == 0
        have = tuple(int(got[f][0]) for f in ("readBegins", "readEnds", "textBegins", "textEnds")) + (af.cigar(af.runs_of(got["ops"][0], int(got["numOps"][0]))),)
        assert have == long_expected(n)[1:] and int(got["editDistances"][0]) == 2
        assert [int(got[f][1]) for f in af.READ_OUTPUTS if f != "scores"] == [0] * 6


def test_planted_reads_against_the_unbanded_local_alignment(awfm):
    """300 planted reads of 30..150 characters, 3 % substitutions, at most 4 inserted plus deleted characters, w = 8 on the true
    diagonals, (1, 4, 6, 1): the banded score is never above the unbanded one and equals it whenever the unbanded path lies inside
    [lo, hi].  That holds for all 300 reads (the bar: 9 in 10); the Python restatement alone agrees on every tenth of them."""
    case = af.planted_case()
    w, x = 8, 15
    got = case.host(awfm, w, x, max_ops=64, threads=4)
    assert got["numUnaligned"] == 0 and got["numTruncated"] == 0
    inside = 0
    for r in range(case.num_reads):
        S, E, lo, hi = case.status(r, w, x)
        R, T = case.read(r), bytes(case.text[S:E])
        full, lowest, highest, runs = af.unbanded_local(R, T)
        if r < 4:  # the prefix maximum is the recurrence
            assert af.unbanded_local(R, T, sequential=True) == (full, lowest, highest, runs)
        assert int(got["scores"][r]) <= full, r
        if lo <= lowest and highest <= hi:
            inside += 1
            assert int(got["scores"][r]) == full, r
            if r % 10 == 0:
                assert af.local(R, T, lo, hi)[0] == full, r
    print("unbanded path inside the band:", inside, "of", case.num_reads)
    assert inside >= 270
    assert af.assert_scripts_replay(case, got, w, x, af.DEFAULT, 64) == case.num_reads


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
  const uint64_t numReads = h[0], slots = h[1], sizeChars = h[2], textLength = h[4], numRecords = h[5], n = numReads * slots, maxOps = h[11];
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
  const uint32_t *chosen = block(f, numReads * 4);
  const uint8_t *text = block(f, textLength);
  const uint64_t *ends = numRecords ? block(f, numRecords * 8) : NULL;
  uint64_t unaligned = h[9], truncated = h[9] + 1;
  const struct AwFmAlignScoring scoring = {(uint32_t)h[12], (uint32_t)h[13], (uint32_t)h[14], (uint32_t)h[15]};
  struct AwFmAffineOutputs out = {malloc(numReads * 4), malloc(numReads * 4), malloc(numReads * 4), malloc(numReads * 4), malloc(numReads * 8),
                                  malloc(numReads * 8), malloc(numReads * 4), calloc(numReads * maxOps, 4), &unaligned, &truncated};
  if (awfmAlignChainsAffine(&in, chosen, numReads, (uint32_t)slots, (uint32_t)h[6], (uint32_t)h[7], &scoring, (uint32_t)maxOps, text, textLength,
                            ends, numRecords, (int)h[8], &out, (unsigned)h[10]) != AwFmSuccess)
    return 3;
  fwrite(out.scores, 4, numReads, stdout);
  fwrite(out.editDistances, 4, numReads, stdout);
  fwrite(out.readBegins, 4, numReads, stdout);
  fwrite(out.readEnds, 4, numReads, stdout);
  fwrite(out.textBegins, 8, numReads, stdout);
  fwrite(out.textEnds, 8, numReads, stdout);
  fwrite(out.numOps, 4, numReads, stdout);
  fwrite(out.ops, 4, numReads * maxOps, stdout);
  fwrite(&unaligned, 8, 1, stdout);
  fwrite(&truncated, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twin indexes the read buffer, the text and its trace table by offsets and diagonals its caller supplies:
    awfm_align_affine.c, the letter tables and the thread pool, compiled with a stand-alone main under
    -fsanitize=address,undefined, run on the edge lists (every malformed shape and every overhang in them), on the tails that
    end at the text's last byte and on random batches spread over four threads, every array in a heap block of exactly its size"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "affine_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_align_affine.c"), os.path.join(CSRC, "awfm_letters.c"), os.path.join(CSRC, "awfm_threads.c"),
                           "-o", exe])
    cases = [("edge", af.edge_builder(2, 3).case(), 2, 3, 2, 2, af.DEFAULT), ("edge-wide", af.edge_builder(24, 15).case(3), 24, 15, 1, 8, af.DEFAULT),
             ("outside", af.outside_builder().case(1), 0, 0, 1, 8, af.DEFAULT), ("tail", af.tail_case(113).case(), 2, 3, 1, 4, (2, 4, 4, 2)),
             ("random", af.random_case(8, 400, 4, max_length=80, hanging=0.3), 4, 7, 4, 6, (255, 255, 255, 255)),
             ("narrow", af.random_case(7, 200, 4, max_length=80, hanging=0.5), 0, 0, 4, 6, (1, 0, 0, 1)),
             ("amino", af.random_case(9, 100, 16, af.AMINO, hanging=0.3), 8, 15, 4, 64, (1, 1, 0, 1))]
    for name, case, w, x, threads, max_ops, scoring in cases:
        header = np.array([case.num_reads, case.C, case.read_chars.size, case.num_read_chars, case.text.size, len(case.ends), w, x, case.alphabet,
                           6, threads, max_ops, *scoring], np.uint64)
        arrays = [header, case.read_chars, case.offsets] + [case.slots[f] for f in vc.SLOT_FIELDS] + [case.chosen, case.text, case.ends]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        want = case.host(awfm, w, x, scoring, max_ops, unaligned_before=6, truncated_before=7)
        n, at, got = case.num_reads, 0, {}
        for field, dtype, count in [(f, d, n) for f, d in af.READ_OUTPUTS.items()] + [("ops", np.uint32, n * max_ops), ("numUnaligned", np.uint64, 1),
                                                                                      ("numTruncated", np.uint64, 1)]:
            got[field] = np.frombuffer(run.stdout, dtype, count, at)
            at += count * np.dtype(dtype).itemsize
        got["ops"] = got["ops"].reshape(n, max_ops)
        got["numUnaligned"], got["numTruncated"] = int(got["numUnaligned"][0]), int(got["numTruncated"][0])
        af.assert_equal(got, want, what=name)
