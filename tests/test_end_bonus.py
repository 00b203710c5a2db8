"""awfmScoreChainsEndBonus and awfmAlignChainsEndBonus (include/awfm_gpu.h "end bonus"), the host twins and checkers of the device
calls: against the plain-Python restatement of tests/end_bonus_common.py on the hand table and its mirror image, the rule "a
substitution k characters from a read end is kept exactly when k match + B > mismatch", reads of 0 and 1 characters, inserted
first and last characters, bands without a cell in row 0 or row n, the edge lists and random batches of both alphabets at every
band shape under the adversarial and the uniform matrices with B = 0, 1, 5, 7, 255, by replaying every script under the restated
invariants, against the matrix calls at B = 0, against each other slot by slot, the per-read rules on V, an unbanded Gotoh pass
under the same B, and every refusal.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import end_bonus_common as eb  # noqa: E402
import matrix_scores_common as mx  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402

NULL_POINTER = -4  # AwFmNullPtrError
ALIGN_OUTPUTS = list(af.READ_OUTPUTS) + ["ops"] + list(af.COUNTERS)
DNA_MATRICES = mx.ADVERSARIAL + tuple(mx.uniform(af.DNA, s) for s in eb.UNIFORM_SCORINGS)
AMINO_MATRICES = (mx.random_matrix(5, -4, 11, 11, 1), mx.random_matrix(6, -128, 127, 11, 1)) + tuple(mx.uniform(af.AMINO, s) for s in eb.UNIFORM_SCORINGS)
WIDTHS = sorted(af.BAND_SHAPES)


def cigars(got):
    return [af.cigar(af.runs_of(got["ops"][r], int(got["numOps"][r]))) for r in range(len(got["numOps"]))]


def test_the_hand_table_and_its_mirror_image_at_the_reads_start(awfm):
    for scoring, b in eb.hand_builders():
        case = b.case()
        got = case.host(awfm, 2, 0, scoring, max_ops=8, fill=0xC3)
        b.check(got, 8)
        af.assert_equal(got, case.expected(2, 0, scoring, max_ops=8), what=repr(scoring), fill=0xC3)
        assert eb.assert_scripts_replay(case, got, 2, 0, scoring, 8) == 2
        assert np.array_equal(case.score(awfm, 2, 0, scoring)["slotScores"][:, 0], got["scores"]), scoring
    # the tie between a clipped and an unclipped end goes to the clip, at both ends: k = 1, B = 3
    scoring, b = eb.hand_builders()[2]
    got = b.case().host(awfm, 2, 0, scoring)
    assert cigars(got) == ["10=2S", "2S10="] and got["scores"].tolist() == [13, 13] and got["editDistances"].tolist() == [0, 0]
    # and one more of B keeps the substitution: 10 + B - 4 + 1 + B = 15 against 10 + B = 14
    got = b.case().host(awfm, 2, 0, eb.uniform((1, 4, 6, 1), 4))
    assert cigars(got) == ["10=1X1=", "1=1X10="] and got["scores"].tolist() == [15, 15] and got["editDistances"].tolist() == [1, 1]
    # a read whose first character mismatches: 1X first
    scoring, b = eb.hand_builders()[0]
    assert cigars(b.case().host(awfm, 2, 0, scoring))[1] == "1X11="


@pytest.mark.parametrize("left", [False, True], ids=["end", "start"])
def test_a_substitution_k_from_a_read_end_is_kept_exactly_when_k_match_plus_bonus_exceeds_mismatch(awfm, left):
    ma, mm = 1, 4
    seen = set()
    for B in eb.BONUSES:
        scoring = eb.uniform((ma, mm, 6, 1), B)
        for k in range(7):
            case = eb.kept_builder(scoring, k, left).case()
            got = case.host(awfm, 2, 0, scoring, max_ops=8)
            af.assert_equal(got, case.expected(2, 0, scoring, max_ops=8), what=f"k={k} B={B}")
            n, kept = 30, k * ma + B > mm
            seen.add(kept)
            assert int(got["editDistances"][0]) == kept and (int(got["readBegins"][0]) == 0 if left else int(got["readEnds"][0]) == n) == kept, (k, B)
            clipped_score = n - 1 - k + B  # the other end is reached
            assert int(got["scores"][0]) == (n - 1 - mm + 2 * B if kept else clipped_score), (k, B, cigars(got))
    assert seen == {False, True}


def test_reads_of_no_and_of_one_character(awfm):
    """n = 1: row 1 is row n, both bonuses on one cell"""
    for B in eb.BONUSES:
        scoring = eb.uniform((1, 4, 6, 1), B)
        b = eb.Builder([b"ACGT", eb.FILLER])
        b.add("n = 0", b"", 0, 1, 1, af.NOTHING)
        b.add("n = 1 equal", b"C", 0, 1, 1, (1 + 2 * B, 0, 1, 1, 2, "1="))
        # B - 4 > 0: an X between two read ends, in the first cell of row 1 that the band holds, (1, 1)
        b.add("n = 1 different", b"n", 0, 1, 1, (2 * B - 4, 0, 1, 0, 1, "1X") if B > 4 else af.NOTHING)
        case = b.case()
        got = case.host(awfm, 1, 0, scoring, max_ops=4, fill=0xC3)
        b.check(got, 4)
        af.assert_equal(got, case.expected(1, 0, scoring, max_ops=4), what=repr(scoring), fill=0xC3)
        eb.assert_scripts_replay(case, got, 1, 0, scoring, 4)


def test_an_inserted_first_and_last_character_next_to_unclipped_ends_when_the_bonus_exceeds_a_gap(awfm):
    """the read hangs one character over either end of its record: cell (1, 0) has no diagonal, its F opens from row 0 at B - o - e"""
    record = b"GATCCTGAAGTCATGCTTGA"
    b = eb.Builder([record, eb.FILLER])
    b.add("one character over either end", b"n" + record + b"n", 0, -1, -1, None, rb=1, re=21)
    case = b.case()
    for B, want in ((7, (20, 1, 21, 0, 20, "1S20=1S")), (8, (22, 0, 22, 0, 20, "1I20=1I")), (255, (516, 0, 22, 0, 20, "1I20=1I"))):
        scoring = eb.uniform((1, 4, 6, 1), B)
        got = case.host(awfm, 2, 0, scoring, max_ops=4)
        have = tuple(int(got[f][0]) for f in ("scores", "readBegins", "readEnds", "textBegins", "textEnds")) + (cigars(got)[0],)
        assert have == want, (B, have)
        af.assert_equal(got, case.expected(2, 0, scoring, max_ops=4), what=repr(scoring))
        assert eb.assert_scripts_replay(case, got, 2, 0, scoring, 4) == 1


def test_bands_without_a_cell_in_row_n_or_in_row_0(awfm):
    """w = 0: a band that leaves the record after 8 rows has no cell in row n, so nothing earns the right bonus; one that enters it
    after 4 rows has none in row 0, so nothing earns the left one"""
    b = af.outside_builder()
    case = eb.as_bonus(b.case())
    L = len(af.R2)
    for B in eb.BONUSES:
        scoring = eb.uniform((1, 4, 6, 1), B)
        got = case.host(awfm, 0, 0, scoring, max_ops=4)
        af.assert_equal(got, case.expected(0, 0, scoring, max_ops=4), what=repr(scoring))
        eb.assert_scripts_replay(case, got, 0, 0, scoring, 4)
        # row 0 has the cell (0, L - 8): the left end is reached, the right one cannot be; and the mirror image
        assert (int(got["scores"][2]), cigars(got)[2]) == (8 + B, "8=4S") and (int(got["scores"][3]), cigars(got)[3]) == (8 + B, "4S8=")
        assert int(got["textEnds"][2]) == L and int(got["scores"][0]) == 0 and int(got["scores"][1]) == 0


@pytest.mark.parametrize("w,x", [(2, 3), (8, 15), (3, 4), (24, 15)])
def test_edge_lists_with_bands_hanging_over_either_record_end(awfm, w, x):
    """af.edge_builder's list (bands hanging 1, w - 1, w and w + 1 characters over either record end among them) under every B"""
    b = af.edge_builder(w, x)
    case = eb.as_bonus(b.case())
    got = case.host(awfm, w, x, eb.uniform(af.DEFAULT, 0), max_ops=8, unaligned_before=9, truncated_before=2, fill=0xC3)
    b.check(got, 8)  # B = 0: the hand-computed values of affine alignment
    assert got["numUnaligned"] == 9 + b.unaligned() and got["numTruncated"] == 2
    for k, B in enumerate(eb.BONUSES):
        for matrix in (DNA_MATRICES[5], DNA_MATRICES[(k + w) % 5]):
            scoring = eb.Scoring(matrix, B)
            got = case.host(awfm, w, x, scoring, max_ops=8, fill=0xC3)
            af.assert_equal(got, case.expected(w, x, scoring, max_ops=8), what=repr(scoring), fill=0xC3)
            eb.assert_scripts_replay(case, got, w, x, scoring, 8)
            sc.assert_equal(case.score(awfm, w, x, scoring), case.by_the_affine_call(awfm, w, x, scoring), names=list(sc.SLOT_OUTPUTS), what=repr(scoring))
            for skew in (1, 2, 3):
                af.assert_equal(eb.as_bonus(b.case(skew)).host(awfm, w, x, scoring, max_ops=8), got, what=f"skew {skew}")


def corpus_case(alphabet, width, C):
    reads = {1: 40, 4: 20, 16: 8}[C]
    return eb.random_case(1000 + width, reads, C, alphabet, text_length=2048, max_length=36, broken=0.05, hanging=0.25)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_random_reads_equal_the_restatement_replay_and_equal_the_matrix_calls_without_a_bonus(awfm, alphabet, width):
    """both alphabets, C = 1, 4, 16, every band shape, every matrix with every B: the band shapes carry the cross product"""
    w, x = af.BAND_SHAPES[width]
    matrices = DNA_MATRICES if alphabet == af.DNA else AMINO_MATRICES
    at = WIDTHS.index(width)
    max_ops, replayed = 48, 0
    for k, B in enumerate(eb.BONUSES):
        C = (1, 4, 16)[(at + k) % 3]
        case = corpus_case(alphabet, width, C)
        for matrix in (matrices[(at + k) % len(matrices)], matrices[(at + 2 * k + 3) % len(matrices)]):
            scoring = eb.Scoring(matrix, B)
            got = case.host(awfm, w, x, scoring, max_ops, unaligned_before=5, truncated_before=7, fill=0x5A, threads=3)
            af.assert_equal(got, case.expected(w, x, scoring, max_ops, unaligned_before=5, truncated_before=7), what=repr(scoring), fill=0x5A)
            assert got["numTruncated"] == 7
            replayed += eb.assert_scripts_replay(case, got, w, x, scoring, max_ops)
            scores = case.score(awfm, w, x, scoring, min_score=3, cap=254, unscored_before=2, mapped_before=1, fill=0x5A, threads=3)
            sc.assert_equal(scores, case.expected_scores(w, x, scoring, min_score=3, cap=254, unscored_before=2, mapped_before=1), what=repr(scoring))
            sc.assert_equal(scores, case.by_the_affine_call(awfm, w, x, scoring), names=list(sc.SLOT_OUTPUTS), what=repr(scoring))
            if B == 0:
                plain = case.matrix_case()
                af.assert_equal(got, plain.host(awfm, w, x, matrix, max_ops, unaligned_before=5, truncated_before=7, fill=0x5A), names=ALIGN_OUTPUTS,
                                what=repr(matrix), fill=0x5A)
                sc.assert_equal(scores, plain.score(awfm, w, x, matrix, min_score=3, cap=254, unscored_before=2, mapped_before=1), names=sc.ALL_OUTPUTS,
                                what=repr(matrix))
            short = case.host(awfm, w, x, scoring, 2, fill=0x5A)  # truncated reads: everything but their rows of ops
            af.assert_equal(short, case.expected(w, x, scoring, 2), what="two runs", fill=0x5A)
    assert replayed >= 40


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_no_bonus_gives_what_the_matrix_calls_give_on_a_larger_batch(awfm, alphabet):
    case = eb.random_case(31, 400, 4, alphabet, max_length=80, hanging=0.2)
    plain = case.matrix_case()
    for matrix, (w, x) in zip((DNA_MATRICES if alphabet == af.DNA else AMINO_MATRICES)[:4], ((8, 15), (2, 3), (20, 23), (31, 1))):
        scoring = eb.Scoring(matrix, 0)
        af.assert_equal(case.host(awfm, w, x, scoring, max_ops=16, fill=0x5A), plain.host(awfm, w, x, matrix, max_ops=16, fill=0x5A), names=ALIGN_OUTPUTS,
                        what=repr(matrix), fill=0x5A)
        sc.assert_equal(case.score(awfm, w, x, scoring, min_score=2), plain.score(awfm, w, x, matrix, min_score=2), names=sc.ALL_OUTPUTS, what=repr(matrix))


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_the_score_of_a_slot_is_what_the_alignment_of_that_slot_gives(awfm, alphabet):
    case = eb.random_case(53, 300, 4, alphabet, max_length=90, hanging=0.2)
    matrices = DNA_MATRICES if alphabet == af.DNA else AMINO_MATRICES
    for matrix, B, (w, x) in zip(matrices[:3], (5, 255, 1), ((8, 15), (2, 3), (20, 23))):
        scoring = eb.Scoring(matrix, B)
        got = case.score(awfm, w, x, scoring)
        sc.assert_equal(got, case.by_the_affine_call(awfm, w, x, scoring), names=list(sc.SLOT_OUTPUTS), what=repr(scoring))
        assert ((got["slotScores"] > 0) & (got["slotScores"] < af.TOO_LONG)).sum() > 100


def test_best_slot_second_slot_duplicates_and_mapping_quality_work_on_scores_with_the_bonus(awfm):
    """sc.rules_builder's list under B = 5: a slot on READ's own diagonal reaches both read ends, 100 + 10; the decoy holds 37
    characters of the read's middle and stays at 37"""
    b = sc.rules_builder(4)
    case = eb.as_bonus(b.case())
    plain, bonus = eb.uniform(af.DEFAULT, 0), eb.uniform(af.DEFAULT, 5)
    b.check(case.score(awfm, 8, 15, plain))  # the hand-computed values of the scoring call
    got = case.score(awfm, 8, 15, bonus)
    sc.assert_equal(got, case.expected_scores(8, 15, bonus))
    r = b.names.index("best 100, second 37")
    assert tuple(int(got[f][r]) for f in sc.READ_OUTPUTS) == (0, 110, 1, 37, 60 * 73 // 110) and got["slotScores"][r].tolist()[:2] == [110, 37]
    r = b.names.index("a duplicate: diagonals 10 and 12 of one sequence give one end cell")
    assert tuple(int(got[f][r]) for f in sc.READ_OUTPUTS) == (0, 110, sc.NO_SLOT, 0, 60)
    # minScore is held against V: 105 lets the read through with the bonus only
    r = b.names.index("one slot: second is 0 and mapq = cap")
    assert int(case.score(awfm, 8, 15, plain, min_score=105)["bestSlots"][r]) == sc.NO_SLOT
    with_floor = case.score(awfm, 8, 15, bonus, min_score=105)
    sc.assert_equal(with_floor, case.expected_scores(8, 15, bonus, min_score=105))
    assert int(with_floor["bestSlots"][r]) == 0 and int(with_floor["bestScores"][r]) == 110


def test_300_planted_reads_against_an_unbanded_pass_under_the_same_bonus(awfm):
    """30..150 characters, 3 % substitutions, at most 4 indel characters, w = 8: never above the unbanded value, and equal to it
    whenever the unbanded path lies inside the band -- which, under this seed, it does for all 300 under every B"""
    w = 8
    case = eb.planted_case(11, 300, w)
    for B in (0, 5, 255):
        scoring = eb.uniform(af.DEFAULT, B)
        got = case.host(awfm, w, 15, scoring, max_ops=32, threads=4)
        inside = 0
        for r in range(case.num_reads):
            S, E, lo, hi = case.status(r, w, 15)
            R, T = case.read(r), bytes(case.text[S:E])
            score, lowest, highest = eb.unbanded(R, T, scoring)
            assert int(got["scores"][r]) <= score, (B, r)
            if lowest is not None and lo <= lowest and highest <= hi:
                inside += 1
                assert int(got["scores"][r]) == score, (B, r)
        assert inside == 300, (B, inside)
        assert eb.assert_scripts_replay(case, got, w, 15, scoring, 32) == 300
    # the restatement itself agrees with the unbanded pass when its band is the whole matrix
    for r in range(0, 300, 37):
        S, E, _, _ = case.status(r, w, 15)
        R, T = case.read(r), bytes(case.text[S:E])
        assert eb.local(R, T, -len(R), len(T), eb.uniform(af.DEFAULT, 5))[0] == eb.unbanded(R, T, eb.uniform(af.DEFAULT, 5))[0], r


def test_every_output_null_in_turn_and_alone(awfm):
    case = eb.as_bonus(af.edge_builder(2, 3).case())
    scoring = eb.Scoring(mx.TRANSITIONS, 5)
    want, want_scores = case.host(awfm, 2, 3, scoring, max_ops=8), case.score(awfm, 2, 3, scoring)
    for names, call, equal, wanted in ((ALIGN_OUTPUTS, lambda o: case.host(awfm, 2, 3, scoring, max_ops=8, outputs=o), af.assert_equal, want),
                                       (sc.ALL_OUTPUTS, lambda o: case.score(awfm, 2, 3, scoring, outputs=o), sc.assert_equal, want_scores)):
        for missing in names:
            for outputs in ([n for n in names if n != missing], [missing]):
                got = call(outputs)
                assert sorted(got) == sorted(outputs)
                if "ops" in outputs and "numOps" not in outputs:
                    got = dict(got, numOps=want["numOps"])
                equal(got, wanted, names=outputs, what=str(outputs))


def test_a_bonus_of_256_is_refused_and_so_is_everything_the_matrix_calls_refuse(awfm):
    case = eb.as_bonus(af.edge_builder(2, 3).case())
    matrix = mx.uniform(af.DNA, af.DEFAULT)
    case.host(awfm, 2, 3, eb.Scoring(matrix, 255))  # the bound itself
    case.score(awfm, 2, 3, eb.Scoring(matrix, 255))
    for B in (256, 2 ** 32 - 1):
        for call in (case.host, case.score):
            with pytest.raises(awfm.AwFmError) as e:
                call(awfm, 2, 3, eb.Scoring(matrix, B))
            assert e.value.rc == awfm.AwFmIllegalPositionError, B
    for kw in (dict(w=32, x=0), dict(w=0, x=64), dict(w=31, x=2), dict(w=2 ** 31, x=2 ** 31), dict(w=2, x=3, max_ops=0), dict(w=2, x=3, max_ops=af.MAX_OPS + 1)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, scoring=eb.Scoring(matrix, 5), **kw)
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    with pytest.raises(awfm.AwFmError) as e:
        case.score(awfm, 2, 3, eb.Scoring(matrix, 5), cap=255)
    assert e.value.rc == awfm.AwFmIllegalPositionError
    for o, e_ in ((0, 1), (255, 255)):  # the bounds themselves
        case.host(awfm, 2, 3, eb.Scoring(mx.Matrix(matrix.values, o, e_), 5))
        case.score(awfm, 2, 3, eb.Scoring(mx.Matrix(matrix.values, o, e_), 5))
    for o, e_ in ((256, 1), (6, 0), (6, 256), (2 ** 32 - 1, 2 ** 32 - 1)):
        for call in (case.host, case.score):
            with pytest.raises(awfm.AwFmError) as e:
                call(awfm, 2, 3, eb.Scoring(mx.Matrix(matrix.values, o, e_), 5))
            assert e.value.rc == awfm.AwFmIllegalPositionError, (o, e_)
    lib, costs = awfm._lib.lib(), matrix.struct(awfm)
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmAlignChainsEndBonus(empty, None, 0, 4, 2, 3, None, 256, 8, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmScoreChainsEndBonus(empty, 0, 4, 2, 3, None, 256, 0, 60, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess
    assert lib.awfmAlignChainsEndBonus(empty, None, 1, 4, 2, 3, costs, 5, 8, None, 0, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER
    slots = {name: np.zeros((1, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
    text, chosen = (case.text.ctypes.data, case.text.size), case.chosen.ctypes.data
    assert lib.awfmAlignChainsEndBonus(vin, None, 1, 1, 2, 3, costs, 5, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER  # no slots
    assert lib.awfmAlignChainsEndBonus(vin, chosen, 1, 1, 2, 3, None, 5, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER  # no matrix
    assert lib.awfmAlignChainsEndBonus(vin, chosen, 1, 1, 2, 3, costs, 5, 8, *text, None, 0, af.DNA, None, 1) == NULL_POINTER  # no outputs
    assert lib.awfmAlignChainsEndBonus(vin, chosen, 1, 1, 2, 3, costs, 5, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == awfm.AwFmSuccess
    assert lib.awfmScoreChainsEndBonus(vin, 1, 1, 2, 3, None, 5, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == NULL_POINTER  # no matrix
    assert lib.awfmScoreChainsEndBonus(vin, 1, 1, 2, 3, costs, 5, 0, 60, *text, None, 0, af.DNA, None, 1) == NULL_POINTER  # no outputs
    assert lib.awfmScoreChainsEndBonus(vin, 1, 1, 2, 3, costs, 5, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == awfm.AwFmSuccess
    # a null comes before a slot count out of range, that before maxOps, that before the gap costs and the bonus: the siblings' order
    assert lib.awfmAlignChainsEndBonus(vin, None, 1, 17, 2, 3, costs, 256, 0, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER
    for C, max_ops, B in ((17, 0, 256), (1, 0, 256), (1, 8, 256)):
        assert lib.awfmAlignChainsEndBonus(vin, chosen, 1, C, 2, 3, costs, B, max_ops, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == awfm.AwFmIllegalPositionError
    assert lib.awfmScoreChainsEndBonus(vin, 1, 1, 2, 3, costs, 256, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == awfm.AwFmIllegalPositionError
