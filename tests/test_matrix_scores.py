"""awfmScoreChainsMatrix, awfmAlignChainsMatrix, awfmMatrixScoringUniform and awfmMatrixScoringFromText (include/awfm_gpu.h
"substitution matrices"), the host twins and checkers of the device calls: against the plain-Python restatement of
tests/matrix_scores_common.py on hand-computed cases, the edge lists and random batches under matrices over the full int8 range
and over -4..11, by replaying every script under the restated invariants, against the affine calls under the uniform matrix,
against each other slot by slot, over all 256 byte values on either side, and the parser on hand-written texts, each refusal and
every prefix of a text.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import matrix_scores_common as mx  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402

NULL_POINTER, FORMAT = -4, -9  # AwFmNullPtrError, AwFmFileFormatError
ALIGN_OUTPUTS = list(af.READ_OUTPUTS) + ["ops"] + list(af.COUNTERS)


def test_hand_computed_cases_of_a_few_letters(awfm):
    for matrix, b in mx.hand_builders():
        case = b.case()
        got = case.host(awfm, 0, 0, matrix, max_ops=8, fill=0xC3)
        b.check(got, 8)
        af.assert_equal(got, case.expected(0, 0, matrix, max_ops=8), what=repr(matrix), fill=0xC3)
        mx.assert_scripts_replay(case, got, 0, 0, matrix, 8)
        scores = case.score(awfm, 0, 0, matrix)
        assert np.array_equal(scores["slotScores"][:, 0], got["scores"]), matrix
    # the script that begins and ends with X, and its edit distance
    matrix, b = mx.hand_builders()[1]
    got = b.case().host(awfm, 0, 0, matrix)
    assert af.cigar(af.runs_of(got["ops"][0], int(got["numOps"][0]))) == "1X2=1X" and int(got["editDistances"][0]) == 2


@pytest.mark.parametrize("w,x", [(2, 3), (8, 15), (3, 4), (24, 15)])
def test_edge_lists_under_the_uniform_and_the_adversarial_matrices(awfm, w, x):
    b = af.edge_builder(w, x)
    case = mx.as_matrix(b.case())
    got = case.host(awfm, w, x, mx.uniform(af.DNA, af.DEFAULT), max_ops=8, unaligned_before=9, truncated_before=2, fill=0xC3)
    b.check(got, 8)  # the hand-computed values of affine alignment
    assert got["numUnaligned"] == 9 + b.unaligned() and got["numTruncated"] == 2
    for matrix in mx.ADVERSARIAL + (mx.random_matrix(w, -128, 127),):
        got = case.host(awfm, w, x, matrix, max_ops=8, fill=0xC3)
        af.assert_equal(got, case.expected(w, x, matrix, max_ops=8), what=repr(matrix), fill=0xC3)
        mx.assert_scripts_replay(case, got, w, x, matrix, 8, unbanded_every=3)
        for skew in (1, 2, 3):
            af.assert_equal(mx.as_matrix(b.case(skew)).host(awfm, w, x, matrix, max_ops=8), got, what=f"skew {skew}")
    outside = mx.as_matrix(af.outside_builder().case())
    for matrix in mx.ADVERSARIAL:
        af.assert_equal(outside.host(awfm, 0, 0, matrix, max_ops=8), outside.expected(0, 0, matrix, max_ops=8), what=repr(matrix))


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
@pytest.mark.parametrize("low,high", [(-128, 127), (-4, 11)], ids=["int8", "-4..11"])
def test_1024_random_reads_equal_the_restatement_and_replay(awfm, alphabet, low, high):
    """16 diagonals; some slots unused, some malformed, some whose band hangs over a record end"""
    w, x, max_ops = 7, 1, 48  # (a read has 46 characters at the most: no script is truncated, every one is replayed)
    case = mx.random_case(77, 1 << 10, 2, alphabet, max_length=40, broken=0.05, hanging=0.2)
    matrix = mx.random_matrix(5, low, high, 11 if alphabet == af.AMINO else 6, 1)
    want = case.expected(w, x, matrix, max_ops, unaligned_before=5, truncated_before=7)
    got = case.host(awfm, w, x, matrix, max_ops, unaligned_before=5, truncated_before=7, fill=0x5A, threads=3)
    af.assert_equal(got, want, what=repr(matrix), fill=0x5A)
    aligned = int(((want["scores"] > 0) & (want["scores"] < af.TOO_LONG)).sum())
    assert want["numTruncated"] == 7 and aligned > 512 and mx.assert_scripts_replay(case, got, w, x, matrix, max_ops, unbanded_every=16) == aligned
    short = case.host(awfm, w, x, matrix, 3, truncated_before=7, fill=0x5A, threads=3)  # most scripts have more than three runs
    af.assert_equal(short, case.expected(w, x, matrix, 3, truncated_before=7), what="three runs", fill=0x5A)
    assert short["numTruncated"] > 7 + aligned // 2
    scores = case.score(awfm, w, x, matrix, min_score=3, cap=254, unscored_before=2, mapped_before=1, fill=0x5A, threads=3)
    sc.assert_equal(scores, case.expected_scores(w, x, matrix, min_score=3, cap=254, unscored_before=2, mapped_before=1), what=repr(matrix))


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_the_uniform_matrix_gives_what_the_affine_calls_give(awfm, alphabet):
    batch = mx.random_case(31, 400, 4, alphabet, max_length=80, hanging=0.2)
    edges = [(mx.as_matrix(af.edge_builder(w, x).case()), w, x) for w, x in ((2, 3), (8, 15))] + [(mx.as_matrix(af.outside_builder().case()), 0, 0)]
    accepted = 0
    for scoring in af.SCORINGS:
        if scoring[0] > 127 or scoring[1] > 128:
            with pytest.raises(awfm.AwFmError) as e:
                awfm.matrix_scoring_uniform(alphabet, scoring)
            assert e.value.rc == awfm.AwFmIllegalPositionError
            continue
        accepted += 1
        made = awfm.matrix_scoring_uniform(alphabet, scoring)
        want = mx.uniform(alphabet, scoring)
        assert np.array_equal(awfm.matrix_values(made), want.values) and (made.gapOpen, made.gapExtend) == scoring[2:]
        for case, w, x in [(batch, 8, 15)] + (edges if alphabet == af.DNA else []):
            affine = case.affine()
            af.assert_equal(case.host(awfm, w, x, want, max_ops=16, fill=0x5A), affine.host(awfm, w, x, scoring, max_ops=16, fill=0x5A),
                            names=ALIGN_OUTPUTS, what=str(scoring), fill=0x5A)
            sc.assert_equal(case.score(awfm, w, x, want, min_score=2, cap=60), affine.score(awfm, w, x, scoring, min_score=2, cap=60),
                            names=sc.ALL_OUTPUTS, what=str(scoring))
    assert accepted == 4 and (255, 255, 255, 255) in af.SCORINGS
    for scoring in ((128, 4, 6, 1), (1, 129, 6, 1), (0, 4, 6, 1), (1, 4, 256, 1), (1, 4, 6, 0)):
        with pytest.raises(awfm.AwFmError) as e:
            awfm.matrix_scoring_uniform(alphabet, scoring)
        assert e.value.rc == awfm.AwFmIllegalPositionError, scoring
    assert awfm.matrix_values(awfm.matrix_scoring_uniform(alphabet, (127, 128, 255, 255))).min() == -128
    lib = awfm._lib.lib()
    assert lib.awfmMatrixScoringUniform(alphabet, None, awfm._lib.AwFmMatrixScoring()) == NULL_POINTER
    assert lib.awfmMatrixScoringUniform(alphabet, awfm.align_scoring(), None) == NULL_POINTER
    assert lib.awfmMatrixScoringUniform(7, awfm.align_scoring(), awfm._lib.AwFmMatrixScoring()) == awfm.AwFmIllegalPositionError


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_the_score_of_a_slot_is_what_the_alignment_of_that_slot_gives(awfm, alphabet):
    case = mx.random_case(53, 300, 4, alphabet, max_length=90, hanging=0.2)
    for matrix, (w, x) in zip((mx.random_matrix(9, -128, 127), mx.random_matrix(10, -4, 11, 11, 1), mx.TRANSITIONS), ((8, 15), (2, 3), (20, 23))):
        got = case.score(awfm, w, x, matrix)
        sc.assert_equal(got, case.by_the_affine_call(awfm, w, x, matrix), names=list(sc.SLOT_OUTPUTS), what=repr(matrix))
        assert ((got["slotScores"] > 0) & (got["slotScores"] < af.TOO_LONG)).sum() > 100


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_all_256_byte_values_on_either_side_fall_into_the_classes_the_header_states(awfm, alphabet):
    case, x, y = mx.byte_pairs_case(alphabet)
    classes = mx.classes_of_all_bytes(alphabet)
    other = mx.other_class(alphabet)
    assert sorted(set(classes)) == list(range(other + 1)) and classes[ord("$")] == other and classes[0] == other
    by_row, by_column = mx.telling_matrices()
    for matrix, want in ((by_row, 1 + classes[x]), (by_column, 1 + classes[y])):
        got = case.host(awfm, 0, 0, matrix, max_ops=2, threads=4)
        assert np.array_equal(got["scores"], want), matrix
        assert np.array_equal(got["textEnds"], y + 1) and (got["readEnds"] == 1).all() and (got["numOps"] == 1).all()
        proper = (classes[x] == classes[y]) & (classes[x] < other)
        assert np.array_equal(got["ops"][:, 0], np.where(proper, 1 << 4 | af.OP_EQ, 1 << 4 | af.OP_X))  # '=' by identity alone
        assert np.array_equal(case.score(awfm, 0, 0, matrix, threads=4)["slotScores"][:, 0], want), matrix


AMINO_ORDER = "ARNDCQEGHILKMFPSTWYV"  # a customary order of the columns, not the library's


def amino_text(with_x, rng):
    """a hand-made amino matrix text and the 21 x 21 values it must give"""
    letters = AMINO_ORDER + "BZ" + ("X" if with_x else "") + "*"
    table = rng.integers(-9, 12, (len(letters), len(letters)))
    lines = ["# a hand-made matrix", "#", "", "   " + "  ".join(letters)]
    for a, row in zip(letters, table):
        lines.append(a + " " + " ".join(f"{int(v):3d}" for v in row))
    want = np.zeros((21, 21), np.int64)
    proper = [letters.index(c.upper()) for c in vc.AMINO_LETTERS]
    for a in range(20):
        for b in range(20):
            want[a, b] = table[proper[a], proper[b]]
    smallest = want[:20, :20].min()
    want[20, :], want[:, 20] = smallest, smallest
    if with_x:
        at = letters.index("X")
        for a in range(20):
            want[a, 20], want[20, a] = table[proper[a], at], table[at, proper[a]]
        want[20, 20] = table[at, at]
    return "\n".join(lines) + "\n", want


def nucleotide_text(with_n):
    lines = ["# transitions cost less", " a  C g\tT" + ("  N" if with_n else "") + "  R", "A  5 -4 -1 -4" + (" -2" if with_n else "") + " 9",
             "c -4  5 -4 -1" + ("  0" if with_n else "") + " 9", "", "G -1 -4  5 -4" + (" -2" if with_n else "") + " 9",
             "u -3 -1 -4 +5" + (" -2" if with_n else "") + " 9"] + (["N -2 -2 -2 -2  1 9"] if with_n else []) + ["R 9 9 9 9 " + ("9 " if with_n else "") + "9"]
    want = np.zeros((21, 21), np.int64)
    want[:4, :4] = [[5, -4, -1, -4], [-4, 5, -4, -1], [-1, -4, 5, -4], [-3, -1, -4, 5]]
    want[4, :5], want[:5, 4] = -4, -4
    if with_n:
        want[:4, 4], want[4, :4], want[4, 4] = [-2, 0, -2, -2], -2, 1
    return "\r\n".join(lines), want  # CR LF, and no newline at the end


def test_the_parser_reads_hand_written_texts_with_and_without_the_other_class(awfm):
    for with_x in (True, False):
        text, want = amino_text(with_x, np.random.default_rng(3))
        made = awfm.matrix_scoring_from_text(text, awfm.AwFmAlphabetAmino, 11, 1)
        assert np.array_equal(awfm.matrix_values(made), want) and (made.gapOpen, made.gapExtend) == (11, 1), with_x
        assert np.array_equal(awfm.matrix_values(awfm.matrix_scoring_from_text(text.lower().rstrip("\n"), awfm.AwFmAlphabetAmino)), want)
    for with_n in (True, False):
        text, want = nucleotide_text(with_n)
        for alphabet in (awfm.AwFmAlphabetDna, awfm.AwFmAlphabetRna):
            made = awfm.matrix_scoring_from_text(text, alphabet, 0, 255)
            assert np.array_equal(awfm.matrix_values(made), want) and (made.gapOpen, made.gapExtend) == (0, 255), with_n
    # what the parser gives scores like the same values put in by hand
    text, want = nucleotide_text(True)
    case = mx.random_case(3, 50, 1, af.DNA)
    parsed = case.host(awfm, 8, 15, mx.Matrix(awfm.matrix_values(awfm.matrix_scoring_from_text(text, awfm.AwFmAlphabetDna, 6, 1))))
    af.assert_equal(parsed, case.host(awfm, 8, 15, mx.Matrix(want)))


def test_the_parser_refuses_each_malformed_text_with_the_code_the_header_names(awfm):
    good = "a c g t\na 1 -1 -1 -1\nc -1 1 -1 -1\ng -1 -1 1 -1\nt -1 -1 -1 1\n"
    dna = awfm.AwFmAlphabetDna
    awfm.matrix_scoring_from_text(good, dna)
    refused = {
        "a proper letter missing as a column": ("a c g\na 1 -1 -1\nc -1 1 -1\ng -1 -1 1\nt -1 -1 -1\n", FORMAT),
        "a proper letter missing as a row": ("a c g t\na 1 -1 -1 -1\nc -1 1 -1 -1\ng -1 -1 1 -1\n", FORMAT),
        "a column repeated": ("a c g t a\n" + "".join(f"{c} 1 1 1 1 1\n" for c in "acgt"), FORMAT),
        "a column repeated in the other case, u for t": ("a c g t U\n" + "".join(f"{c} 1 1 1 1 1\n" for c in "acgt"), FORMAT),
        "a row repeated": (good + "A 1 1 1 1\n", FORMAT),
        "the other class repeated": ("a c g t n N\n" + "".join(f"{c} 1 1 1 1 1 1\n" for c in "acgtn"), FORMAT),
        "a row with a value too few": (good.replace("c -1 1 -1 -1", "c -1 1 -1"), FORMAT),
        "a row with a value too many": (good.replace("c -1 1 -1 -1", "c -1 1 -1 -1 0"), FORMAT),
        "a skipped row with a value too few": (good + "r 1 1 1\n", FORMAT),
        "a value that is no integer": (good.replace("g -1 -1 1 -1", "g -1 -1 1.5 -1"), FORMAT),
        "a bare sign": (good.replace("g -1 -1 1 -1", "g -1 - 1 -1"), FORMAT),
        "a row name of two characters": (good.replace("\ng ", "\ngg "), FORMAT),
        "a column name of two characters": (good.replace("a c g t\n", "a c gg t\n"), FORMAT),
        "a text that ends inside a row": (good[:-6], FORMAT),
        "only comments": ("# nothing\n\n   \n", FORMAT),
        "128": (good.replace("g -1 -1 1 -1", "g -1 -1 128 -1"), awfm.AwFmIllegalPositionError),
        "-129": (good.replace("g -1 -1 1 -1", "g -129 -1 1 -1"), awfm.AwFmIllegalPositionError),
        "a value beyond 32 bits": (good.replace("g -1 -1 1 -1", "g -1 -1 99999999999999999999 -1"), awfm.AwFmIllegalPositionError),
        "a value out of range in a skipped row": (good + "r 1 1 1 300\n", awfm.AwFmIllegalPositionError),
    }
    for what, (text, code) in refused.items():
        with pytest.raises(awfm.AwFmError) as e:
            awfm.matrix_scoring_from_text(text, dna)
        assert e.value.rc == code, what
    assert awfm.matrix_values(awfm.matrix_scoring_from_text(good.replace("t -1 -1 -1 1", "t -128 127 +0 -0"), dna))[3, :4].tolist() == [-128, 127, 0, 0]
    for kw in (dict(gap_open=256), dict(gap_extend=0), dict(gap_extend=256), dict(alphabet=0)):
        with pytest.raises(awfm.AwFmError) as e:
            awfm.matrix_scoring_from_text(good, **dict(dict(alphabet=dna), **kw))
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    lib, out = awfm._lib.lib(), awfm._lib.AwFmMatrixScoring()
    assert lib.awfmMatrixScoringFromText(dna, None, 5, 6, 1, out) == NULL_POINTER and lib.awfmMatrixScoringFromText(dna, None, 0, 6, 1, out) == FORMAT
    block = np.frombuffer(good.encode(), np.uint8)
    assert lib.awfmMatrixScoringFromText(dna, block.ctypes.data, block.size, 6, 1, None) == NULL_POINTER
    # a refusal leaves *out as it was
    out.substitution[0], out.gapOpen = 77, 5
    assert lib.awfmMatrixScoringFromText(dna, block.ctypes.data, block.size - 6, 6, 1, out) == FORMAT and (out.substitution[0], out.gapOpen) == (77, 5)


def test_every_prefix_of_a_text_gives_a_refusal_or_a_result(awfm):
    text, want = nucleotide_text(True)
    results = 0
    for size in range(len(text) + 1):
        try:
            made = awfm.matrix_scoring_from_text(text, awfm.AwFmAlphabetDna, num_bytes=size)
        except awfm.AwFmError as e:
            assert e.rc in (FORMAT, awfm.AwFmIllegalPositionError), size
            continue
        results += 1
        assert np.array_equal(awfm.matrix_values(made)[:4, :4], want[:4, :4]), size  # (the rows behind t are optional)
    assert 1 <= results < 40 and np.array_equal(awfm.matrix_values(made), want)


def test_argument_checks_in_affine_alignments_order_and_a_null_matrix(awfm):
    case = mx.as_matrix(af.edge_builder(2, 3).case())
    matrix = mx.uniform(af.DNA, af.DEFAULT)
    for kw in (dict(w=32, x=0), dict(w=0, x=64), dict(w=31, x=2), dict(w=2 ** 31, x=2 ** 31), dict(w=2, x=3, max_ops=0), dict(w=2, x=3, max_ops=af.MAX_OPS + 1)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, scoring=matrix, **kw)
        assert e.value.rc == awfm.AwFmIllegalPositionError, kw
    with pytest.raises(awfm.AwFmError) as e:
        case.score(awfm, 2, 3, matrix, cap=255)
    assert e.value.rc == awfm.AwFmIllegalPositionError
    for o, e_ in ((0, 1), (255, 255)):  # the bounds themselves
        case.host(awfm, 2, 3, mx.Matrix(matrix.values, o, e_))
        case.score(awfm, 2, 3, mx.Matrix(matrix.values, o, e_))
    for o, e_ in ((256, 1), (6, 0), (6, 256), (2 ** 32 - 1, 2 ** 32 - 1)):
        for call in (case.host, case.score):
            with pytest.raises(awfm.AwFmError) as e:
                call(awfm, 2, 3, mx.Matrix(matrix.values, o, e_))
            assert e.value.rc == awfm.AwFmIllegalPositionError, (o, e_)
    lib, costs = awfm._lib.lib(), matrix.struct(awfm)
    empty = awfm.verify_inputs(0, 0, 0)
    assert lib.awfmAlignChainsMatrix(empty, None, 0, 4, 2, 3, None, 8, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess  # no reads: nothing touched
    assert lib.awfmScoreChainsMatrix(empty, 0, 4, 2, 3, None, 0, 60, None, 0, None, 0, af.DNA, None, 1) == awfm.AwFmSuccess
    assert lib.awfmAlignChainsMatrix(empty, None, 1, 4, 2, 3, costs, 8, None, 0, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER
    slots = {name: np.zeros((1, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    vin = awfm.verify_inputs(case.read_chars.ctypes.data, 4, case.offsets.ctypes.data, **{n: a.ctypes.data for n, a in slots.items()})
    text, chosen = (case.text.ctypes.data, case.text.size), case.chosen.ctypes.data
    assert lib.awfmAlignChainsMatrix(vin, None, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER  # no slots
    assert lib.awfmAlignChainsMatrix(vin, chosen, 1, 1, 2, 3, None, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER  # no matrix
    assert lib.awfmAlignChainsMatrix(vin, chosen, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, None, 1) == NULL_POINTER  # no outputs
    assert lib.awfmAlignChainsMatrix(vin, chosen, 1, 1, 2, 3, costs, 8, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == awfm.AwFmSuccess
    assert lib.awfmScoreChainsMatrix(vin, 1, 1, 2, 3, None, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == NULL_POINTER  # no matrix
    assert lib.awfmScoreChainsMatrix(vin, 1, 1, 2, 3, costs, 0, 60, *text, None, 0, af.DNA, None, 1) == NULL_POINTER  # no outputs
    assert lib.awfmScoreChainsMatrix(vin, 1, 1, 2, 3, costs, 0, 60, *text, None, 0, af.DNA, awfm.slot_score_outputs(), 1) == awfm.AwFmSuccess
    bad = mx.Matrix(matrix.values, 256, 1).struct(awfm)
    # a null comes before a slot count out of range, that before maxOps, that before the gap costs: affine alignment's order
    assert lib.awfmAlignChainsMatrix(vin, None, 1, 17, 2, 3, bad, 0, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == NULL_POINTER
    for C, max_ops, costs_ in ((17, 0, bad), (1, 0, bad), (1, 8, bad)):
        assert lib.awfmAlignChainsMatrix(vin, chosen, 1, C, 2, 3, costs_, max_ops, *text, None, 0, af.DNA, awfm.affine_outputs(), 1) == awfm.AwFmIllegalPositionError
