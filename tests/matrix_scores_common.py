"""Shared by the tests of the matrix twins (include/awfm_gpu.h, "substitution matrices"): awfmScoreChainsMatrix /
awfmAlignChainsMatrix and their device calls.  A plain-Python restatement of the definition -- tests/align_affine_common.py's
`local` with s(a, b) out of a 21 x 21 table and '=' / 'X' by identity --, an unbanded pass over the whole record, a replay that
re-scores a script from the text and checks the restated invariants, the matrices of the tests (uniform, full int8 range,
-4..11, two that tell a cell's row and column, and the hand-made adversarial ones) and hand-computed cases of a few letters.  Slots, texts and
batches are those of tests/align_chains_common.py; the per-read rules are tests/score_chains_common.py's."""
import numpy as np

import align_affine_common as af
import align_chains_common as ac
import score_chains_common as sc
import verify_chains_common as vc

DNA, AMINO = af.DNA, af.AMINO
CLASSES = 21
INF = af.INF
OP_I, OP_D, OP_S, OP_EQ, OP_X = af.OP_I, af.OP_D, af.OP_S, af.OP_EQ, af.OP_X


def other_class(alphabet):
    return 20 if alphabet == AMINO else 4


def class_of(alphabet, c):
    """the class of a byte as the header states it: the proper letter's index, everything else the last class"""
    x = vc.letter(alphabet, c)
    return other_class(alphabet) if x is None else x


class Matrix:
    """21 x 21 values [class of the read's character, class of the text's] and the gap costs"""

    def __init__(self, values, gap_open=6, gap_extend=1, name=""):
        self.values = np.array(values, np.int64).reshape(CLASSES, CLASSES)
        assert self.values.min() >= -128 and self.values.max() <= 127
        self.o, self.e, self.name = gap_open, gap_extend, name

    def s(self, alphabet, a, b):
        return int(self.values[class_of(alphabet, a), class_of(alphabet, b)])

    def struct(self, awfm):
        return awfm.matrix_scoring(self.values, self.o, self.e)

    def __repr__(self):
        return f"Matrix({self.name or 'unnamed'}, o={self.o}, e={self.e})"


def uniform(alphabet, scoring):
    """what awfmMatrixScoringUniform must give: + match where both classes are the same proper letter, - mismatch elsewhere"""
    ma, mm, o, e = scoring
    values = np.full((CLASSES, CLASSES), -mm, np.int64)
    for k in range(other_class(alphabet)):
        values[k, k] = ma
    return Matrix(values, o, e, f"uniform{scoring}")


def random_matrix(seed, low, high, gap_open=6, gap_extend=1):
    """every entry drawn from low .. high, the diagonal of the proper letters from the upper half so that alignments exist"""
    rng = np.random.default_rng(seed)
    values = rng.integers(low, high + 1, (CLASSES, CLASSES))
    for k in range(20):
        values[k, k] = rng.integers((low + high + 1) // 2, high + 1)
    return Matrix(values, gap_open, gap_extend, f"random[{low},{high}]#{seed}")


def telling_matrices():
    """An int8 has 256 values, so no matrix has 441 distinct entries; two matrices tell a cell's (row, column) between them: the
    first holds 1 + row everywhere, the second 1 + column, all positive so that a one-cell alignment scores exactly the entry"""
    rows = np.repeat(np.arange(1, CLASSES + 1), CLASSES).reshape(CLASSES, CLASSES)
    return Matrix(rows, 0, 1, "1 + class of the read's byte"), Matrix(rows.T, 0, 1, "1 + class of the text's byte")


def byte_pairs_case(alphabet):
    """65536 reads of one byte each, read 256 x + y holding byte x on the diagonal that puts it on byte y of a record of all 256
    byte values, under w = 0 and x = 0: the one cell (1, y + 1) pairs R[0] = x with T[y]"""
    x, y = np.divmod(np.arange(1 << 16), 256)
    slots = {name: np.zeros((1 << 16, 1), vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    slots["chainAnchors"][:] = 1
    slots["chainReadEnds"][:] = 1
    slots["chainBeginDiagonals"][:, 0] = slots["chainEndDiagonals"][:, 0] = y
    text = bytes(range(256)) + b"\0"
    return Case(x.astype(np.uint8).tobytes(), np.arange((1 << 16) + 1), slots, np.zeros(1 << 16, np.uint32), text, [256], alphabet), x, y


def classes_of_all_bytes(alphabet):
    return np.array([class_of(alphabet, c) for c in range(256)], np.int64)


def local(R, T, lo, hi, matrix, alphabet=DNA):
    """af.local with s from the matrix: (score, editDistance, readBegin, readEnd, textBegin, textEnd, [(run, op), ...])"""
    o, e = matrix.o, matrix.e
    n, L = len(R), len(T)
    H, E, F = {}, {}, {}

    def get(table, i, t):
        return table.get((i, t), -INF)

    def diagonal(i, t):
        return get(H, i - 1, t - 1) + (matrix.s(alphabet, R[i - 1], T[t - 1]) if t >= 1 else 0)

    best = (0, 0, 0)
    for i in range(n + 1):
        for t in range(max(0, i + lo), min(L, i + hi) + 1):
            if i == 0:
                H[i, t], E[i, t], F[i, t] = 0, -INF, -INF
                continue
            F[i, t] = max(get(H, i - 1, t) - o - e, get(F, i - 1, t) - e)
            E[i, t] = max(get(H, i, t - 1) - o - e, get(E, i, t - 1) - e)
            H[i, t] = max(0, diagonal(i, t), F[i, t], E[i, t])
            if H[i, t] > best[0]:
                best = (H[i, t], i, t)
    score, i, t = best
    if score == 0:
        return 0, 0, 0, 0, 0, 0, []
    read_end, text_end, state, script = i, t, "H", [OP_S] * (n - i)
    while True:
        if state == "H":
            if H[i, t] == 0:
                break
            if diagonal(i, t) == H[i, t]:
                script.append(OP_X if vc.sub(alphabet, R[i - 1], T[t - 1]) else OP_EQ)
                i, t = i - 1, t - 1
            elif F[i, t] == H[i, t]:
                state = "F"
            else:
                state = "E"
        elif state == "F":
            script.append(OP_I)
            state = "H" if get(H, i - 1, t) - o - e >= get(F, i - 1, t) - e else "F"
            i -= 1
        else:
            script.append(OP_D)
            state = "H" if get(H, i, t - 1) - o - e >= get(E, i, t - 1) - e else "E"
            t -= 1
    script += [OP_S] * i
    distance = sum(op in (OP_X, OP_I, OP_D) for op in script)
    return score, distance, i, read_end, t, text_end, af.merge(reversed(script))


def unbanded_score(R, T, matrix, alphabet=DNA):
    """the local score over the whole record, a row's E cell by cell as the recurrence is written"""
    o, e = matrix.o, matrix.e
    n, L = len(R), len(T)
    NEG = -(1 << 40)
    classes_t = np.array([class_of(alphabet, c) for c in T], np.int64)
    H, F, best = np.zeros(L + 1, np.int64), np.full(L + 1, NEG, np.int64), 0
    for i in range(1, n + 1):
        S = matrix.values[class_of(alphabet, R[i - 1])][classes_t] if L else np.zeros(0, np.int64)
        M = np.full(L + 1, NEG, np.int64)
        M[1:] = H[:-1] + S
        F = np.maximum(H - o - e, F - e)
        tilde = np.maximum(0, np.maximum(M, F))
        new, left = np.zeros(L + 1, np.int64), NEG
        for t in range(L + 1):
            if t:
                left = max(int(new[t - 1]) - o - e, left - e)
            new[t] = max(int(tilde[t]), left)
        H = new
        best = max(best, int(H.max()))
    return best


def replay(runs, R, T, text_begin, matrix, alphabet=DNA):
    """(read characters, text characters, score, X + I + D characters) of the runs over R and T from text_begin on, re-scored from
    the text with the matrix; asserts the '=' / X split by identity, that equal neighbours are merged, that clips stand only at
    the ends, that the script neither begins nor ends with I or D, and that its first and last aligned column have s > 0"""
    i, t, score, distance, columns = 0, text_begin, 0, 0, []
    for k, (run, op) in enumerate(runs):
        assert run >= 1 and op in af.LETTER_OF_OP, (run, op)
        if op == OP_S:
            assert k in (0, len(runs) - 1), runs
            i += run
            continue
        if op in (OP_I, OP_D):
            score -= matrix.o + run * matrix.e
        for _ in range(run):
            if op in (OP_EQ, OP_X):
                assert vc.sub(alphabet, R[i], T[t]) == (op == OP_X), (i, t, op)
                columns.append(matrix.s(alphabet, R[i], T[t]))
                score += columns[-1]
                i, t = i + 1, t + 1
            elif op == OP_I:
                i += 1
            else:
                t += 1
        distance += run * (op != OP_EQ)
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), runs
    inner = [op for _, op in runs if op != OP_S]
    assert not inner or (inner[0] in (OP_EQ, OP_X) and inner[-1] in (OP_EQ, OP_X)), runs
    assert not columns or (columns[0] > 0 and columns[-1] > 0), (runs, columns[:1], columns[-1:])
    return i, t - text_begin, score, distance


class Case(sc.Case):
    """an alignment and scoring case under the matrix calls; `scoring` is a Matrix"""

    def host(self, awfm, w, x, scoring, max_ops=32, **kw):
        return awfm.align_chains_matrix_host(self.read_chars, self.offsets, self.slots, self.chosen, self.text, scoring.struct(awfm), self.ends,
                                             self.alphabet, band_pad=w, max_drift=x, max_ops=max_ops, num_read_chars=self.num_read_chars, **kw)

    def score(self, awfm, w, x, scoring, min_score=0, cap=60, **kw):
        return awfm.score_chains_matrix_host(self.read_chars, self.offsets, self.slots, self.text, scoring.struct(awfm), self.ends, self.alphabet,
                                             band_pad=w, max_drift=x, min_score=min_score, mapq_cap=cap, num_read_chars=self.num_read_chars, **kw)

    def affine(self):
        """the same case under the affine calls"""
        return sc.Case(self.read_chars.tobytes(), self.offsets, self.slots, self.chosen, self.text.tobytes(), self.ends, self.alphabet,
                       self.num_read_chars)

    def expected(self, w, x, scoring, max_ops=32, max_rows=af.MAX_LENGTH, unaligned_before=0, truncated_before=0):
        """the alignment call restated in Python"""
        want = {name: np.zeros(self.num_reads, dtype) for name, dtype in af.READ_OUTPUTS.items()}
        want["ops"] = np.zeros((self.num_reads, max_ops), np.uint32)
        unaligned, truncated = unaligned_before, truncated_before
        for r in range(self.num_reads):
            status = self.status(r, w, x, max_rows)
            if not isinstance(status, tuple):
                want["scores"][r] = status
                unaligned += status != af.NONE
                continue
            S, E, lo, hi = status
            result = local(self.read(r), bytes(self.text[S:E]), lo, hi, scoring, self.alphabet)
            for name, value in zip(af.READ_OUTPUTS, result[:6] + (len(result[6]),)):
                want[name][r] = value
            if len(result[6]) > max_ops:
                truncated += 1
            else:
                want["ops"][r, :len(result[6])] = [run << 4 | op for run, op in result[6]]
        return dict(want, numUnaligned=unaligned, numTruncated=truncated)

    def expected_scores(self, w, x, scoring, min_score=0, cap=60, unscored_before=0, mapped_before=0):
        """the scoring call restated in Python: `local` per slot, sc.read_rules per read"""
        want = {name: np.zeros((self.num_reads, self.C), dtype) for name, dtype in sc.SLOT_OUTPUTS.items()}
        want.update({name: np.zeros(self.num_reads, dtype) for name, dtype in sc.READ_OUTPUTS.items()})
        unscored, mapped, kept = unscored_before, mapped_before, self.chosen
        for r in range(self.num_reads):
            for j in range(self.C):
                self.chosen = np.full(self.num_reads, j, np.uint32)
                status = self.status(r, w, x)
                if not isinstance(status, tuple):
                    want["slotScores"][r, j] = status
                    unscored += status != af.NONE
                    continue
                S, E, lo, hi = status
                score, _, _, re, _, te, _ = local(self.read(r), bytes(self.text[S:E]), lo, hi, scoring, self.alphabet)
                want["slotScores"][r, j], want["slotReadEnds"][r, j], want["slotTextEnds"][r, j] = score, re, te
            rules = sc.read_rules([int(v) for v in want["slotScores"][r]], [int(v) for v in want["slotReadEnds"][r]],
                                  [int(v) for v in want["slotTextEnds"][r]], [int(v) for v in self.slots["sequences"][r]], min_score, cap)
            for name, value in zip(sc.READ_OUTPUTS, rules):
                want[name][r] = value
            mapped += rules[0] != sc.NO_SLOT
        self.chosen = kept
        return dict(want, numUnscored=unscored, numMapped=mapped)


def as_matrix(case):
    chosen = getattr(case, "chosen", np.zeros(case.num_reads, np.uint32))
    return Case(case.read_chars.tobytes(), case.offsets, case.slots, chosen, case.text.tobytes(), case.ends, case.alphabet, case.num_read_chars)


def random_case(*args, **kw):
    return as_matrix(ac.random_case(*args, **kw))


def assert_scripts_replay(case, got, w, x, scoring, max_ops, unbanded_every=0):
    """the restated invariants of every aligned, untruncated read -> how many there were; every `unbanded_every`-th of them is
    also held against the unbanded local score of its record, which a banded score never exceeds"""
    replayed = 0
    for r in range(case.num_reads):
        status = case.status(r, w, x)
        k, score = int(got["numOps"][r]), int(got["scores"][r])
        if not isinstance(status, tuple) or k > max_ops:
            continue
        S, E = status[:2]
        rb, re, tb, te = (int(got[name][r]) for name in ("readBegins", "readEnds", "textBegins", "textEnds"))
        assert 0 <= tb <= te <= E - S and 0 <= rb <= re <= len(case.read(r)), r
        if score == 0:
            assert (k, rb, re, tb, te, int(got["editDistances"][r])) == (0, 0, 0, 0, 0, 0), r
            continue
        runs = af.runs_of(got["ops"][r], k)
        R, T = case.read(r), bytes(case.text[S:E])
        assert replay(runs, R, T, tb, scoring, case.alphabet) == (len(R), te - tb, score, int(got["editDistances"][r])), (r, af.cigar(runs))
        assert (runs[0] == (rb, OP_S)) == (rb > 0) and (runs[-1] == (len(R) - re, OP_S)) == (re < len(R)), (r, af.cigar(runs))
        if unbanded_every and replayed % unbanded_every == 0 and len(T) <= 600:
            assert score <= unbanded_score(R, T, scoring, case.alphabet), r
        replayed += 1
    return replayed


class Builder(af.Builder):
    def case(self, skew=0):
        return as_matrix(ac.Builder.case(self, skew))


def _nucleotide(diagonal, off, entries=(), other=None, gap_open=6, gap_extend=1, name=""):
    """a nucleotide matrix: the diagonal of a, c, g, t, `off` everywhere else, then single entries ((read letter, text letter), value)
    with 'n' for the last class"""
    index = {"a": 0, "c": 1, "g": 2, "t": 3, "n": 4}
    values = np.full((CLASSES, CLASSES), off, np.int64)
    for k, d in enumerate(diagonal):
        values[k, k] = d
    if other is not None:
        values[4, :], values[:, 4] = other, other
    for (a, b), v in entries:
        values[index[a], index[b]] = v
    return Matrix(values, gap_open, gap_extend, name)


ASYMMETRIC = _nucleotide((1, 1, 1, 1), -4, [(("a", "c"), 5), (("c", "a"), -3)], name="asymmetric")
TRANSITIONS = _nucleotide((2, 2, 2, 2), -4, [(("a", "g"), 1), (("g", "a"), 1), (("c", "t"), 1), (("t", "c"), 1)], name="positive off-diagonal")
POOR_LETTER = _nucleotide((2, -1, 2, 2), -4, name="a diagonal below 0")
EXTREMES = _nucleotide((127, 127, 127, 127), -128, [(("c", "a"), -1)], name="-128, -1, 127")
FOLDING = _nucleotide((1, 1, 1, 1), -4, [(("n", "n"), 3)], other=-2, name="other x other positive")
ADVERSARIAL = (ASYMMETRIC, TRANSITIONS, POOR_LETTER, EXTREMES, FOLDING)


FILLER = b"acgt" * 16  # a third record, so that the text is long enough to build an index from


def hand_builders():
    """[(matrix, builder)] of hand-computed cases of a few letters, each under w = 0, x = 0: the band is one diagonal, so a cell's H
    is max(0, H of the cell before + s).  Values are (score, readBegin, readEnd, textBegin, textEnd, cigar)."""
    out = []
    b = Builder([b"c", b"a", FILLER])
    b.add("read a on text c scores s(a, c) = 5, not s(c, a) = -3: an X with a positive score", b"a", 0, 0, 0, (5, 0, 1, 0, 1, "1X"))
    b.add("read c on text a scores -3: nothing", b"c", 1, 0, 0, af.NOTHING)
    b.add("read c on text c: the diagonal", b"c", 0, 0, 0, (1, 0, 1, 0, 1, "1="))
    out.append((ASYMMETRIC, b))
    b = Builder([b"gggg", b"ctgg", FILLER])
    b.add("1 + 2 + 2 + 1: the script begins and ends with X", b"agga", 0, 0, 0, (6, 0, 4, 0, 4, "1X2=1X"))
    b.add("t on c, c on t: two X worth 1 each, then c on g, -4 twice", b"tccc", 1, 0, 0, (2, 0, 2, 0, 2, "2X2S"))
    out.append((TRANSITIONS, b))
    b = Builder([b"aca", b"cc", FILLER])
    b.add("2 - 1 + 2: an '=' that costs", b"aca", 0, 0, 0, (3, 0, 3, 0, 3, "3="))
    b.add("c on c alone never scores", b"cc", 1, 0, 0, af.NOTHING)
    out.append((POOR_LETTER, b))
    b = Builder([b"aaaa", b"aaa", FILLER])
    b.add("127 + 127 - 1 + 127", b"aaca", 0, 0, 0, (380, 0, 4, 0, 4, "2=1X1="))
    b.add("127, then -128 takes it to 0, then 127 again: the smaller i", b"aga", 1, 0, 0, (127, 0, 1, 0, 1, "1=2S"))
    out.append((EXTREMES, b))
    b = Builder([b"-n", b"an", FILLER])
    b.add("N and the sentinel on two other bytes: 3 + 3, both X", b"N$", 0, 0, 0, (6, 0, 2, 0, 2, "2X"))
    b.add("other on a letter is -2, other on other 3", b"rY", 1, 0, 0, (3, 1, 2, 1, 2, "1S1X"))
    out.append((FOLDING, b))
    return out
