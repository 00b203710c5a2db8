"""Shared by the tests of the end-bonus calls (include/awfm_gpu.h, "end bonus"): awfmScoreChainsEndBonus / awfmAlignChainsEndBonus and
their device calls.  A plain-Python restatement of the definition -- tests/matrix_scores_common.py's `local` with H(0, t) = B, the
value V of a cell and the end cell over V --, an unbanded Gotoh pass under the same B that returns its path, a replay that
re-scores a script from the text plus B per read end that is not clipped and checks the restated invariants, the scorings of the
tests and the hand table of the issue with its mirror image.  Slots, texts and batches are those of tests/align_chains_common.py,
matrices those of tests/matrix_scores_common.py, the per-read rules tests/score_chains_common.py's."""
import numpy as np

import align_affine_common as af
import align_chains_common as ac
import matrix_scores_common as mx
import score_chains_common as sc
import verify_chains_common as vc

DNA, AMINO = af.DNA, af.AMINO
INF = af.INF
OP_I, OP_D, OP_S, OP_EQ, OP_X = af.OP_I, af.OP_D, af.OP_S, af.OP_EQ, af.OP_X
BONUSES = (0, 1, 5, 7, 255)
UNIFORM_SCORINGS = ((1, 4, 6, 1), (2, 4, 4, 2), (1, 1, 0, 1))


class Scoring(mx.Matrix):
    """a mx.Matrix and the end bonus B"""

    def __init__(self, matrix, bonus):
        super().__init__(matrix.values, matrix.o, matrix.e, matrix.name)
        self.B = bonus

    def matrix(self):
        return mx.Matrix(self.values, self.o, self.e, self.name)

    def __repr__(self):
        return f"Scoring({self.name or 'unnamed'}, o={self.o}, e={self.e}, B={self.B})"


def uniform(scoring, bonus, alphabet=DNA):
    return Scoring(mx.uniform(alphabet, scoring), bonus)


def local(R, T, lo, hi, scoring, alphabet=DNA):
    """the definition restated: (score, editDistance, readBegin, readEnd, textBegin, textEnd, [(run, op), ...]) of R against the
    record T inside the diagonals [lo, hi]; dicts of the cells that exist, -inf for the others; row 0 holds B, the value of a
    cell of row n with H > 0 is H + B, the end cell is the first largest value in row-major order"""
    o, e, B = scoring.o, scoring.e, scoring.B
    n, L = len(R), len(T)
    H, E, F = {}, {}, {}

    def get(table, i, t):
        return table.get((i, t), -INF)

    def diagonal(i, t):
        return get(H, i - 1, t - 1) + (scoring.s(alphabet, R[i - 1], T[t - 1]) if t >= 1 else 0)

    best = (0, 0, 0)  # (V, i, t)
    for i in range(n + 1):
        for t in range(max(0, i + lo), min(L, i + hi) + 1):
            if i == 0:
                H[i, t], E[i, t], F[i, t] = B, -INF, -INF
                continue
            F[i, t] = max(get(H, i - 1, t) - o - e, get(F, i - 1, t) - e)
            E[i, t] = max(get(H, i, t - 1) - o - e, get(E, i, t - 1) - e)
            H[i, t] = max(0, diagonal(i, t), F[i, t], E[i, t])
            V = H[i, t] + B if i == n and H[i, t] > 0 else H[i, t]
            if V > best[0]:
                best = (V, i, t)
    score, i, t = best
    if score == 0:
        return 0, 0, 0, 0, 0, 0, []
    read_end, text_end, state, script = i, t, "H", [OP_S] * (n - i)
    while i > 0:  # the walk stops at H = 0 or at row 0
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


def unbanded(R, T, scoring, alphabet=DNA):
    """the Gotoh pass over the whole record under the same B, the same end and walk rules -> (score, the smallest and the largest
    diagonal t - i of the path's cells, row 0 included (None, None without a path)); a row's E from a prefix maximum"""
    o, e, B = scoring.o, scoring.e, scoring.B
    n, L = len(R), len(T)
    NEG = -(1 << 40)
    classes_t = np.array([mx.class_of(alphabet, c) for c in T], np.int64)
    H = np.zeros((n + 1, L + 1), np.int64)
    E = np.full((n + 1, L + 1), NEG, np.int64)
    F = np.full((n + 1, L + 1), NEG, np.int64)
    S = np.zeros((n + 1, L), np.int64)  # S[i, t - 1] = s(R[i - 1], T[t - 1])
    H[0] = B
    ramp = np.arange(L + 1, dtype=np.int64) * e
    for i in range(1, n + 1):
        S[i] = scoring.values[mx.class_of(alphabet, R[i - 1])][classes_t]
        M = np.full(L + 1, NEG, np.int64)
        M[1:] = H[i - 1, :-1] + S[i]
        F[i] = np.maximum(H[i - 1] - o - e, F[i - 1] - e)
        tilde = np.maximum(0, np.maximum(M, F[i]))
        E[i, 1:] = np.maximum.accumulate(tilde + ramp)[:-1] - o - ramp[1:]
        H[i] = np.maximum(tilde, E[i])
    if n == 0:
        return 0, None, None
    V = H[1:].copy()
    V[n - 1] = np.where(V[n - 1] > 0, V[n - 1] + B, V[n - 1])
    score = int(V.max())
    if score == 0:
        return 0, None, None
    i, t = (int(v) for v in np.argwhere(V == score)[0])  # row-major: the smallest i, then the smallest t
    i += 1
    state, lowest, highest = "H", t - i, t - i
    while True:
        lowest, highest = min(lowest, t - i), max(highest, t - i)
        if i == 0:
            break
        if state == "H":
            if H[i, t] == 0:
                break
            if t >= 1 and H[i - 1, t - 1] + S[i, t - 1] == H[i, t]:
                i, t = i - 1, t - 1
            elif F[i, t] == H[i, t]:
                state = "F"
            else:
                state = "E"
        elif state == "F":
            state = "H" if H[i - 1, t] - o - e >= F[i - 1, t] - e else "F"
            i -= 1
        else:
            state = "H" if H[i, t - 1] - o - e >= E[i, t - 1] - e else "E"
            t -= 1
    return score, lowest, highest


def replay(runs, R, T, text_begin, scoring, alphabet=DNA):
    """(read characters, text characters, score, X + I + D characters) of the runs over R and T from text_begin on, re-scored from
    the text with the matrix and the gap costs plus B per read end that is not clipped; asserts the '=' / X split by identity,
    that equal neighbours are merged, that clips stand only at the ends, that the script neither begins nor ends with D, and
    that next to a clip the first / last aligned column has s > 0 and is no I.  Next to an unclipped read end it may be X, a
    column with s <= 0, or I -- also when that column is the alignment's only one and a clip follows it: the cell before it
    lies in row 0, which is no end cell, so B + s > 0 (or B - o - e > 0) is all that the column needs"""
    i, t, score, distance, columns = 0, text_begin, 0, 0, []  # columns: s of a diagonal column, None for a gap's
    for k, (run, op) in enumerate(runs):
        assert run >= 1 and op in af.LETTER_OF_OP, (run, op)
        if op == OP_S:
            assert k in (0, len(runs) - 1), runs
            i += run
            continue
        if op in (OP_I, OP_D):
            score -= scoring.o + run * scoring.e
        for _ in range(run):
            if op in (OP_EQ, OP_X):
                assert vc.sub(alphabet, R[i], T[t]) == (op == OP_X), (i, t, op)
                columns.append(scoring.s(alphabet, R[i], T[t]))
                score += columns[-1]
                i, t = i + 1, t + 1
            elif op == OP_I:
                columns.append(None)
                i += 1
            else:
                columns.append(None)
                t += 1
        distance += run * (op != OP_EQ)
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), runs
    inner = [op for _, op in runs if op != OP_S]
    assert inner and inner[0] != OP_D and inner[-1] != OP_D, runs
    clipped_left, clipped_right = runs[0][1] == OP_S, runs[-1][1] == OP_S and len(runs) > 1
    if clipped_left:
        assert inner[0] in (OP_EQ, OP_X) and columns[0] > 0, runs
    if clipped_right and (clipped_left or len(columns) > 1):
        assert inner[-1] in (OP_EQ, OP_X) and columns[-1] > 0, runs
    score += scoring.B * (not clipped_left) + scoring.B * (not clipped_right)
    return i, t - text_begin, score, distance


class Case(mx.Case):
    """an alignment and scoring case under the end-bonus calls; `scoring` is a Scoring"""

    def host(self, awfm, w, x, scoring, max_ops=32, **kw):
        return awfm.align_chains_end_bonus_host(self.read_chars, self.offsets, self.slots, self.chosen, self.text, scoring.struct(awfm), scoring.B,
                                                self.ends, self.alphabet, band_pad=w, max_drift=x, max_ops=max_ops,
                                                num_read_chars=self.num_read_chars, **kw)

    def score(self, awfm, w, x, scoring, min_score=0, cap=60, **kw):
        return awfm.score_chains_end_bonus_host(self.read_chars, self.offsets, self.slots, self.text, scoring.struct(awfm), scoring.B, self.ends,
                                                self.alphabet, band_pad=w, max_drift=x, min_score=min_score, mapq_cap=cap,
                                                num_read_chars=self.num_read_chars, **kw)

    def matrix_case(self):
        """the same case under the matrix calls"""
        return mx.Case(self.read_chars.tobytes(), self.offsets, self.slots, self.chosen, self.text.tobytes(), self.ends, self.alphabet,
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
        """the scoring call restated in Python: `local` per slot, sc.read_rules per read, all on V"""
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


def as_bonus(case):
    chosen = getattr(case, "chosen", np.zeros(case.num_reads, np.uint32))
    return Case(case.read_chars.tobytes(), case.offsets, case.slots, chosen, case.text.tobytes(), case.ends, case.alphabet, case.num_read_chars)


def random_case(*args, **kw):
    return as_bonus(ac.random_case(*args, **kw))


def assert_scripts_replay(case, got, w, x, scoring, max_ops):
    """the restated invariants of every aligned, untruncated read -> how many there were"""
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
        replayed += 1
    return replayed


class Builder(af.Builder):
    def case(self, skew=0):
        return as_bonus(ac.Builder.case(self, skew))


HAND_TEXT = b"ACGTTGCAAGCTTAGC"
HAND_READ = HAND_TEXT[2:14]  # GTTGCAAGCTTA, on diagonal 2
FILLER = mx.FILLER


def substituted(read, at):
    """the read with a character that differs from the text's at `at`"""
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}[read[at]]
    return read[:at] + other + read[at + 1:]


#: the issue's table under (1, 4, 6, 1): (k characters behind the substitution, B, score, the script at the read's end)
HAND_TABLE = ((0, 5, 17, "11=1X"), (1, 4, 15, "10=1X1="), (1, 3, 13, "10=2S"), (4, 0, 7, "7=5S"), (4, 3, 13, "7=1X4="))


def mirrored(script):
    """the script of the mirror image: its runs in reverse order"""
    runs, number = [], ""
    for c in script:
        if c.isdigit():
            number += c
        else:
            runs.append(number + c)
            number = ""
    return "".join(reversed(runs))


def hand_builders():
    """[(Scoring, builder)]: the hand table and its mirror image at the read's start, w = 2 and x = 0 (five diagonals, the read's
    own in the middle).  Values are (score, readBegin, readEnd, textBegin, textEnd, cigar)"""
    out = []
    n = len(HAND_READ)
    for k, B, score, script in HAND_TABLE:
        b = Builder([HAND_TEXT, FILLER])
        end = n if script[-1] != "S" else n - int(script[script.index("=") + 1:-1])
        b.add(f"k = {k}, B = {B} at the end", substituted(HAND_READ, n - 1 - k), 0, 2, 2, (score, 0, end, 2, 2 + end, script))
        b.add(f"k = {k}, B = {B} at the start", substituted(HAND_READ, k), 0, 2, 2, (score, n - end, n, 2 + n - end, 2 + n, mirrored(script)))
        out.append((uniform((1, 4, 6, 1), B), b))
    return out


def kept_builder(scoring, k, left):
    """one read of 30 characters of a record, a substitution k characters from its end (left: from its start)"""
    rng = np.random.default_rng(77)
    record = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60))
    read = record[10:40]
    b = Builder([record, FILLER])
    b.add(f"k = {k}", substituted(read, k if left else len(read) - 1 - k), 0, 10, 10, None)
    return b


def planted_case(seed, num_reads=300, w=8):
    """af.planted_case's reads under the end-bonus calls: 30..150 characters, 3 % substitutions, at most 4 indel characters"""
    return as_bonus(af.planted_case(seed, num_reads, w))
