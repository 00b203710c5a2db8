"""Shared by the tests of awfmAlignChainsAffine / awfmGpuAlignChainsAffine (include/awfm_gpu.h, "affine alignment"): a plain-Python
restatement of the definition (dict of cells, exact integers, minus infinity for a cell that does not exist, the tie and state
rules as written), an unbanded local Gotoh pass over the whole record that returns its path, a replay that re-scores a script,
the edge list with hand-computed values, and seeded random batches.  Slots, letters, texts and batches are those of
tests/align_chains_common.py."""
import numpy as np

import align_chains_common as ac
import verify_chains_common as vc

NONE, MALFORMED, TOO_WIDE, TOO_LONG = ac.NONE, ac.MALFORMED, ac.TOO_WIDE, ac.TOO_LONG
NO_SLOT = ac.NO_SLOT
MAX_LENGTH, MAX_OPS = ac.MAX_LENGTH, ac.MAX_OPS
DNA, AMINO = ac.DNA, ac.AMINO
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8
LETTER_OF_OP = {OP_I: "I", OP_D: "D", OP_S: "S", OP_EQ: "=", OP_X: "X"}
READ_OUTPUTS = dict(scores=np.uint32, editDistances=np.uint32, readBegins=np.uint32, readEnds=np.uint32, textBegins=np.uint64,
                    textEnds=np.uint64, numOps=np.uint32)
COUNTERS = ac.COUNTERS
BAND_SHAPES = ac.BAND_SHAPES
DEFAULT = (1, 4, 6, 1)  # match, mismatch, gapOpen, gapExtend
SCORINGS = (DEFAULT, (2, 4, 4, 2), (1, 1, 0, 1), (255, 255, 255, 255), (1, 0, 0, 1))
INF = float("inf")  # (compares exactly with Python's integers)


def merge(script):
    """a script in read order -> [(run, op), ...]"""
    runs = []
    for op in script:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return [(run, op) for run, op in runs]


def local(R, T, lo, hi, scoring=DEFAULT, alphabet=DNA):
    """the definition restated: (score, editDistance, readBegin, readEnd, textBegin, textEnd, [(run, op), ...]) of R against the
    record T inside the diagonals [lo, hi]; dicts of the cells that exist, -inf for the others"""
    ma, mm, o, e = scoring
    n, L = len(R), len(T)
    H, E, F = {}, {}, {}

    def get(table, i, t):
        return table.get((i, t), -INF)

    best = (0, 0, 0)  # (H, i, t)
    for i in range(n + 1):
        for t in range(max(0, i + lo), min(L, i + hi) + 1):
            if i == 0:
                H[i, t], E[i, t], F[i, t] = 0, -INF, -INF
                continue
            M = get(H, i - 1, t - 1) + (-mm if t < 1 or vc.sub(alphabet, R[i - 1], T[t - 1]) else ma)
            F[i, t] = max(get(H, i - 1, t) - o - e, get(F, i - 1, t) - e)
            E[i, t] = max(get(H, i, t - 1) - o - e, get(E, i, t - 1) - e)
            H[i, t] = max(0, M, F[i, t], E[i, t])
            if H[i, t] > best[0]:  # rows in ascending order, then columns: the smallest i, then the smallest t
                best = (H[i, t], i, t)
    score, i, t = best
    if score == 0:
        return 0, 0, 0, 0, 0, 0, []
    read_end, text_end, state, script = i, t, "H", [OP_S] * (n - i)
    while True:
        if state == "H":
            if H[i, t] == 0:
                break
            M = get(H, i - 1, t - 1) + (-mm if t < 1 or vc.sub(alphabet, R[i - 1], T[t - 1]) else ma)
            if M == H[i, t]:
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
    return score, distance, i, read_end, t, text_end, merge(reversed(script))


def unbanded_local(R, T, scoring=DEFAULT, alphabet=DNA, sequential=False):
    """the local Gotoh pass over the whole record, the same end and walk rules -> (score, the smallest and the largest diagonal
    t - i of the path's cells (None, None without a path), [(run, op), ...] without clips).  A row's E comes from a prefix
    maximum; sequential=True takes it cell by cell as the recurrence is written (slow: for a cross-check)"""
    ma, mm, o, e = scoring
    n, L = len(R), len(T)
    NEG = -(1 << 40)
    letters_t = np.array([-1 if vc.letter(alphabet, c) is None else vc.letter(alphabet, c) for c in T], np.int64)
    H = np.zeros((n + 1, L + 1), np.int64)
    E = np.full((n + 1, L + 1), NEG, np.int64)
    F = np.full((n + 1, L + 1), NEG, np.int64)
    S = np.full((n + 1, L), -mm, np.int64)  # S[i, t - 1] = s(R[i - 1], T[t - 1])
    ramp = np.arange(L + 1, dtype=np.int64) * e
    for i in range(1, n + 1):
        x = vc.letter(alphabet, R[i - 1])
        if x is not None:
            S[i] = np.where(letters_t == x, ma, -mm)
        M = np.full(L + 1, NEG, np.int64)
        M[1:] = H[i - 1, :-1] + S[i]
        F[i] = np.maximum(H[i - 1] - o - e, F[i - 1] - e)
        tilde = np.maximum(0, np.maximum(M, F[i]))
        if sequential:
            for t in range(L + 1):
                if t:
                    E[i, t] = max(H[i, t - 1] - o - e, E[i, t - 1] - e)
                H[i, t] = max(tilde[t], E[i, t])
        else:
            E[i, 1:] = np.maximum.accumulate(tilde + ramp)[:-1] - o - ramp[1:]
            H[i] = np.maximum(tilde, E[i])
    score = int(H[1:].max()) if n else 0
    if score == 0:
        return 0, None, None, []
    i, t = (int(v) for v in np.argwhere(H == score)[0])  # row-major: the smallest i, then the smallest t
    state, script, lowest, highest = "H", [], t - i, t - i
    while True:
        lowest, highest = min(lowest, t - i), max(highest, t - i)
        if state == "H":
            if H[i, t] == 0:
                break
            if t >= 1 and H[i - 1, t - 1] + S[i, t - 1] == H[i, t]:
                script.append(OP_EQ if S[i, t - 1] == ma and not vc.sub(alphabet, R[i - 1], T[t - 1]) else OP_X)
                i, t = i - 1, t - 1
            elif F[i, t] == H[i, t]:
                state = "F"
            else:
                state = "E"
        elif state == "F":
            script.append(OP_I)
            state = "H" if H[i - 1, t] - o - e >= F[i - 1, t] - e else "F"
            i -= 1
        else:
            script.append(OP_D)
            state = "H" if H[i, t - 1] - o - e >= E[i, t - 1] - e else "E"
            t -= 1
    return score, lowest, highest, merge(reversed(script))


def cigar(runs):
    return "".join(f"{run}{LETTER_OF_OP[op]}" for run, op in runs)


def runs_of(ops_row, num_ops):
    return [(int(v) >> 4, int(v) & 15) for v in ops_row[:num_ops]]


def replay(runs, R, T, text_begin, scoring=DEFAULT, alphabet=DNA):
    """(read characters, text characters, score, X + I + D characters) of the runs over R and T from text_begin on; asserts the
    '=' / X split, that equal neighbours are merged, that clips stand only at the ends, and that the script neither begins nor
    ends with I, D or X next to a clip or a read end"""
    ma, mm, o, e = scoring
    i, t, score, distance = 0, text_begin, 0, 0
    for k, (run, op) in enumerate(runs):
        assert run >= 1 and op in LETTER_OF_OP, (run, op)
        if op == OP_S:
            assert k in (0, len(runs) - 1), runs
            i += run
            continue
        if op in (OP_I, OP_D):
            score -= o + run * e
        for _ in range(run):
            if op in (OP_EQ, OP_X):
                assert vc.sub(alphabet, R[i], T[t]) == (op == OP_X), (i, t, op)
                score += -mm if op == OP_X else ma
                i, t = i + 1, t + 1
            elif op == OP_I:
                i += 1
            else:
                t += 1
        distance += run * (op != OP_EQ)
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), runs
    inner = [op for _, op in runs if op != OP_S]
    assert not inner or (inner[0] == OP_EQ and inner[-1] == OP_EQ), runs
    return i, t - text_begin, score, distance


class Case(ac.Case):
    """an alignment case under the affine call"""

    def host(self, awfm, w, x, scoring=DEFAULT, max_ops=32, **kw):
        return awfm.align_chains_affine_host(self.read_chars, self.offsets, self.slots, self.chosen, self.text, self.ends, self.alphabet,
                                             band_pad=w, max_drift=x, scoring=scoring, max_ops=max_ops, num_read_chars=self.num_read_chars, **kw)

    def status(self, r, w, x, max_rows=MAX_LENGTH):
        """NONE .. TOO_LONG by the definition in exact integers, or (record start, record end, lo, hi): there is no overhang"""
        status = super().status(r, w, x, max_rows)
        if status != ac.OVERHANG:
            return status
        j = int(self.chosen[r])
        S, E = self.record(int(self.slots["sequences"][r, j]))
        bD, eD = int(self.slots["chainBeginDiagonals"][r, j]), int(self.slots["chainEndDiagonals"][r, j])
        return S, E, min(bD, eD) - w, max(bD, eD) + w

    def expected(self, w, x, scoring=DEFAULT, max_ops=32, max_rows=MAX_LENGTH, unaligned_before=0, truncated_before=0):
        """the whole call restated in Python; the rows of ops hold the runs where they fit and zeros elsewhere"""
        want = {name: np.zeros(self.num_reads, dtype) for name, dtype in READ_OUTPUTS.items()}
        want["ops"] = np.zeros((self.num_reads, max_ops), np.uint32)
        unaligned, truncated = unaligned_before, truncated_before
        for r in range(self.num_reads):
            status = self.status(r, w, x, max_rows)
            if not isinstance(status, tuple):
                want["scores"][r] = status
                unaligned += status != NONE
                continue
            S, E, lo, hi = status
            score, distance, rb, re, tb, te, runs = local(self.read(r), bytes(self.text[S:E]), lo, hi, scoring, self.alphabet)
            for name, value in zip(READ_OUTPUTS, (score, distance, rb, re, tb, te, len(runs))):
                want[name][r] = value
            if len(runs) > max_ops:
                truncated += 1
            else:
                want["ops"][r, :len(runs)] = [run << 4 | op for run, op in runs]
        return dict(want, numUnaligned=unaligned, numTruncated=truncated)


assert_equal = ac.assert_equal  # every output but the rows of ops of truncated reads: the names come from `want`


def assert_scripts_replay(case, got, w, x, scoring, max_ops):
    """the invariants of every aligned, untruncated read -> how many there were"""
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
        runs = runs_of(got["ops"][r], k)
        R, T = case.read(r), bytes(case.text[S:E])
        assert replay(runs, R, T, tb, scoring, case.alphabet) == (len(R), te - tb, score, int(got["editDistances"][r])), (r, cigar(runs))
        assert (runs[0] == (rb, OP_S)) == (rb > 0) and (runs[-1] == (len(R) - re, OP_S)) == (re < len(R)), (r, cigar(runs))
        replayed += 1
    return replayed


def as_affine(case):
    """an ac.Case (ac.random_case's, say) under the affine call"""
    return Case(case.read_chars.tobytes(), case.offsets, case.slots, case.chosen, case.text.tobytes(), case.ends, case.alphabet, case.num_read_chars)


def random_case(*args, **kw):
    return as_affine(ac.random_case(*args, **kw))


class Builder(ac.Builder):
    """ac.Builder with what a read must get under the affine call: a status, or (score, readBegin, readEnd, textBegin, textEnd,
    cigar); a score of 0 comes with zeros and an empty script"""

    def case(self, skew=0):
        return as_affine(super().case(skew))

    def check(self, got, max_ops):
        bad = []
        for r, (name, value) in enumerate(zip(self.names, self.values)):
            k = int(got["numOps"][r])
            have = tuple(int(got[f][r]) for f in ("scores", "readBegins", "readEnds", "textBegins", "textEnds"))
            if isinstance(value, tuple):
                have += (cigar(runs_of(got["ops"][r], k)) if k <= max_ops else None,)
                if have != value:
                    bad.append((name, have, value))
            elif value is not None and have + (k, int(got["editDistances"][r])) != (value, 0, 0, 0, 0, 0, 0):
                bad.append((name, have, value))
        assert not bad, bad

    def unaligned(self):
        return sum(v in (MALFORMED, TOO_WIDE, TOO_LONG) for v in self.values if not isinstance(v, tuple))


NOTHING = (0, 0, 0, 0, 0, "")
R0, R2, EDGE_RECORDS, BASE = ac.R0, ac.R2, ac.EDGE_RECORDS, ac.BASE


def edge_builder(w, x):
    """the edge list under (1, 4, 6, 1) for one (w, x) with w >= 2 and x >= 3: every value computed by hand.  BASE is R2[10:30];
    a substituted character is an n, which matches nothing."""
    b = Builder(EDGE_RECORDS)
    L, last = len(R2), len(EDGE_RECORDS) - 1
    b.add("n = 0", b"", 0, 5, 5, NOTHING)
    b.add("n = 1 equal: the first c the band reaches", b"c", 0, 3, 3, (1, 0, 1, 3, 4, "1="))
    b.add("n = 1 different", b"n", 0, 3, 3, NOTHING)
    b.add("exact", BASE, 2, 10, 10, (20, 0, 20, 10, 30, "20="))
    b.add("exact at the record's first character", R2[:20], 2, 0, 0, (20, 0, 20, 0, 20, "20="))
    b.add("exact at the record's last character", R2[L - 20:], 2, L - 20, L - 20, (20, 0, 20, L - 20, L, "20="))
    b.add("exact in the first record", R0[2:14], 0, 2, 2, (12, 0, 12, 2, 14, "12="))
    # a substitution p characters from the start: the prefix is worth p - 4
    b.add("sub 3 from the start: clipped", BASE[:3] + b"n" + BASE[4:], 2, 10, 10, (16, 4, 20, 14, 30, "4S16="))
    b.add("sub 4 from the start: the prefix scores 0, the tie goes to the clip", BASE[:4] + b"n" + BASE[5:], 2, 10, 10, (15, 5, 20, 15, 30, "5S15="))
    b.add("sub 5 from the start: kept", BASE[:5] + b"n" + BASE[6:], 2, 10, 10, (15, 0, 20, 10, 30, "5=1X14="))
    b.add("sub 3 from the end: clipped", BASE[:16] + b"n" + BASE[17:], 2, 10, 10, (16, 0, 16, 10, 26, "16=4S"))
    b.add("sub 4 from the end: the tie goes to the smaller i", BASE[:15] + b"n" + BASE[16:], 2, 10, 10, (15, 0, 15, 10, 25, "15=5S"))
    b.add("sub 5 from the end: kept", BASE[:14] + b"n" + BASE[15:], 2, 10, 10, (15, 0, 20, 10, 30, "14=1X5="))
    # (R2[20] = R2[23]: eleven characters match before the gap, so the twelve behind it are needed to beat the clip, 13 > 11)
    b.add("three characters deleted: one run, 22 - 9", R2[10:20] + R2[23:35], 2, 10, 13, (13, 0, 22, 10, 35, "10=3D12="))
    b.add("three characters inserted: one run, 20 - 9", R2[10:20] + b"nnn" + R2[20:30], 2, 10, 7, (11, 0, 23, 10, 30, "10=3I10="))
    # the text has two characters more, one on either side of a t: unit costs take two 1-gaps, here one 2-gap and a substitution
    # are worth 40 - 8 - 4 against 41 - 7 - 7, and of the two orders the walk meets the substitution first
    b.add("one 2-gap where unit costs take two 1-gaps", R2[6:26] + b"t" + R2[29:49], 2, 6, 8, (28, 0, 41, 6, 49, "20=2D1X20="))
    for h in (1, w - 1, w, w + 1):  # (w + 1: hi = -1 resp. lo + n = L + 1, which chain alignment refuses)
        b.add(f"{h} characters over the record's first character", b"n" * h + R2[:12], 2, -h, -h, (12, h, h + 12, 0, 12, f"{h}S12="), rb=h)
        b.add(f"{h} characters over the record's last character", R2[L - 12:] + b"n" * h, 2, L - 12, L - 12, (12, 0, 12, L - 12, L, f"12={h}S"), re=12)
    b.add("fits at 2 and at 6: the smaller t", b"acgt", 4, 4, 4, (4, 0, 4, 2, 6, "4="))
    b.add("upper against lower", b"acgt", last, 0, 0, (4, 0, 4, 0, 4, "4="))
    # N matches nothing: the clip; "ac" lies at 6 and (for a band that reaches diagonal -2) at 0, the smaller t
    b.add("n against n, N against n", b"NNac", last, 4, 4, (2, 2, 4, 0, 2, "2S2=") if w >= 6 else (2, 2, 4, 6, 8, "2S2="))
    b.add("u against t: tUUt one character earlier fits as well", b"tutu", last, 10, 10, (4, 0, 4, 9, 13, "4="))
    b.add("one-residue record", b"g", 3, 0, 0, (1, 0, 1, 0, 1, "1="))
    b.add("the empty record, n = 0", b"", 1, 0, 0, NOTHING)
    b.add("the empty record, n = 1", b"a", 1, 0, 0, NOTHING, re=0)
    b.add("too wide: eD - bD = x + 1", b"acgt", 2, 0, x + 1, TOO_WIDE)
    b.add("too wide: eD - bD = -x - 1", b"a" * (x + 5), 2, x + 1, 0, TOO_WIDE)
    b.add("as wide as allowed: eD - bD = x", R2[:4], 2, 0, x, (4, 0, 4, 0, 4, "4="))
    b.add("unused: no slot", b"acgt", 0, 0, 0, NONE, chosen=NO_SLOT)
    b.add("unused: no sequence", b"acgt", NONE, 0, 0, NONE)
    b.add("unused: no anchor", b"acgt", 0, 0, 0, NONE, anchors=0)
    b.add("malformed: slots[r] = C", b"acgt", 0, 0, 0, MALFORMED, chosen=1)
    b.add("malformed: slots[r] = 2^32 - 2", b"acgt", 0, 0, 0, MALFORMED, chosen=NO_SLOT - 1)
    b.add("malformed: sequence beyond the table", b"acgt", len(EDGE_RECORDS), 0, 0, MALFORMED)
    b.add("malformed: rb > re", b"acgt", 0, 0, 0, MALFORMED, rb=3, re=2)
    b.add("malformed: re > the read's length", b"acgt", 0, 0, 0, MALFORMED, re=5)
    b.add("malformed: tb < 0", b"acgt", 0, -1, -1, MALFORMED)
    b.add("malformed: tb > te", b"acgt", 0, 2, 1, MALFORMED, rb=1, re=1)
    b.add("malformed: te > the record's length", b"acgt", 0, 13, 13, MALFORMED)
    b.add("malformed: te > the empty record's length", b"a", 1, 0, 0, MALFORMED)
    for name, bD, eD in (("-2^63", -2 ** 63, -2 ** 63), ("2^63 - 1", 2 ** 63 - 1, 2 ** 63 - 1), ("a sum that would wrap to 0", 2 ** 63 - 1, 0),
                         ("begin -2^63", -2 ** 63, 0), ("end 2^63 - 1", 0, 2 ** 63 - 1), ("a begin that would wrap", -2 ** 63 + 2, 0)):
        b.add("malformed: diagonals " + name, b"acgt", 0, bD, eD, MALFORMED, rb=2)
    return b


def outside_builder():
    """w = 0: a band that meets the record in the one cell (n, 0), and one that lies wholly behind it -- with a well-formed slot
    a band cannot lie wholly before the record for w > 0 (rb + bD >= 0 puts row n's diagonal hi at t >= w) --, and bands that
    leave it half way: all valid slots with an empty chain interval"""
    b = Builder(EDGE_RECORDS)
    L = len(R2)
    b.add("the band ends in the cell (n, 0)", b"acgt", 2, -4, -4, NOTHING, rb=4, re=4)
    b.add("the band lies behind the record", b"acgt", 2, L, L, NOTHING, rb=0, re=0)
    b.add("the band leaves the record after 8 characters", R2[L - 8:] + b"acgt", 2, L - 8, L - 8, (8, 0, 8, L - 8, L, "8=4S"), rb=0, re=0)
    b.add("the band enters the record after 4 characters", b"acgt" + R2[:8], 2, -4, -4, (8, 4, 12, 0, 8, "4S8="), rb=4, re=4)
    return b


def unit_builder():
    """(1, 1, 0, 1): a gap of one character costs 1"""
    b = Builder(EDGE_RECORDS)
    b.add("one character deleted", BASE[:10] + R2[21:30], 2, 10, 11, (18, 0, 19, 10, 30, "10=1D9="))
    b.add("one character inserted", BASE[:10] + b"n" + BASE[10:], 2, 10, 9, (19, 0, 21, 10, 30, "10=1I10="))
    return b


def shapes_builder(seed=3):
    """reads of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 300 characters (the chunk edges) cut from a record of 700, each with a
    substitution, a deleted and an inserted character where it is long enough, on the diagonal of its first character"""
    rng = np.random.default_rng(seed)
    record = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 700))
    b = Builder([record, b"acgtacgt"])
    for k, n in enumerate((0, 1, 2, 63, 64, 65, 127, 128, 129, 300)):
        at = 40 + 31 * k
        read = bytearray(record[at:at + n])
        if n >= 63:
            read[n // 2] = ord("n")
            del read[n // 3]
            read.insert(2 * n // 3, ord("a"))
        b.add(f"n = {n}", bytes(read), 0, at, at, None)
    return b


def tail_case(length):
    """ac.tail_case's two reads at the text's last byte, a substitution in their second character (1 - 4 < 0: clipped with the
    first): the second hangs one character over and is clipped by it"""
    base = ac.tail_case(length)
    b = Builder([b"acgtacg", bytes(base.text[8:])], open_end=True)
    assert bytes(b.text) == bytes(base.text) and len(b.text) == length
    n, at = 24, length - 8 - 24
    for read, (s, anchors, rb, re, bD, eD), name in zip(base.reads, base.rows, base.names):
        clip = len(read) - n
        b.add(name, read, s, bD, eD, (n - 2, 2, n, at + 2, at + n, f"2S{n - 2}=" + (f"{clip}S" if clip else "")), rb=rb, re=re, anchors=anchors)
    return b


def planted_case(seed=11, num_reads=300, w=8):
    """reads of 30..150 characters planted in records of 400 with 3 % substitutions and at most 4 inserted plus deleted characters,
    one slot each on the true begin and end diagonals"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"acgt", np.uint8)
    records = [bytes(rng.choice(letters, 400)) for _ in range(12)]
    b = Builder(records)
    for r in range(num_reads):
        s, n = int(rng.integers(0, len(records))), int(rng.integers(30, 151))
        tb = int(rng.integers(w, 400 - n - w))
        indels = {int(p): bool(rng.integers(0, 2)) for p in rng.choice(np.arange(1, n - 1), int(rng.integers(0, 5)), replace=False)}
        read = bytearray()
        for p, c in enumerate(records[s][tb:tb + n]):
            if indels.get(p) is True:
                continue  # the text's character is deleted
            read.append(int(rng.choice([v for v in letters if v != c])) if rng.random() < 0.03 else c)
            if indels.get(p) is False:
                read.append(int(rng.choice(letters)))
        b.add(f"read {r}", bytes(read), s, tb, tb + n - len(read), None)
    return b.case()
