"""Window scores (include/awfm_gpu.h "window scores", csrc/awfm_window_affine.c) restated in plain Python for the tests of the host
twin and the device call: the local Gotoh pass of tests/align_affine_common.py over a whole window with the begin cell found by
the WALK BACK (the twin and the kernel carry origins forward instead: the tests pin one to the other), the per-read order of
the header (not looked at, malformed, clipping, too wide, too long), the slot rule, and cases: random batches, the edge list with
hand-computed values, and planted reads."""
import numpy as np

import align_affine_common as af
import verify_chains_common as vc
from align_affine_common import replay, unbanded_local  # noqa: F401  (as they are)

DNA, AMINO = vc.DNA, vc.AMINO
NONE, MALFORMED, TOO_WIDE, TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
UNUSED = 0xFFFFFFFF  # AWFM_CANDIDATES_NONE
MAX_WIDTH = MAX_LENGTH = 4096
DEFAULT, SCORINGS = af.DEFAULT, af.SCORINGS
READ_OUTPUTS = dict(scores=np.uint32, readBegins=np.uint32, readEnds=np.uint32, textBegins=np.uint64, textEnds=np.uint64)
SLOT_OUTPUTS = vc.SLOT_DTYPES
COUNTERS = ("numUnscored", "numFound")


def window_local(R, T, scoring=DEFAULT, alphabet=DNA, ties=None):
    """unbanded_local's pass and walk, returning the cells instead of the script: (score, readBegin, readEnd, textBegin, textEnd)
    of R against the window T, window-local; zeros without an alignment.  ties: a set that receives "MFE" when the walk meets a
    cell with M = F = E = H and "opened" when it leaves a gap where opening and extending tie"""
    ma, mm, o, e = scoring
    n, L = len(R), len(T)
    if n == 0 or L == 0:
        return 0, 0, 0, 0, 0
    NEG = -(1 << 40)
    letters_t = np.array([-1 if vc.letter(alphabet, c) is None else vc.letter(alphabet, c) for c in T], np.int64)
    H = np.zeros((n + 1, L + 1), np.int64)
    E = np.full((n + 1, L + 1), NEG, np.int64)
    F = np.full((n + 1, L + 1), NEG, np.int64)
    S = np.full((n + 1, L), -mm, np.int64)
    ramp = np.arange(L + 1, dtype=np.int64) * e
    for i in range(1, n + 1):
        x = vc.letter(alphabet, R[i - 1])
        if x is not None:
            S[i] = np.where(letters_t == x, ma, -mm)
        M = np.full(L + 1, NEG, np.int64)
        M[1:] = H[i - 1, :-1] + S[i]
        F[i] = np.maximum(H[i - 1] - o - e, F[i - 1] - e)
        tilde = np.maximum(0, np.maximum(M, F[i]))
        E[i, 1:] = np.maximum.accumulate(tilde + ramp)[:-1] - o - ramp[1:]
        H[i] = np.maximum(tilde, E[i])
    score = int(H[1:].max())
    if score == 0:
        return 0, 0, 0, 0, 0
    i, t = (int(v) for v in np.argwhere(H == score)[0])  # row-major: the smallest i, then the smallest t
    read_end, text_end, state = i, t, "H"
    while True:
        if state == "H":
            if H[i, t] == 0:
                break
            if t >= 1 and H[i - 1, t - 1] + S[i, t - 1] == H[i, t]:
                if ties is not None and F[i, t] == H[i, t] == E[i, t]:
                    ties.add("MFE")
                i, t = i - 1, t - 1
            elif F[i, t] == H[i, t]:
                state = "F"
            else:
                state = "E"
        elif state == "F":
            if ties is not None and H[i - 1, t] - o - e == F[i - 1, t] - e:
                ties.add("opened")
            state = "H" if H[i - 1, t] - o - e >= F[i - 1, t] - e else "F"
            i -= 1
        else:
            if ties is not None and H[i, t - 1] - o - e == E[i, t - 1] - e:
                ties.add("opened")
            state = "H" if H[i, t - 1] - o - e >= E[i, t - 1] - e else "E"
            t -= 1
    return score, i, read_end, t, text_end


def text_of(records, open_end=False):
    """the records with their NUL terminators (the last one without when open_end), and the records' ends"""
    body, ends = bytearray(), []
    for k, record in enumerate(records):
        body += record
        ends.append(len(body))
        if not (open_end and k == len(records) - 1):
            body += b"\0"
    return np.frombuffer(bytes(body), np.uint8), np.array(ends, np.uint64)


class Case:
    """one call's inputs: reads (bytes each, one after the other from `skew` bytes into the buffer on), a window per read
    (sequence, begin, end), the text and its records' ends; offsets: other offsets than the reads' own (malformed ones)"""

    def __init__(self, reads, windows, text, ends, alphabet=DNA, skew=0, offsets=None, num_read_chars=None):
        self.reads, self.alphabet, self.text, self.ends = [bytes(r) for r in reads], alphabet, np.ascontiguousarray(text, np.uint8), ends
        buffer = b"#" * skew + b"".join(self.reads)
        self.read_chars = np.frombuffer(buffer, np.uint8) if buffer else np.zeros(0, np.uint8)
        self.offsets = np.array(offsets if offsets is not None else np.cumsum([skew] + [len(r) for r in self.reads]), np.uint64)
        self.num_read_chars = self.read_chars.size if num_read_chars is None else num_read_chars
        self.num_reads = len(self.reads)
        self.sequences = np.array([w[0] for w in windows], np.uint32)
        self.begins = np.array([w[1] for w in windows], np.uint64)
        self.window_ends = np.array([w[2] for w in windows], np.uint64)

    def record(self, s):
        ends = self.ends
        if ends is None or not len(ends):
            return 0, self.text.size
        return (int(ends[s - 1]) + 1 if s else 0), int(ends[s])

    def num_sequences(self):
        return len(self.ends) if self.ends is not None and len(self.ends) else 1

    def host(self, awfm, scoring=DEFAULT, min_score=0, stride=1, column=0, **kw):
        return awfm.score_windows_affine(self.read_chars, self.offsets, self.sequences, self.begins, self.window_ends, self.text, self.ends,
                                         self.alphabet, scoring=scoring, min_score=min_score, slot_stride=stride, slot_column=column,
                                         num_read_chars=self.num_read_chars, **kw)

    def one(self, r, scoring, max_length=MAX_LENGTH):
        """(value, readBegin, readEnd, textBegin, textEnd) of read r by the header's order, in exact integers"""
        s = int(self.sequences[r])
        if s == UNUSED:
            return NONE, 0, 0, 0, 0
        begin, end = int(self.begins[r]), int(self.window_ends[r])
        a, z = int(self.offsets[r]), int(self.offsets[r + 1])
        if s >= self.num_sequences() or begin > end or a > z or z > self.num_read_chars:
            return MALFORMED, 0, 0, 0, 0
        S, E = self.record(s)
        if E < S or E > self.text.size:
            return MALFORMED, 0, 0, 0, 0
        L = E - S
        b, e = min(begin, L), min(end, L)
        if e - b > MAX_WIDTH:
            return TOO_WIDE, 0, 0, 0, 0
        if z - a > min(MAX_LENGTH, max_length):
            return TOO_LONG, 0, 0, 0, 0
        score, rb, re, tb, te = window_local(bytes(self.read_chars[a:z]), bytes(self.text[S + b:S + e]), scoring, self.alphabet)
        return (score, rb, re, b + tb, b + te) if score else (0, 0, 0, 0, 0)

    def expected(self, scoring=DEFAULT, min_score=0, stride=1, column=0, slots=None, unscored_before=0, found_before=0, max_length=MAX_LENGTH):
        """the whole call restated; slots: what the slot arrays hold before (None: the unused slot everywhere)"""
        n = self.num_reads
        want = {name: np.zeros(n, dtype) for name, dtype in READ_OUTPUTS.items()}
        for name, dtype in SLOT_OUTPUTS.items():
            want[name] = np.array(slots[name], dtype) if slots is not None else np.zeros((n, stride), dtype)
            if slots is None and name == "sequences":
                want[name][...] = UNUSED
        unscored, found = unscored_before, found_before
        for r in range(n):
            value, rb, re, tb, te = self.one(r, scoring, max_length)
            for name, v in zip(READ_OUTPUTS, (value, rb, re, tb, te)):
                want[name][r] = v
            if value == NONE:
                continue
            unscored += value >= TOO_LONG
            counts = value < TOO_LONG and value >= max(min_score, 1)
            found += counts
            slot = (int(self.sequences[r]), 1, rb, re, tb - rb, te - re) if counts else (UNUSED, 0, 0, 0, 0, 0)
            for name, v in zip(vc.SLOT_FIELDS, slot):
                want[name][r, column] = v
        return dict(want, numUnscored=int(unscored), numFound=int(found))


def assert_equal(got, want, names=None, what=""):
    for name in (names or want):
        if name in COUNTERS:
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            a, b = np.asarray(got[name]), np.asarray(want[name])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape, a.dtype, b.dtype)
            if not np.array_equal(a, b):
                at = np.argwhere(a != b)[0]
                raise AssertionError((what, name, tuple(int(v) for v in at), a[tuple(at)], b[tuple(at)]))


def letters_of(alphabet):
    return np.frombuffer(b"acgt" if alphabet == DNA else vc.AMINO_LETTERS.encode(), np.uint8)


def random_text(rng, alphabet, lengths):
    letters = letters_of(alphabet)
    records = []
    for length in lengths:
        body = rng.choice(letters, length)
        if length > 40:  # some ambiguity letters
            body[rng.integers(0, length, max(length // 200, 1))] = ord("n") if alphabet == DNA else ord("x")
        records.append(bytes(body))
    return records


def random_case(seed, num_reads, alphabet=DNA, text_length=4096, num_records=9, lengths=None, max_length=60, max_window=200, max_rate=0.12,
                skipped=0.1, broken=0.03, clipped=0.1, skew=0):
    """reads planted in a text of records (an empty one and a one-residue one among them), each with a window around its locus of a
    random width that may cut the locus; some reads not looked at, a few malformed, some windows clipped by the record's end"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, text_length, num_records - 3))
    sizes = [int(v) for v in np.diff(np.concatenate(([0], cuts, [text_length])))]
    sizes += [0, 1]
    records = random_text(rng, alphabet, sizes)
    text, ends = text_of(records)
    letters = letters_of(alphabet)
    big = [s for s, record in enumerate(records) if len(record) >= 8]
    reads, windows = [], []
    for r in range(num_reads):
        n = int(lengths[r]) if lengths is not None else int(rng.integers(0, max_length + 1))
        s = int(rng.choice(big))
        L = len(records[s])
        width = int(rng.integers(0, max_window + 1))
        at = int(rng.integers(0, max(L - min(n, L), 0) + 1))
        read = bytes(vc.edit(rng, records[s][at:at + n], rng.uniform(0, max_rate), letters))[:MAX_LENGTH] if n else b""
        begin = max(at - int(rng.integers(0, width + 1)), 0)
        end = begin + width
        roll = rng.uniform()
        if roll < skipped:
            s = UNUSED
        elif roll < skipped + broken:
            kind = int(rng.integers(0, 3))
            if kind == 0:
                s = len(records) + int(rng.integers(0, 3))
            elif kind == 1:
                begin, end = end + 1, begin
            else:
                s = 0xFFFFFFFE
        elif roll < skipped + broken + clipped:
            begin = max(L - int(rng.integers(0, width + 1)), 0)
            end = begin + width + int(rng.integers(0, 2)) * (1 << 40)
        reads.append(read)
        windows.append((s, begin, end))
    return Case(reads, windows, text, ends, alphabet, skew=skew)


class Builder:
    """reads added one at a time with their window and the five values they must get, computed by hand"""

    def __init__(self, records, alphabet=DNA):
        self.records, self.alphabet = records, alphabet
        self.reads, self.windows, self.values, self.names = [], [], [], []

    def add(self, name, read, window, value):
        self.names.append(name)
        self.reads.append(read)
        self.windows.append(window)
        self.values.append(value)

    def case(self, skew=0):
        text, ends = text_of(self.records)
        return Case(self.reads, self.windows, text, ends, self.alphabet, skew=skew)

    def check(self, got):
        for r, (name, value) in enumerate(zip(self.names, self.values)):
            have = tuple(int(got[field][r]) for field in READ_OUTPUTS)
            assert have == value, (name, have, value)


NOTHING = (0, 0, 0, 0, 0)
#              0         1         2         3
#              0123456789012345678901234567890123456789
EDGE_RECORDS = [b"ttttacgtacgtaccccccccccacgtacgtacgggg",  # 37: the read acgtacgtac at 4 and at 23
                b"",
                b"ggggggggggacgtacgtac",                     # 20: the read at the record's end
                b"acgtacgtacgggggggggg",                     # 20: and at its start
                b"ccccaaaaccccttttcccc",                     # 20
                b"ggacgtnacgtgg" + b"c" * 10,                # an ambiguity letter in the text
                b"aaaaaaaaaa"]
READ = b"acgtacgtac"


def edge_builder():
    """the edge list under DEFAULT = (1, 4, 6, 1): every value computed by hand"""
    b = Builder(EDGE_RECORDS)
    b.add("the read in a window of its own width", READ, (0, 4, 14), (10, 0, 10, 4, 14))
    b.add("an empty read", b"", (0, 0, 37), NOTHING)
    b.add("an empty window", READ, (0, 9, 9), NOTHING)
    b.add("a window wholly behind the record's end", READ, (0, 40, 90), NOTHING)
    b.add("a window in an empty record", READ, (1, 0, 10), NOTHING)
    b.add("not looked at", READ, (UNUSED, 0, 37), (NONE, 0, 0, 0, 0))
    b.add("a window clipped at the record's end", READ, (2, 5, 1 << 40), (10, 0, 10, 10, 20))
    b.add("a window at the record's start", READ, (3, 0, 12), (10, 0, 10, 0, 10))
    b.add("a window that cuts the read's locus: its first six characters", READ, (3, 0, 6), (6, 0, 6, 0, 6))
    b.add("begin > end", READ, (0, 10, 9), (MALFORMED, 0, 0, 0, 0))
    b.add("a bad sequence", READ, (len(EDGE_RECORDS), 0, 10), (MALFORMED, 0, 0, 0, 0))
    b.add("two equal placements: the smallest i, then the smallest t", READ, (0, 0, 37), (10, 0, 10, 4, 14))
    b.add("the second placement alone", READ, (0, 5, 37), (10, 0, 10, 23, 33))
    # aaaacccctttt against ccccaaaaccccttttcccc from 4 on: twelve matches
    b.add("clips at both ends of the read", b"gg" + b"aaaacccctttt" + b"gg", (4, 0, 20), (12, 2, 14, 4, 16))
    # acgt n acgt in the text, acgtaacgt in the read: 4 - 4 + 4 = 4 through the letter, so the first acgt alone wins: 4
    b.add("an ambiguity letter in the text matches nothing", b"acgtaacgt", (5, 0, 23), (4, 0, 4, 2, 6))
    b.add("an ambiguity letter in the read matches nothing", b"acgtnacgt", (5, 0, 23), (4, 0, 4, 2, 6))
    b.add("a one-character read", b"g", (2, 3, 20), (1, 0, 1, 3, 4))
    b.add("a one-character window", READ, (0, 4, 5), (1, 0, 1, 4, 5))
    return b


TIE_SCORING = (3, 2, 0, 1)  # a free opening: a gap of g costs g


def tie_builder():
    """the two ties of the origin rule under TIE_SCORING, computed by hand.
    accac in acaac: the diagonal a= c= c/a a= c= scores 3 + 3 - 2 + 3 + 3 = 10 from (0, 0) to (5, 5).  At its cell (3, 3)
    M = H(2, 2) - 2 = 6 - 2 = 4, F = H(2, 3) - 1 = 5 - 1 = 4 (H(2, 3) = H(2, 2) - 1) and E = H(3, 2) - 1 = 5 - 1 = 4: M = F = E = H,
    and the origin follows M.
    acca in aaa: a= at (1, 1) is 3; the read's cc is a gap: F(2, 1) = 3 - 1 = 2, and at (3, 1) opening gives H(2, 1) - 0 - 1 = 1 and
    extending F(2, 1) - 1 = 1: a tie, the gap was OPENED at (2, 1), whose H = F leads on to (1, 1); then a= makes H(4, 2) = 4.
    (4, 3) holds 4 as well (H(3, 2) = 1 the same way): the smallest t wins."""
    b = Builder([b"acaac", b"aaa"])
    b.add("a cell where M = F = E = H: the origin follows M", b"accac", (0, 0, 5), (10, 0, 5, 0, 5))
    b.add("a gap where opening and extending tie: opened", b"acca", (1, 0, 3), (4, 0, 4, 0, 2))
    return b


def wide_case(n, W, seed=7):
    """one read of n characters in a window of W (record of W + 40): planted at window offset 10 when it fits"""
    rng = np.random.default_rng(seed)
    record = bytes(rng.choice(letters_of(DNA), W + 40))
    text, ends = text_of([b"acgt", record])
    at = 10
    read = record[at:at + n] if n <= W else record[:n] + bytes(rng.choice(letters_of(DNA), max(n - len(record), 0)))
    return Case([read[:n]], [(1, 0, W)], text, ends)


def planted_case(seed, num_reads=200, length=150, width=600):
    """reads of `length` characters with up to 8 % substitutions and up to two gaps of 1..3, each in a window of `width` positions
    that holds its locus at a random offset; -> the case"""
    rng = np.random.default_rng(seed)
    letters = letters_of(DNA)
    record = bytes(rng.choice(letters, 20000))
    text, ends = text_of([record])
    reads, windows = [], []
    for _ in range(num_reads):
        at = int(rng.integers(width, len(record) - 2 * width))
        read = bytearray(record[at:at + length])
        for p in rng.choice(length, int(rng.integers(0, length * 8 // 100 + 1)), replace=False):
            read[p] = int(rng.choice([c for c in letters if c != read[p]]))
        for _ in range(int(rng.integers(0, 3))):
            p, g = int(rng.integers(20, len(read) - 20)), int(rng.integers(1, 4))
            if rng.integers(0, 2):
                read[p:p] = bytes(rng.choice(letters, g))
            else:
                del read[p:p + g]
        begin = at - int(rng.integers(0, width - length - 10))
        reads.append(bytes(read))
        windows.append((0, begin, begin + width))
    return Case(reads, windows, text, ends)
