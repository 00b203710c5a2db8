"""Shared by the tests of awfmAlignChains / awfmGpuAlignChains (include/awfm_gpu.h, "chain alignment"): a plain-Python restatement
of the definition (dict of cells, exact integers, the direction and end rules as written), an unbanded fitting dynamic
programme, the edge list with hand-computed values, and seeded random batches.  The slot arrays, the letter mapping and the
texts are those of tests/verify_chains_common.py."""
import os

import numpy as np

import verify_chains_common as vc

NONE, MALFORMED, TOO_WIDE, TOO_LONG, OVERHANG = vc.NONE, vc.MALFORMED, vc.TOO_WIDE, vc.TOO_LONG, 0xFFFFFFFB
NO_SLOT = vc.NO_SLOT
MAX_LENGTH, MAX_OPS = 1 << 16, 4096
DNA, AMINO = vc.DNA, vc.AMINO
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
LETTER_OF_OP = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
READ_OUTPUTS = dict(editDistances=np.uint32, textBegins=np.uint64, textEnds=np.uint64, numOps=np.uint32)
COUNTERS = ("numUnaligned", "numTruncated")
BAND_SHAPES = vc.BAND_SHAPES


def fitting(R, T, lo, hi, alphabet=DNA):
    """the definition restated: (distance, textBegin, textEnd, [(run, op), ...]) of R against the record T inside the diagonals
    [lo, hi]; a dict of the cells that exist"""
    n, L = len(R), len(T)
    H, direction = {}, {}
    for i in range(n + 1):
        for t in range(max(0, i + lo), min(L, i + hi) + 1):
            if i == 0:
                H[i, t] = 0
                continue
            options = []  # (value, rank of the direction): diagonal before up before left
            if (i - 1, t - 1) in H:
                options.append((H[i - 1, t - 1] + vc.sub(alphabet, R[i - 1], T[t - 1]), 0))
            if (i - 1, t) in H:
                options.append((H[i - 1, t] + 1, 1))
            if (i, t - 1) in H:
                options.append((H[i, t - 1] + 1, 2))
            H[i, t], direction[i, t] = min(options)
    distance, end = min((H[n, t], t) for t in range(L + 1) if (n, t) in H)
    i, t, script = n, end, []
    while i > 0:
        d = direction[i, t]
        if d == 0:
            script.append(OP_X if vc.sub(alphabet, R[i - 1], T[t - 1]) else OP_EQ)
            i, t = i - 1, t - 1
        elif d == 1:
            script.append(OP_I)
            i -= 1
        else:
            script.append(OP_D)
            t -= 1
    runs = []
    for op in reversed(script):
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return distance, t, end, [(run, op) for run, op in runs]


def unbanded_fitting(R, T, alphabet=DNA):
    """the fitting distance without a band: global in R, free at both ends in T"""
    letters_t = np.array([-1 if vc.letter(alphabet, c) is None else vc.letter(alphabet, c) for c in T], np.int64)
    row = np.zeros(len(T) + 1, np.int64)
    ramp = np.arange(len(T) + 1)
    for c in R:
        x = vc.letter(alphabet, c)
        cost = np.ones(len(T), np.int64) if x is None else (letters_t != x).astype(np.int64)
        new = np.empty_like(row)
        new[0] = row[0] + 1
        new[1:] = np.minimum(row[:-1] + cost, row[1:] + 1)
        row = np.minimum.accumulate(new - ramp) + ramp  # H[t] = min over t' <= t of new[t'] + (t - t')
    return int(row.min())


def cigar(runs):
    return "".join(f"{run}{LETTER_OF_OP[op]}" for run, op in runs)


def runs_of(ops_row, num_ops):
    return [(int(v) >> 4, int(v) & 15) for v in ops_row[:num_ops]]


def replay(runs, R, T, alphabet=DNA):
    """(read characters, text characters, distance) of the runs over R and T; asserts the '=' / X split on the way"""
    i = t = distance = 0
    for run, op in runs:
        assert run >= 1 and op in LETTER_OF_OP, (run, op)
        for _ in range(run):
            if op in (OP_EQ, OP_X):
                assert vc.sub(alphabet, R[i], T[t]) == (op == OP_X), (i, t, op)
                i, t = i + 1, t + 1
            elif op == OP_I:
                i += 1
            else:
                t += 1
            distance += op != OP_EQ
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), runs  # equal neighbours are merged
    return i, t, distance


class Case(vc.Case):
    """a verification case and the slot of every read to align"""

    def __init__(self, read_chars, offsets, slots, chosen, text, ends=None, alphabet=DNA, num_read_chars=None):
        super().__init__(read_chars, offsets, slots, text, ends, alphabet, num_read_chars)
        self.chosen = np.ascontiguousarray(chosen, dtype=np.uint32)

    def host(self, awfm, w, x, max_ops=32, **kw):
        return awfm.align_chains_host(self.read_chars, self.offsets, self.slots, self.chosen, self.text, self.ends, self.alphabet, band_pad=w,
                                      max_drift=x, max_ops=max_ops, num_read_chars=self.num_read_chars, **kw)

    def record(self, s):
        S = 0 if not s or self.ends is None else int(self.ends[s - 1]) + 1
        E = len(self.text) if self.ends is None or not len(self.ends) else int(self.ends[s])
        return S, E

    def read(self, r):
        return bytes(self.read_chars[int(self.offsets[r]):int(self.offsets[r + 1])])

    def status(self, r, w, x, max_rows=MAX_LENGTH):
        """NONE .. OVERHANG by the definition in exact integers, or (record start, record end, lo, hi) of a read that is aligned"""
        j = int(self.chosen[r])
        if j == NO_SLOT:
            return NONE
        if j >= self.C:
            return MALFORMED
        s = int(self.slots["sequences"][r, j])
        if s == NONE or int(self.slots["chainAnchors"][r, j]) == 0:
            return NONE
        o0, o1 = int(self.offsets[r]), int(self.offsets[r + 1])
        if o0 > o1 or o1 > self.num_read_chars:
            return MALFORMED
        n = o1 - o0
        rb, re = int(self.slots["chainReadBegins"][r, j]), int(self.slots["chainReadEnds"][r, j])
        if rb > re or re > n:
            return MALFORMED
        if s >= (1 if self.ends is None or not len(self.ends) else len(self.ends)):
            return MALFORMED
        S, E = self.record(s)
        bD, eD = int(self.slots["chainBeginDiagonals"][r, j]), int(self.slots["chainEndDiagonals"][r, j])
        tb, te = rb + bD, re + eD
        if E < S or E > len(self.text) or tb < 0 or tb > te or te > E - S:
            return MALFORMED
        if abs(eD - bD) > x:
            return TOO_WIDE
        if n > max_rows:
            return TOO_LONG
        lo, hi = min(bD, eD) - w, max(bD, eD) + w
        if hi < 0 or lo + n > E - S:
            return OVERHANG
        return S, E, lo, hi

    def expected(self, w, x, max_ops=32, max_rows=MAX_LENGTH, unaligned_before=0, truncated_before=0):
        """the whole call restated in Python; the rows of ops hold the runs where they fit and zeros elsewhere"""
        want = {name: np.zeros(self.num_reads, dtype) for name, dtype in READ_OUTPUTS.items()}
        want["ops"] = np.zeros((self.num_reads, max_ops), np.uint32)
        unaligned, truncated = unaligned_before, truncated_before
        for r in range(self.num_reads):
            status = self.status(r, w, x, max_rows)
            if not isinstance(status, tuple):
                want["editDistances"][r] = status
                unaligned += status != NONE
                continue
            S, E, lo, hi = status
            distance, begin, end, runs = fitting(self.read(r), bytes(self.text[S:E]), lo, hi, self.alphabet)
            want["editDistances"][r], want["textBegins"][r], want["textEnds"][r], want["numOps"][r] = distance, begin, end, len(runs)
            if len(runs) > max_ops:
                truncated += 1
            else:
                want["ops"][r, :len(runs)] = [run << 4 | op for run, op in runs]
        return dict(want, numUnaligned=unaligned, numTruncated=truncated)


def assert_equal(got, want, names=None, what="", fill=None):
    """every output but the rows of ops of truncated reads; of the other rows the runs, and with `fill` (the byte the rows held
    before the call) that nothing behind the runs was written.  `want` comes from Case.expected or from another call."""
    names = list(names or want)
    for name in names:
        if name in COUNTERS:
            assert got[name] == want[name], (what, name, got[name], want[name])
        elif name != "ops":
            bad = np.flatnonzero(got[name] != want[name])
            assert not len(bad), (what, name, bad[:5].tolist(), int(got[name][bad[0]]), int(want[name][bad[0]]))
    if "ops" in names:
        assert got["ops"].shape == want["ops"].shape, (what, got["ops"].shape, want["ops"].shape)
        max_ops = want["ops"].shape[1]
        counts = np.asarray(want["numOps"], np.int64)  # (a caller that compares the rows passes the counts along)
        pattern = None if fill is None else np.uint32(fill * 0x01010101)
        for r in range(len(counts)):
            if counts[r] > max_ops:
                continue
            k = int(counts[r])
            assert np.array_equal(got["ops"][r, :k], want["ops"][r, :k]), (what, r, cigar(runs_of(got["ops"][r], k)), cigar(runs_of(want["ops"][r], k)))
            if pattern is not None:
                assert (got["ops"][r, k:] == pattern).all(), (what, r, "written behind the runs")


class Builder:
    """a text of records (vc.Builder's) and reads with one slot each, added one at a time with what the read must get:
    a status, or (distance, textBegin, textEnd, cigar)"""

    def __init__(self, records, open_end=False, alphabet=DNA):
        base = vc.Builder(records, open_end, alphabet)
        self.text, self.ends, self.alphabet = base.text, base.ends, alphabet
        self.reads, self.rows, self.chosen, self.values, self.names = [], [], [], [], []

    def add(self, name, read, s, bD, eD, value, rb=0, re=None, anchors=1, chosen=0):
        self.reads.append(bytes(read))
        self.rows.append((s, anchors, rb, len(read) if re is None else re, bD, eD))
        self.chosen.append(chosen)
        self.values.append(value)
        self.names.append(name)

    def case(self, skew=0):
        offsets = np.cumsum([skew] + [len(r) for r in self.reads])
        rows = np.array(self.rows, dtype=object)
        slots = {name: np.array([[int(v)] for v in rows[:, k]], vc.SLOT_DTYPES[name]) for k, name in enumerate(vc.SLOT_FIELDS)}
        return Case(b"#" * skew + b"".join(self.reads), offsets, slots, self.chosen, self.text, self.ends, self.alphabet)

    def check(self, got, max_ops):
        """the hand-computed values against a call's outputs"""
        bad = []
        for r, (name, value) in enumerate(zip(self.names, self.values)):
            if isinstance(value, tuple):
                distance, begin, end, script = value
                k = int(got["numOps"][r])
                have = (int(got["editDistances"][r]), int(got["textBegins"][r]), int(got["textEnds"][r]),
                        cigar(runs_of(got["ops"][r], k)) if k <= max_ops else None)
                if have != (distance, begin, end, script):
                    bad.append((name, have, value))
            else:
                have = (int(got["editDistances"][r]), int(got["textBegins"][r]), int(got["textEnds"][r]), int(got["numOps"][r]))
                if have != (value, 0, 0, 0):
                    bad.append((name, have, value))
        assert not bad, bad

    def unaligned(self):
        return sum(v in (MALFORMED, TOO_WIDE, TOO_LONG, OVERHANG) for v in self.values if not isinstance(v, tuple))


#       0         1         2         3         4         5
#       01234567890123456789012345678901234567890123456789012
R0 = b"gatcctgaagtcatgc"
R2 = b"ttgacgcatagcctagtaccgatgcaatcggtaccatgcgtaagctaggcatc"
EDGE_RECORDS = [R0, b"", R2, b"g", b"ttacgtacgtcc", b"ACGTNNacntUUtt"]
BASE = R2[10:30]  # gcctagtaccgatgcaatcg


def edge_builder(w, x):
    """the edge list for one (w, x) with w >= 2 and x >= 3: every value computed by hand.  A read is aligned on the diagonals
    [min(bD, eD) - w, max(bD, eD) + w] of its record; of several ends at the smallest distance the leftmost counts, and of
    several predecessors the diagonal one before the upper one before the left one."""
    b = Builder(EDGE_RECORDS)
    L, last = len(R2), len(EDGE_RECORDS) - 1
    at = max(5 - w, 0)
    b.add("n = 0: no run, at max(lo, 0)", b"", 0, 5, 5, (0, at, at, ""))
    b.add("n = 1 equal: the first c of the record", b"c", 0, 3, 3, (0, 3, 4, "1="))
    t = max(4 - w, 0)  # nothing matches n: every cell of row 1 holds 1, the leftmost one counts; in column 0 it has no diagonal
    b.add("n = 1 different", b"n", 0, 3, 3, (1, t - 1, t, "1X") if t >= 1 else (1, 0, 0, "1I"))
    b.add("exact at the record's first character", R2[:20], 2, 0, 0, (0, 0, 20, "20="))
    b.add("exact at the record's last character", R2[L - 20:], 2, L - 20, L - 20, (0, L - 20, L, "20="))
    b.add("exact in the first record", R0[2:14], 0, 2, 2, (0, 2, 14, "12="))
    b.add("sub first: diagonal and up tie at 1, diagonal counts", b"t" + BASE[1:], 2, 10, 10, (1, 10, 30, "1X19="))
    b.add("sub middle", BASE[:10] + b"a" + BASE[11:], 2, 10, 10, (1, 10, 30, "10=1X9="))
    # the last character as X ends at 30, as I at 29 with the same distance: the smaller end counts
    b.add("sub last: the smaller end makes it an insertion", BASE[:19] + b"a", 2, 10, 10, (1, 10, 29, "19=1I"))
    b.add("ins first: a substitution one character earlier costs the same, the diagonal counts", b"c" + R2[10:29], 2, 9, 9, (1, 9, 29, "1X19="))
    b.add("ins middle", BASE[:10] + b"a" + R2[20:29], 2, 10, 9, (1, 10, 29, "10=1I9="))
    b.add("ins last", R2[10:29] + b"a", 2, 10, 10, (1, 10, 29, "19=1I"))
    b.add("del first: the text's ends are free", R2[11:30], 2, 10, 11, (0, 11, 30, "19="))
    b.add("del middle", BASE[:10] + R2[21:30], 2, 10, 11, (1, 10, 30, "10=1D9="))
    b.add("del last: the text's ends are free", R2[10:29], 2, 10, 11, (0, 10, 29, "19="))
    b.add("fits at 2 and at 6: the smaller end", b"acgt", 4, 4, 4, (0, 2, 6, "4="))
    b.add("upper against lower", b"acgt", last, 0, 0, (0, 0, 4, "4="))
    # N matches nothing: two substitutions where it lies, or (a band that reaches diagonal -2) two insertions ahead of "AC"
    b.add("n against n, N against n", b"NNac", last, 4, 4, (2, 0, 2, "2I2=") if w >= 6 else (2, 4, 8, "2X2="))
    b.add("u against t: tUUt one character earlier fits as well", b"tutu", last, 10, 10, (0, 9, 13, "4="))
    b.add("one-residue record", b"g", 3, 0, 0, (0, 0, 1, "1="))
    b.add("the empty record, n = 0", b"", 1, 0, 0, (0, 0, 0, ""))
    b.add("the empty record, n = 1", b"a", 1, 0, 0, (1, 0, 0, "1I"), re=0)
    b.add("hi = 0: w characters ahead of the record", b"n" * w + R2[:12], 2, -w, -w, (w, 0, 12, f"{w}I12="), rb=w)
    b.add("hi = 1: w - 1 characters ahead of the record", b"n" * (w - 1) + R2[:12], 2, 1 - w, 1 - w, (w - 1, 0, 12, f"{w - 1}I12="), rb=w - 1)
    b.add("hi = -1: w + 1 characters ahead of the record", b"n" * (w + 1) + R2[:12], 2, -w - 1, -w - 1, OVERHANG, rb=w + 1)
    b.add("lo + n = L: w characters behind the record", R2[L - 12:] + b"n" * w, 2, L - 12, L - 12, (w, L - 12, L, f"12={w}I"), re=12)
    b.add("lo + n = L - 1: w - 1 characters behind the record", R2[L - 12:] + b"n" * (w - 1), 2, L - 12, L - 12, (w - 1, L - 12, L, f"12={w - 1}I"), re=12)
    b.add("lo + n = L + 1: w + 1 characters behind the record", R2[L - 12:] + b"n" * (w + 1), 2, L - 12, L - 12, OVERHANG, re=12)
    b.add("too wide: eD - bD = x + 1", b"acgt", 2, 0, x + 1, TOO_WIDE)
    b.add("too wide: eD - bD = -x - 1", b"a" * (x + 5), 2, x + 1, 0, TOO_WIDE)
    b.add("as wide as allowed: eD - bD = x", R2[:4], 2, 0, x, (0, 0, 4, "4="))
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


def band_shape_case(w, x, seed=5):
    """vc.band_shape_case's read of 40 characters (one text character deleted near the start, one inserted near the end) between
    flanks of 70 characters, the chain on the true diagonals: 2 operations when w >= 1; and with x > 0 a read whose chain drifts
    by +x and by -x over a text that does not"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"acgt", np.uint8)
    read = bytes(rng.choice(letters, 40))
    flank = bytes(rng.choice(letters, 70))
    b = Builder([flank + read[:5] + read[6:30] + b"g" + read[30:] + flank[::-1], flank + read + flank[::-1]])
    b.add("shifted and back", read, 0, 70, 70, None)
    if x:
        b.add("eD - bD = +x", read, 1, 70, 70 + x, None, re=40 - x)
        b.add("eD - bD = -x", read, 1, 70 + x, 70, None)
    return b


def tail_case(length):
    """two records, the second one without a terminator and ending at the text's last byte; the read ends there with a
    substitution in its second character and hangs one character over"""
    rng = np.random.default_rng(length)
    body = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), length - 8))
    b = Builder([b"acgtacg", body], open_end=True)
    assert len(b.text) == length and b.ends[-1] == length
    n = 24
    tail = bytearray(body[-n:])
    tail[1] = ord("n")
    at = len(body) - n
    b.add("ends at the text's last byte", bytes(tail), 1, at, at, (1, at, len(body), f"1=1X{n - 2}="))
    b.add("one character over the text's last byte", bytes(tail) + b"n", 1, at, at, (2, at, len(body), f"1=1X{n - 2}=1I"), re=n)
    return b


def random_case(seed, num_reads, C, alphabet=DNA, text_length=4096, num_records=9, max_length=60, lengths=None, max_rate=0.12,
                unused=0.1, broken=0.03, hanging=0.05, other=0.15):
    """vc.random_case's reads and slots (slot 0 of a read is its own locus, the others are loci elsewhere) and a chosen slot per
    read: mostly slot 0, `other` of them any slot, now and then no slot at all or a slot number beyond C; and `hanging` of the
    reads get a chain at a record's very start or end, so that the band of many of them leaves the record"""
    case = vc.random_case(seed, num_reads, C, alphabet, text_length, num_records, max_length, lengths, max_rate, unused, broken)
    rng = np.random.default_rng(seed + 1000)
    chosen = np.zeros(num_reads, np.uint32)
    for r in range(num_reads):
        roll = rng.random()
        if roll < other:
            chosen[r] = rng.integers(0, C)
        elif roll < other + 0.05:
            chosen[r] = NO_SLOT
        elif roll < other + 0.08:
            chosen[r] = C + int(rng.integers(0, 3))
        if rng.random() < hanging and chosen[r] < C:
            j = int(chosen[r])
            s = int(case.slots["sequences"][r, j])
            if s != NONE and s < len(case.ends):
                # an empty chain interval at read position p, put e characters from the record's start or end: a valid slot whose
                # band leaves the record when more than w + e characters of the read lie beyond p on that side
                size = int(case.ends[s]) - (0 if not s else int(case.ends[s - 1]) + 1)
                p, e = int(rng.integers(0, int(case.offsets[r + 1] - case.offsets[r]) + 1)), int(rng.integers(0, 3))
                d = e - p if rng.random() < 0.5 else size - p - e
                case.slots["chainReadBegins"][r, j] = case.slots["chainReadEnds"][r, j] = p
                case.slots["chainBeginDiagonals"][r, j] = case.slots["chainEndDiagonals"][r, j] = d
    return Case(case.read_chars.tobytes(), case.offsets, case.slots, chosen, case.text.tobytes(), case.ends, alphabet)


def planted_case(seed=7, num_reads=300, w=8):
    """reads of 30..150 characters planted in records of 400 with 3 % substitutions, 1.5 % deletions and 1.5 % insertions, one slot
    each on the true begin and end diagonals -> (case, the planted text intervals)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"acgt", np.uint8)
    records = [bytes(rng.choice(letters, 400)) for _ in range(12)]
    b = Builder(records)
    intervals = []
    for r in range(num_reads):
        s, n = int(rng.integers(0, len(records))), int(rng.integers(30, 151))
        tb = int(rng.integers(w, 400 - n - w))
        read = bytearray()
        for c in records[s][tb:tb + n]:
            roll = rng.random()
            if roll < 0.03:
                read.append(int(rng.choice([v for v in letters if v != c])))
            elif roll < 0.045:
                continue  # the text's character is deleted
            else:
                read.append(c)
            if rng.random() < 0.015:
                read.append(int(rng.choice(letters)))
        b.add(f"read {r}", bytes(read), s, tb, tb + n - len(read), None)
        intervals.append((s, tb, tb + n))
    return b.case(), intervals


def planted_inside(directory, band_pad):
    """-> (FASTA path, records, reads, planted): the records of tests/local_positions_common.py and the planted reads of
    tests/read_candidates_common.py under the first seed with which every planted locus lies at least band_pad inside its
    record"""
    import local_positions_common as lp
    import read_candidates_common as rc
    lengths = lp.record_lengths(43, count=200, longest=1500)
    records = lp.write_fasta(os.path.join(directory, "plain.fa"), lengths, lp.DNA_LETTERS, 13)
    for seed in range(21, 121):
        reads, planted = rc.planted_reads(records, seed=seed)
        if all(p is None or (p[1] >= band_pad and p[1] + rc.E2E_READ_LENGTH + 1 + band_pad <= len(records[p[0]])) for p in planted):
            break
    else:
        raise AssertionError("no seed plants every read inside its record")
    path = os.path.join(directory, "records.fa")
    with open(path, "wb") as f:
        for i, record in enumerate(records):
            f.write(b">r%d\n" % i + b"".join(record[j:j + 70] + b"\n" for j in range(0, len(record), 70)))
    return path, records, reads, planted
