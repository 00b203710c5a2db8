"""Shared by the tests of awfmVerifyChains / awfmGpuVerifyChains (include/awfm_gpu.h, "chain verification"): a plain-Python
restatement of the definition (dict-of-cells dynamic programme, exact integers, the band rule as written), an unbanded full
dynamic programme, the edge list with hand-computed values, and seeded random batches."""
import os

import numpy as np

NONE, MALFORMED, TOO_WIDE, TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NO_SLOT = 0xFFFFFFFF
MAX_LENGTH = 1 << 20
DNA, AMINO = 2, 1  # AwFmAlphabetDna, AwFmAlphabetAmino
SLOT_FIELDS = ("sequences", "chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
SLOT_DTYPES = dict(sequences=np.uint32, chainAnchors=np.uint32, chainReadBegins=np.uint32, chainReadEnds=np.uint32,
                   chainBeginDiagonals=np.int64, chainEndDiagonals=np.int64)
AMINO_LETTERS = "acdefghiklmnpqrstvwy"  # the twenty proper letters in the order of their indices
# band widths x + 2 w + 1 of the edge list as (w, x); 65 is refused
BAND_SHAPES = {1: (0, 0), 15: (7, 0), 16: (7, 1), 17: (8, 0), 31: (15, 0), 32: (15, 1), 33: (16, 0), 63: (31, 0), 64: (31, 1)}


def letter(alphabet, c):
    """the proper letter index of a character under the library's mapping, None for anything else"""
    ch = chr(c | 0x20)
    if alphabet == AMINO:
        if c == ord("$") or not (1 <= (c & 31) <= 26):
            return None
        ch = chr(96 + (c & 31))  # the mapping looks at the low five bits alone
        return AMINO_LETTERS.index(ch) if ch in AMINO_LETTERS else None
    return {"a": 0, "c": 1, "g": 2, "t": 3, "u": 3}.get(ch) if 97 <= (c | 0x20) <= 122 else None


def sub(alphabet, a, b):
    x, y = letter(alphabet, a), letter(alphabet, b)
    return 0 if x is not None and x == y else 1


def banded(R, T, w, alphabet=DNA):
    """H(n, m) by the recurrence as the header writes it: a dict of the cells in band and matrix"""
    n, m = len(R), len(T)
    delta = m - n
    lo, hi = min(0, delta) - w, max(0, delta) + w
    H = {(0, 0): 0}
    for i in range(n + 1):
        for j in range(max(0, i + lo), min(m, i + hi) + 1):
            if (i, j) == (0, 0):
                continue
            options = []
            if (i - 1, j - 1) in H:
                options.append(H[i - 1, j - 1] + sub(alphabet, R[i - 1], T[j - 1]))
            if (i - 1, j) in H:
                options.append(H[i - 1, j] + 1)
            if (i, j - 1) in H:
                options.append(H[i, j - 1] + 1)
            H[i, j] = min(options)
    return H[n, m]


def unbanded(R, T, alphabet=DNA):
    """the full edit distance under the same substitution cost"""
    row = list(range(len(T) + 1))
    for i in range(1, len(R) + 1):
        new = [i]
        for j in range(1, len(T) + 1):
            new.append(min(row[j - 1] + sub(alphabet, R[i - 1], T[j - 1]), row[j] + 1, new[j - 1] + 1))
        row = new
    return row[len(T)]


class Case:
    """one call's inputs: the read buffer, the offsets, the six slot arrays shaped (reads, C), the text and its records' ends"""

    def __init__(self, read_chars, offsets, slots, text, ends=None, alphabet=DNA, num_read_chars=None):
        self.read_chars = np.ascontiguousarray(np.frombuffer(bytes(read_chars), np.uint8))
        self.offsets = np.asarray(offsets, np.uint64)
        self.slots = {name: np.ascontiguousarray(slots[name], dtype=SLOT_DTYPES[name]) for name in SLOT_FIELDS}
        self.text = np.ascontiguousarray(np.frombuffer(bytes(text), np.uint8))
        self.ends = None if ends is None else np.asarray(ends, np.uint64)
        self.alphabet = alphabet
        self.num_read_chars = len(self.read_chars) if num_read_chars is None else num_read_chars
        self.num_reads, self.C = self.slots["sequences"].shape

    def host(self, awfm, w, x, **kw):
        return awfm.verify_chains_host(self.read_chars, self.offsets, self.slots, self.text, self.ends, self.alphabet, band_pad=w,
                                       max_drift=x, num_read_chars=self.num_read_chars, **kw)

    def intervals(self, r, j):
        """(R, T) of a slot that has a distance"""
        s = int(self.slots["sequences"][r, j])
        S = 0 if not s or self.ends is None else int(self.ends[s - 1]) + 1
        rb, re = int(self.slots["chainReadBegins"][r, j]), int(self.slots["chainReadEnds"][r, j])
        tb, te = rb + int(self.slots["chainBeginDiagonals"][r, j]), re + int(self.slots["chainEndDiagonals"][r, j])
        o = int(self.offsets[r])
        return bytes(self.read_chars[o + rb:o + re]), bytes(self.text[S + tb:S + te])

    def classify(self, r, j, x):
        """NONE .. TOO_LONG by the definition in exact integers, or None for a slot that has a distance"""
        s = int(self.slots["sequences"][r, j])
        if s == NONE or int(self.slots["chainAnchors"][r, j]) == 0:
            return NONE
        o0, o1 = int(self.offsets[r]), int(self.offsets[r + 1])
        if o0 > o1 or o1 > self.num_read_chars:
            return MALFORMED
        rb, re = int(self.slots["chainReadBegins"][r, j]), int(self.slots["chainReadEnds"][r, j])
        if rb > re or re > o1 - o0:
            return MALFORMED
        num_sequences = 1 if self.ends is None or not len(self.ends) else len(self.ends)
        if s >= num_sequences:
            return MALFORMED
        S = 0 if not s or self.ends is None else int(self.ends[s - 1]) + 1
        E = len(self.text) if self.ends is None or not len(self.ends) else int(self.ends[s])
        tb, te = rb + int(self.slots["chainBeginDiagonals"][r, j]), re + int(self.slots["chainEndDiagonals"][r, j])
        if E < S or E > len(self.text) or tb < 0 or tb > te or te > E - S:
            return MALFORMED
        if abs((te - tb) - (re - rb)) > x:
            return TOO_WIDE
        if re - rb > MAX_LENGTH:
            return TOO_LONG
        return None

    def expected(self, w, x, unverified_before=0, distance=None):
        """the whole call restated in Python; distance(R, T): the banded value (default: the dict-of-cells programme)"""
        distance = distance or (lambda R, T: banded(R, T, w, self.alphabet))
        d = np.zeros((self.num_reads, self.C), np.uint32)
        best = np.full(self.num_reads, NO_SLOT, np.uint32)
        unverified = unverified_before
        for r in range(self.num_reads):
            for j in range(self.C):
                kind = self.classify(r, j, x)
                d[r, j] = distance(*self.intervals(r, j)) if kind is None else kind
                unverified += kind in (MALFORMED, TOO_WIDE, TOO_LONG)
                if kind is None and (best[r] == NO_SLOT or d[r, j] < d[r, best[r]]):
                    best[r] = j
        return dict(editDistances=d, bestSlots=best, numUnverified=unverified)


def assert_equal(got, want, names=None, what=""):
    for name in (names or want):
        if name == "numUnverified":
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            bad = np.argwhere(got[name] != want[name])
            assert not len(bad), (what, name, bad[:5].tolist(), got[name][tuple(bad[0])], want[name][tuple(bad[0])])


class Builder:
    """a text of records (each followed by its NUL terminator unless open_end leaves the last one without) and reads with one
    slot each, added one at a time with the value the slot must get"""

    def __init__(self, records, open_end=False, alphabet=DNA):
        self.text, self.ends = bytearray(), []
        for k, record in enumerate(records):
            self.text += record
            self.ends.append(len(self.text))
            if not (open_end and k == len(records) - 1):
                self.text += b"\0"
        self.starts = [0] + [e + 1 for e in self.ends[:-1]]
        self.alphabet = alphabet
        self.reads, self.rows, self.values, self.names = [], [], [], []

    def add(self, name, read, rb, re, s, tb, te, value, anchors=1):
        """tb / te are offsets in record s; the diagonals follow"""
        self.reads.append(bytes(read))
        self.rows.append((s, anchors, rb, re, tb - rb, te - re))
        self.values.append(value)
        self.names.append(name)

    def add_raw(self, name, read, row, value):
        self.reads.append(bytes(read))
        self.rows.append(tuple(row))
        self.values.append(value)
        self.names.append(name)

    def case(self, skew=0):
        offsets = np.cumsum([skew] + [len(r) for r in self.reads])
        rows = np.array(self.rows, dtype=object)
        slots = {name: np.array([[int(v)] for v in rows[:, k]], SLOT_DTYPES[name]) for k, name in enumerate(SLOT_FIELDS)}
        return Case(b"#" * skew + b"".join(self.reads), offsets, slots, self.text, self.ends, self.alphabet)

    def want(self):
        return np.array(self.values, np.uint32).reshape(-1, 1)


BASE = b"acgtacgtac"
EDGE_RECORDS = [b"acgtacgtacgtacgt", b"", b"ccgtacgtac" + b"acgtacgtaa" + b"acgtaggtac" + b"gacgtacgtac" + b"acgtatcgtac" + b"acgtacgtacg"
                + b"cgtacgtac" + b"acgtcgtac" + b"acgtacgta", b"g", b"acgtacgtacgcagcagcagtt", b"ACGTNNacntUUtt"]
# offsets in record 2 of the variants of BASE: substitution first / last / middle, insertion first / middle / last, deletion ...
_R2 = {"sub first": (0, 10), "sub last": (10, 20), "sub middle": (20, 30), "ins first": (30, 41), "ins middle": (41, 52), "ins last": (52, 63),
       "del first": (63, 72), "del middle": (72, 81), "del last": (81, 90)}


def edge_builder(w, x):
    """the edge list for one (w, x) with w >= 2 and x >= 3: every value computed by hand"""
    b = Builder(EDGE_RECORDS)
    last = len(EDGE_RECORDS) - 1
    b.add("n = 0, m = 0", b"acgt", 2, 2, 0, 1, 1, 0)
    b.add("n = 0, m = 2", b"acgt", 4, 4, 0, 1, 3, 2)
    b.add("n = 1 equal", b"a", 0, 1, 0, 0, 1, 0)
    b.add("n = 1 different", b"a", 0, 1, 0, 1, 2, 1)
    b.add("n = 1 against nothing", b"a", 0, 1, 0, 5, 5, 1)
    b.add("tb = 0, first record, whole record", b"acgtacgtacgtacgt", 0, 16, 0, 0, 16, 0)
    for name, (tb, te) in _R2.items():
        b.add(name, BASE, 0, 10, 2, tb, te, 1)
    b.add("one-residue record", b"tgt", 1, 2, 3, 0, 1, 0)
    b.add("delta = +3", b"acgt", 0, 4, 0, 0, 7, 3)
    b.add("delta = -3", b"acgtacg", 0, 7, 0, 0, 4, 3)
    b.add("too wide: delta = +4", b"acgt", 0, 4, 0, 0, 8, 4 if x >= 4 else TOO_WIDE)
    b.add("too wide: delta = -4", b"acgtacgt", 0, 8, 0, 0, 4, 4 if x >= 4 else TOO_WIDE)
    # delete "tt", match ten, insert "tt": 4 inside a band of +-2; the Hamming distance of the tails is 12
    b.add("indel run of 2", b"acgtacgtacttgcagcagcag", 0, 22, 4, 0, 22, 4)
    b.add("upper against lower", b"acgt", 0, 4, last, 0, 4, 0)
    b.add("n against n, N against n", b"NNacnt", 0, 6, last, 4, 10, 3)
    b.add("u against t", b"tutu", 0, 4, last, 10, 14, 0)
    b.add("te = the record's length, last record", b"xxxacntuutt", 3, 11, last, 6, 14, 1)
    b.add("a single character at the read's end", b"ggggggt", 6, 7, last, 13, 14, 0)
    b.add("unused: no sequence", b"acgt", 0, 4, NONE, 0, 4, NONE)
    b.add("unused: no anchor", b"acgt", 0, 4, 0, 0, 4, NONE, anchors=0)
    b.add("malformed: sequence beyond the table", b"acgt", 0, 4, len(EDGE_RECORDS), 0, 4, MALFORMED)
    b.add("malformed: rb > re", b"acgt", 3, 2, 0, 3, 2, MALFORMED)
    b.add("malformed: re > the read's length", b"acgt", 0, 5, 0, 0, 5, MALFORMED)
    b.add("malformed: tb < 0", b"acgt", 0, 4, 0, -1, 3, MALFORMED)
    b.add("malformed: tb > te", b"acgt", 1, 1, 0, 3, 2, MALFORMED)
    b.add("malformed: te > the record's length", b"acgt", 0, 4, 0, 13, 17, MALFORMED)
    b.add("malformed: te > the empty record's length", b"a", 0, 1, 1, 0, 1, MALFORMED)
    b.add("the empty record, n = 0", b"a", 1, 1, 1, 0, 0, 0)
    for name, bD, eD in (("-2^63", -2 ** 63, -2 ** 63), ("2^63 - 1", 2 ** 63 - 1, 2 ** 63 - 1), ("a sum that would wrap to 0", 2 ** 63 - 1, 0),
                         ("begin -2^63", -2 ** 63, 0), ("end 2^63 - 1", 0, 2 ** 63 - 1), ("a begin that would wrap", -2 ** 63 + 2, 0)):
        b.add_raw("malformed: diagonals " + name, b"acgt", (0, 1, 2, 4, bD, eD), MALFORMED)
    return b


def band_shape_case(w, x, seed=5):
    """a read of 40 characters whose text has one character deleted near the start and one inserted near the end (distance 2
    when w >= 1, the Hamming distance of the two when w = 0), and with delta = +x / -x where x > 0"""
    rng = np.random.default_rng(seed)
    read = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 40))
    text = read[:5] + read[6:30] + b"g" + read[30:]
    b = Builder([text, read[:40 - x] if x else read, read + b"c" * x])
    b.add("shifted and back", read, 0, 40, 0, 0, 40, 2 if w >= 1 else sum(p != q for p, q in zip(read, text)))
    if x:
        b.add("delta = -x", read, 0, 40, 1, 0, 40 - x, x)
        b.add("delta = +x", read, 0, 40, 2, 0, 40 + x, x)
    return b


def tail_case(length):
    """two records, the second one without a terminator and ending at the text's last byte; the slot's interval ends there"""
    rng = np.random.default_rng(length)
    body = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), length - 8))
    b = Builder([b"acgtacg", body], open_end=True)
    assert len(b.text) == length and b.ends[-1] == length
    n = min(24, len(body))
    tail = bytearray(body[-n:])
    if n > 2:
        tail[1] = ord("a") if tail[1] != ord("a") else ord("c")
    b.add("ends at the text's last byte", bytes(tail), 0, n, 1, len(body) - n, len(body), 1 if n > 2 else 0)
    return b


def edit(rng, segment, rate, letters):
    """a copy of the segment with about rate * len substitutions, insertions and deletions"""
    out = bytearray()
    for c in segment:
        roll = rng.random()
        if roll < rate / 2:
            out.append(int(rng.choice(letters)))  # substitution (now and then by the same letter)
        elif roll < rate * 3 / 4:
            out.append(c)
            out.append(int(rng.choice(letters)))  # insertion
        elif roll >= rate:
            out.append(c)  # (else: deletion)
    return bytes(out)


def random_case(seed, num_reads, C, alphabet=DNA, text_length=4096, num_records=9, max_length=60, lengths=None, max_rate=0.12,
                unused=0.1, broken=0.03):
    """reads planted in a text of records (empty ones and a one-residue one among them): slot 0 of a read is its own locus, the
    others are loci elsewhere (distances up to the band's worst, too wide ones among them); some slots unused, a few malformed"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"acgtACGTn" if alphabet == DNA else (AMINO_LETTERS + AMINO_LETTERS.upper() + "xbz").encode(), np.uint8)
    cuts = np.sort(rng.choice(np.arange(1, text_length - 1), num_records - 1, replace=False))
    cuts[1] = cuts[0] + 1  # record 1 is empty, record 3 too, record 5 has one residue
    if num_records > 6:
        cuts[3], cuts[5] = cuts[2] + 1, cuts[4] + 2
    cuts = np.sort(np.unique(cuts))
    text = bytearray(rng.choice(letters[:4] if alphabet == DNA else letters[:20], text_length).tobytes())
    for cut in cuts:
        text[cut] = 0
    text[-1] = 0
    ends = np.array(list(cuts) + [text_length - 1], np.uint64)
    starts = np.concatenate(([0], ends[:-1] + 1)).astype(np.int64)
    sizes = ends.astype(np.int64) - starts
    big = np.flatnonzero(sizes >= 8)
    reads, offsets = bytearray(), [0]
    slots = {name: np.zeros((num_reads, C), SLOT_DTYPES[name]) for name in SLOT_FIELDS}
    for r in range(num_reads):
        want = int(lengths[r]) if lengths is not None else int(rng.integers(1, max_length + 1))
        s = int(rng.choice(big))
        m = min(want, int(sizes[s]))
        tb = int(rng.integers(0, sizes[s] - m + 1))
        segment = edit(rng, text[starts[s] + tb:starts[s] + tb + m], rng.random() * max_rate, letters)
        flank = bytes(rng.choice(letters, int(rng.integers(0, 4))))
        read = flank + segment + bytes(rng.choice(letters, int(rng.integers(0, 4))))
        rb, re = len(flank), len(flank) + len(segment)
        for j in range(C):
            row = (s, 1 + j, rb, re, tb - rb, tb + m - re)
            if j:  # somewhere else: another record or another place, the text interval a little longer or shorter
                s2 = int(rng.choice(big))
                m2 = max(0, min(int(sizes[s2]), re - rb + int(rng.integers(-3, 4))))
                tb2 = int(rng.integers(0, sizes[s2] - m2 + 1))
                row = (s2, 1, rb, re, tb2 - rb, tb2 + m2 - re)
            roll = rng.random()
            if roll < unused:
                row = (NONE, 0, 0, 0, 0, 0) if rng.random() < 0.5 else row[:1] + (0,) + row[2:]
            elif roll < unused + broken:
                row = [(len(ends),) + row[1:], row[:3] + (len(read) + 1,) + row[4:], row[:4] + (-rb - 1, row[5]),
                       row[:5] + (int(sizes[row[0]]) - re + 1,)][int(rng.integers(0, 4))]
            for name, value in zip(SLOT_FIELDS, row):
                slots[name][r, j] = value
        reads += read
        offsets.append(len(reads))
    return Case(bytes(reads), offsets, slots, bytes(text), ends, alphabet)


# ---- end to end: FASTA + planted reads + decoy records ----
E2E_W, E2E_X = 8, 15


def planted_with_decoys(directory):
    """-> (FASTA path, records, reads, planted, decoy_of): the records of tests/local_positions_common.py, the planted reads of
    tests/read_candidates_common.py (a substitution at every 30th character, a third of them with one deletion), and for every
    planted read that has its stretch of record to itself a decoy record appended: a copy of the read's locus with 8 more
    substitutions, in pairs at the tail of the read's four long matching stretches, so that the decoy is located by the seeds
    ahead of them and a chain over it spans them"""
    import local_positions_common as lp
    import read_candidates_common as rc
    lengths = lp.record_lengths(43, count=200, longest=1500)
    records = lp.write_fasta(os.path.join(directory, "plain.fa"), lengths, lp.DNA_LETTERS, 13)
    reads, planted = rc.planted_reads(records)
    other = {ord("a"): ord("c"), ord("c"): ord("g"), ord("g"): ord("t"), ord("t"): ord("a")}
    decoy_of = {}
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        # a decoy would also be a locus of any other read planted nearby: only reads that have their stretch of record alone
        if any(q is not None and k != r and q[0] == record and abs(q[1] - at) < 300 for k, q in enumerate(planted)):
            continue
        lo, hi = max(at - 40, 0), min(at + 161, len(records[record]))
        copy = bytearray(records[record][lo:hi])
        # at the tail of the read's matching stretches (read offsets; one further in the text behind a deleted character): the
        # windows that end ahead of them match the decoy as far as they match the locus, so the decoy is located too
        for p in (43, 44, 73, 74, 103, 104, 118, 119):
            q = at - lo + p + (1 if deleted and p >= 60 else 0)
            copy[q] = other[copy[q]]
        decoy_of[r] = len(records)
        records.append(bytes(copy))
    path = os.path.join(directory, "records.fa")
    with open(path, "wb") as f:
        for i, record in enumerate(records):
            f.write(b">r%d\n" % i + b"".join(record[j:j + 70] + b"\n" for j in range(0, len(record), 70)))
    return path, records, reads, planted, decoy_of


def text_of(records):
    """the text of a FASTA index: the records concatenated with their NUL terminators, and the records' ends in it"""
    import local_positions_common as lp
    return np.frombuffer(b"".join(record + b"\0" for record in records), np.uint8), lp.ends_of([len(record) for record in records])


def assert_planted_reads_verified(case, got, planted, decoy_of, read_length=120):
    """the best verified slot of every planted read is its record, its distance is at most the edits planted inside the chain's
    interval and equals the unbanded distance of the two intervals; the decoy's slot gets a strictly larger distance"""
    decoys_met = 0
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        best = int(got["bestSlots"][r])
        assert best != NO_SLOT and case.slots["sequences"][r, best] == record, (r, plant, got["editDistances"][r].tolist())
        rb, re = int(case.slots["chainReadBegins"][r, best]), int(case.slots["chainReadEnds"][r, best])
        edits = sum(rb <= p < re for p in range(15, read_length, 30)) + (1 if deleted and rb < 60 < re else 0)
        distance = int(got["editDistances"][r, best])
        assert distance <= edits, (r, plant, distance, edits)
        assert distance == unbanded(*case.intervals(r, best)), (r, plant)
        for j in range(case.C):
            if r in decoy_of and case.slots["sequences"][r, j] == decoy_of[r] and got["editDistances"][r, j] < TOO_LONG:
                decoys_met += 1
                assert got["editDistances"][r, j] > distance, (r, j, got["editDistances"][r].tolist())
    assert decoys_met >= len(decoy_of) // 2, (decoys_met, len(decoy_of))
