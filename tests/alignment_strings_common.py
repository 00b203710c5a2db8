"""What the tests of "alignment strings" (include/awfm_gpu.h) share: a batch builder, and a plain-Python restatement of the
definition -- the CIGAR in both forms and the MD:Z string of a read from its row of runs and the text, which reads are NONE or
SKIPPED, the packing behind offsets and what a capacity leaves out -- written from the header's rules and from nothing of the
library's code, so that the host twin is not the only witness of the device call."""
import numpy as np

I, D, S, EQ, X = 1, 2, 4, 7, 8  # BAM numbering of the operations
LETTERS = {I: b"I", D: b"D", S: b"S", EQ: b"=", X: b"X"}
MAX_LENGTH = 1 << 16  # AWFM_ALIGN_MAX_LENGTH
MAX_OPS = 4096  # AWFM_ALIGN_MAX_OPS
NO_SLOT = 0xFFFFFFFF  # AWFM_CHAINS_NO_SLOT
DNA, AMINO = 2, 1  # AwFmAlphabetDna, AwFmAlphabetAmino (asserted against the api by the tests)
NULL_ERROR, ILLEGAL, UNSUPPORTED = -4, -6, -2  # AwFmNullPtrError, AwFmIllegalPositionError, AwFmUnsupportedVersionError (include/AwFmIndex.h)


def letter_table(alphabet):
    """letter(c) of all 256 byte values: a..z raised, A..Z kept, the rest N (nucleotide) or X (amino)"""
    other = ord("X") if alphabet == AMINO else ord("N")
    return bytes(c - 32 if 97 <= c <= 122 else c if 65 <= c <= 90 else other for c in range(256))


class Read:
    """one read of a batch: the record its slot names, where its text begins in it, its runs [(len, op), ...] -- and what a test
    may bend: the slot number, the sequence number as stored, numOps as stored, raw words in place of the runs"""

    def __init__(self, record=0, begin=0, runs=(), slot=0, num_ops=None, sequence=None, words=None):
        self.record, self.begin, self.runs, self.slot = record, begin, list(runs), slot
        self.words = [(length << 4) | op for length, op in self.runs] if words is None else list(words)
        self.num_ops = len(self.words) if num_ops is None else num_ops
        self.sequence = record if sequence is None else sequence


def script(text):
    """'2S 3= 1X' -> [(2, S), (3, EQ), (1, X)]"""
    ops = {"I": I, "D": D, "S": S, "=": EQ, "X": X}
    return [(int(token[:-1]), ops[token[-1]]) for token in text.split()]


class Case:
    """a batch as the alignment calls leave it: sequences (n, C), slots, textBegins, numOps (n,), ops (n, max_ops); rows are filled
    with `pad` beyond what a read stores (the alignment calls leave those words unwritten)"""

    def __init__(self, reads, text, ends=None, alphabet=DNA, C=2, max_ops=8, pad=0xDEADBEEF):
        n = len(reads)
        self.reads, self.alphabet, self.C, self.max_ops, self.num_reads = reads, alphabet, C, max_ops, n
        self.text = np.frombuffer(bytes(text), np.uint8).copy()
        self.ends = None if ends is None else np.asarray(ends, np.uint64)
        self.sequences = np.full((n, C), 0xFFFFFFFE, np.uint32)  # (slots nobody names hold a sequence that does not exist)
        self.slots = np.zeros(n, np.uint32)
        self.text_begins = np.zeros(n, np.uint64)
        self.num_ops = np.zeros(n, np.uint32)
        self.ops = np.full((n, max_ops), pad, np.uint32)
        for r, read in enumerate(reads):
            self.slots[r] = read.slot
            if read.slot < C:
                self.sequences[r, read.slot] = read.sequence
            self.text_begins[r] = read.begin
            self.num_ops[r] = read.num_ops
            stored = read.words[:max_ops]
            self.ops[r, :len(stored)] = stored

    def arrays(self):
        return dict(sequences=self.sequences, slots=self.slots, text_begins=self.text_begins, num_ops=self.num_ops, ops=self.ops)

    def record_bounds(self, s):
        """[S, E) of record s, or None when the table gives it no place inside the text"""
        if self.ends is None or self.ends.size == 0:
            return (0, len(self.text)) if s == 0 else None
        if s >= self.ends.size:
            return None
        begin, end = (int(self.ends[s - 1]) + 1 if s else 0), int(self.ends[s])
        return (begin, end) if begin <= end <= len(self.text) else None


def decimal(value):
    return str(value).encode()


def read_strings(case, r, classic):
    """the restatement, per read: None (NONE), "skipped", or (cigar, md) as bytes"""
    k, j = int(case.num_ops[r]), int(case.slots[r])
    if k == 0:
        return None
    if k > case.max_ops or j >= case.C:
        return "skipped"
    bounds = case.record_bounds(int(case.sequences[r, j]))
    if bounds is None:
        return "skipped"
    runs = [(int(w) >> 4, int(w) & 15) for w in case.ops[r, :k]]
    if any(length == 0 or op not in LETTERS for length, op in runs):
        return "skipped"
    read_length = sum(length for length, op in runs if op in (I, S, EQ, X))
    text_length = sum(length for length, op in runs if op in (EQ, X, D))
    L, begin = bounds[1] - bounds[0], int(case.text_begins[r])
    if read_length > MAX_LENGTH or text_length > 2 * MAX_LENGTH or begin > L or text_length > L - begin:
        return "skipped"
    cigar, merged = [], 0
    for i, (length, op) in enumerate(runs):
        if classic and op in (EQ, X):
            merged += length
            if i + 1 == len(runs) or runs[i + 1][1] not in (EQ, X):
                cigar.append(decimal(merged) + b"M")
                merged = 0
        else:
            cigar.append(decimal(length) + LETTERS[op])
    table, text = letter_table(case.alphabet), case.text.tobytes()
    md, p, m = [], bounds[0] + begin, 0
    for length, op in runs:
        if op == EQ:
            m += length
            p += length
        elif op == X:
            letters = text[p:p + length].translate(table)
            md.append(decimal(m) + letters[:1] + b"".join(b"0" + letters[i:i + 1] for i in range(1, length)))
            m = 0
            p += length
        elif op == D:
            md.append(decimal(m) + b"^" + text[p:p + length].translate(table))
            m = 0
            p += length
    md.append(decimal(m))
    return b"".join(cigar), b"".join(md)


def expected(case, classic=False, cigar_capacity=None, md_capacity=None, fill=0, skipped_before=0, overflow_before=0,
             cigar_arena=True, md_arena=True):
    """the restatement, per batch: cigarOffsets, mdOffsets, cigarChars, mdChars (arenas of the capacities, `fill` where nothing
    is written; None: exactly the total), numSkipped, numOverflow, and the strings themselves"""
    per_read = [read_strings(case, r, classic) for r in range(case.num_reads)]
    strings = [s if isinstance(s, tuple) else (b"", b"") for s in per_read]
    result = {"numSkipped": skipped_before + sum(s == "skipped" for s in per_read), "strings": strings}
    missed = np.zeros(case.num_reads, bool)
    for which, name, capacity, wanted in ((0, "cigar", cigar_capacity, cigar_arena), (1, "md", md_capacity, md_arena)):
        offsets = np.zeros(case.num_reads + 1, np.uint64)
        offsets[1:] = np.cumsum([len(s[which]) for s in strings], dtype=np.uint64)
        capacity = int(offsets[-1]) if capacity is None else capacity
        arena = np.full(capacity, fill, np.uint8)
        for r, s in enumerate(strings):
            if not s[which] or not wanted:
                continue
            if int(offsets[r + 1]) <= capacity:
                arena[int(offsets[r]):int(offsets[r + 1])] = np.frombuffer(s[which], np.uint8)
            else:
                missed[r] = True
        result[name + "Offsets"], result[name + "Chars"] = offsets, arena
    result["numOverflow"] = overflow_before + int(missed.sum())
    return result


def assert_same(got, want, names=("cigarOffsets", "cigarChars", "mdOffsets", "mdChars", "numSkipped", "numOverflow"), what=""):
    for name in names:
        if name in ("numSkipped", "numOverflow"):
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            a, b = np.asarray(got[name]), np.asarray(want[name])
            assert a.shape == b.shape, (what, name, a.shape, b.shape)
            if not np.array_equal(a, b):
                at = int(np.flatnonzero(a != b)[0])
                raise AssertionError((what, name, "first difference at", at, a[max(at - 8, 0):at + 8].tolist(), b[max(at - 8, 0):at + 8].tolist()))


# ---- the hand values of the definition ------------------------------------------------------------------------------------------
# (record text, textBegin, script, extended CIGAR, classic CIGAR, MD)
HAND = (
    (b"ACGTACGTAC", 1, "2S 3= 1X 2I 1D 2=", b"2S3=1X2I1D2=", b"2S4M2I1D2M", b"3A0^C2"),
    (b"TTGGGGG", 0, "2X 5=", b"2X5=", b"7M", b"0T0T5"),
    (b"AAAAAg", 0, "5= 1X", b"5=1X", b"6M", b"5G0"),
    (b"AAAAAAAAAA", 0, "9= 1I 1=", b"9=1I1=", b"9M1I1M", b"10"),
    (b"a\x00C", 0, "1D 1X 1=", b"1D1X1=", b"1D2M", b"0^A0N1"),
    (b"ACGTACGT", 0, "3= 2D 1I 2D 1=", b"3=2D1I2D1=", b"3M2D1I2D1M", b"3^TA0^CG1"),
)


def records_of(texts, separator=b"$"):
    """the concatenated text of some records, one separator after each, and their ends (separators excluded)"""
    text, ends = b"", []
    for t in texts:
        text += t
        ends.append(len(text))
        text += separator
    return text, np.asarray(ends, np.uint64)


def hand_case(C=2, max_ops=8):
    text, ends = records_of([h[0] for h in HAND])
    reads = [Read(record=s, begin=h[1], runs=script(h[2]), slot=s % C) for s, h in enumerate(HAND)]
    return Case(reads, text, ends, DNA, C=C, max_ops=max_ops)


# ---- edge lists -----------------------------------------------------------------------------------------------------------------
DECIMAL_EDGES = (9, 10, 99, 100, 999, 1000, 9999, 10000, 65535, 65536, 99999, 100000, 1 << 17)


def random_text(rng, length, alphabet, rich=0.25):
    """letters of the alphabet in both cases, a share `rich` of the bytes any value at all"""
    letters = np.frombuffer(b"acgtACGTnN" if alphabet == DNA else b"acdefghiklmnpqrstvwyACDEFGHIKLMNPQRSTVWYxX", np.uint8)
    text = letters[rng.integers(0, letters.size, length)]
    any_value = rng.random(length) < rich
    text[any_value] = rng.integers(0, 256, int(any_value.sum()), dtype=np.uint8)
    return text


def edge_case(alphabet=DNA, max_ops=12):
    """run lengths at every decimal edge, as '=', 'X', 'D', 'I', 'S' and classic M runs; m reaching the edges across '=' runs that
    an I separates; scripts that begin and end with X, D and S; classic merging and what stops it"""
    rng = np.random.default_rng(20 + alphabet)
    length = 1 << 19
    text = random_text(rng, length, alphabet)
    ends = np.asarray([length // 2 - 1, length - 7, length], np.uint64)  # three records; the last has 6 characters
    reads = []
    for edge in DECIMAL_EDGES:
        if edge <= MAX_LENGTH:
            reads.append(Read(0, 5, [(edge, EQ)]))
            reads.append(Read(0, 3, [(edge, X)] if edge <= 10000 else [(edge - 1, EQ), (1, X)]))
            reads.append(Read(1, 1, [(1, S), (edge - 1, I)] if edge > 1 else [(1, S)]))
            reads.append(Read(0, 0, [(edge - 1, S), (1, EQ)]))
            rest = edge - edge // 2 - (1 if edge == MAX_LENGTH else 0)  # (the I is a read character too)
            reads.append(Read(0, 2, [(edge // 2, EQ), (1, I), (rest, EQ)]))  # m reaches the edge by accumulation
            reads.append(Read(0, 2, [(edge // 2, EQ), (edge - edge // 2, X), (3, EQ)] if edge <= 2000 else [(edge - 1, EQ), (1, X)]))
        else:  # only a text length reaches it: '=' and D together, or D alone
            reads.append(Read(0, 7, [(MAX_LENGTH, EQ), (edge - MAX_LENGTH, D)]))
            reads.append(Read(1, 0, [(edge, D)]))
        reads.append(Read(1, 4, [(2, EQ), (edge if edge + 4 <= 2 * MAX_LENGTH else edge - 4, D), (2, EQ)]))
        reads.append(Read(0, 1, [(min(edge, MAX_LENGTH) // 3, EQ), (1, D), (1, I), (min(edge, MAX_LENGTH) // 3, EQ)]))
    for first in (X, D, S):
        for last in (X, D, S):
            reads.append(Read(1, 9, [(2, first), (4, EQ), (3, last)]))
            reads.append(Read(1, 9, [(1, first), (1, last)]))
    reads += [Read(0, 11, script("3= 2X 4=")), Read(0, 11, script("3= 1I 2X 1D 4= 1S")), Read(0, 11, script("1X 1= 1X 1= 1X")),
              Read(0, 11, script("2= 2= 1X 1X 1I 1I 3= 1D 1D 2X")), Read(2, 0, script("6=")), Read(2, 5, script("1X")),
              Read(2, 6, script("1S")), Read(2, 0, script("3X 3D"))]
    return Case(reads, text, ends, alphabet, C=3, max_ops=max_ops)


def text_under(case, r):
    """the global text positions the script of read r covers from its textBegin on, whether the read is valid or not, cut to the
    text: range(begin, end), or None where the row, the slot or the record do not say (truncated rows count their stored runs)"""
    j, k = int(case.slots[r]), min(int(case.num_ops[r]), case.max_ops)
    if k == 0 or j >= case.C:
        return None
    bounds = case.record_bounds(int(case.sequences[r, j]))
    if bounds is None:
        return None
    length = sum(int(w) >> 4 for w in case.ops[r, :k] if int(w) & 15 in (EQ, X, D))
    begin = bounds[0] + int(case.text_begins[r])
    return range(min(begin, len(case.text)), min(begin + length, len(case.text)))


def skipped_case(alphabet=DNA, max_ops=8, C=3):
    """every SKIPPED condition in turn, each between two reads that are fine -> (case, the numbers of the reads that are skipped).
    The skipped reads that have a place in the text lie at position 1000 of the long record, where no valid read lies, or past a
    record's end (there they would read its separator, the byte at ends[s]: valid reads never do)"""
    rng = np.random.default_rng(30 + alphabet)
    text, ends = records_of([bytes(random_text(rng, n, alphabet, rich=0.1)) for n in (40, 1 << 18, 25)])
    fine = lambda: Read(1, 7, script("2S 3= 1X 2D 4= 1I 1="))  # noqa: E731
    L1, L2 = 1 << 18, 25
    bad = [
        Read(1, 1000, script("3= 1X 2=") * 3, num_ops=9),                      # k > maxOps: a truncated row
        Read(1, 1000, script("3= 1X"), slot=C),                                # j >= C
        Read(1, 1000, script("3= 1X"), slot=NO_SLOT),                          # AWFM_CHAINS_NO_SLOT
        Read(1, 1000, script("3= 1X"), sequence=3),                            # s >= numRecords
        Read(1, 1000, script("3= 1X"), sequence=0xFFFFFFFF),
        Read(1, 1000, words=[3 << 4 | EQ, 0 << 4 | X, 2 << 4 | EQ]),           # a run without a length
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 0, 2 << 4 | EQ]),           # operations outside the five: M, N, H, P, 9..15
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 3]),
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 5]),
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 6]),
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 9]),
        Read(1, 1000, words=[3 << 4 | EQ, 1 << 4 | 15]),
        Read(1, 0, [(MAX_LENGTH, EQ), (1, I)]),                             # read length 2^16 + 1
        Read(1, 0, [(MAX_LENGTH - 1, S), (1, X), (1, S)]),
        Read(1, 0, [(MAX_LENGTH, EQ), (MAX_LENGTH, D), (1, D)]),            # text length 2^17 + 1
        Read(1, 0, [((1 << 28) - 1, EQ)] * 6),                              # sums beyond 32 bits
        Read(1, L1 + 1, script("1S")),                                      # textBegin > L
        Read(1, L1 - 5, script("3= 3X")),                                   # one position past the record's end
        Read(2, L2 - 2, script("1= 2D")),                                   # ... of the last record
        Read(0, 38, script("2= 1D")),                                       # ... of the first
        Read(1, (1 << 64) - 1, script("1=")),                               # textBegin near 2^64
        Read(1, (1 << 64) - 3, script("2= 2X")),
        Read(2, (1 << 63) + 5, script("1X")),
    ]
    valid_at_the_end = [Read(1, L1 - 6, script("3= 3X")), Read(2, L2 - 3, script("1= 2D")), Read(0, 37, script("2= 1D")), Read(0, 40, script("2S")),
                        Read(2, L2, script("1I"))]
    reads, skipped = [fine()], []
    for read in bad:
        skipped.append(len(reads))
        reads += [read, fine()]
    reads += valid_at_the_end + [Read(num_ops=0, slot=NO_SLOT, begin=(1 << 64) - 1), fine()]  # (and one that is NONE)
    return Case(reads, text, ends, alphabet, C=C, max_ops=max_ops), skipped


def random_case(seed, num_reads, alphabet=DNA, C=4, max_ops=32, text_length=1 << 14, num_records=5, none=0.08, skipped=0.05, max_runs=None,
                max_run=40, like=None):
    """random valid scripts over a byte-rich text with a record table (like: another case's), a share of the reads NONE and SKIPPED"""
    rng = np.random.default_rng(seed)
    if like is None:
        text = random_text(rng, text_length, alphabet)
        cuts = np.sort(rng.choice(np.arange(200, text_length - 200), num_records - 1, replace=False)) if num_records > 1 else np.zeros(0, np.int64)
        ends = np.concatenate((cuts, [text_length])).astype(np.uint64)
    else:
        text, ends, num_records = like.text, like.ends, like.ends.size
        cuts = ends[:-1].astype(np.int64)
    begins = np.concatenate(([0], cuts + 1))
    max_runs = max_ops if max_runs is None else min(max_runs, max_ops)
    reads = []
    for r in range(num_reads):
        u = rng.random()
        if u < none:
            reads.append(Read(num_ops=0, slot=int(rng.integers(0, C)) if rng.random() < 0.5 else NO_SLOT, record=int(rng.integers(0, num_records))))
            continue
        s = int(rng.integers(0, num_records))
        L = int(ends[s]) - int(begins[s])
        k = int(rng.integers(1, max_runs + 1))
        ops = rng.choice([EQ, EQ, EQ, X, X, I, D, S], k)
        lengths = np.where(rng.random(k) < 0.7, rng.integers(1, 4, k), rng.integers(1, max_run + 1, k))
        runs = [(int(n), int(op)) for n, op in zip(lengths, ops)]
        while sum(n for n, op in runs if op in (EQ, X, D)) > L:
            runs.pop()
        if not runs:
            runs = [(1, S)]
        text_len = sum(n for n, op in runs if op in (EQ, X, D))
        begin = int(rng.integers(0, L - text_len + 1))
        slot = int(rng.integers(0, C))
        if u < none + skipped:
            kind = int(rng.integers(0, 4))
            bent = [dict(slot=NO_SLOT), dict(sequence=num_records + int(rng.integers(0, 3))), dict(begin=L + 1 + int(rng.integers(0, 9))),
                    dict(words=[(n << 4) | op for n, op in runs[:-1]] + [int(rng.integers(0, 9)) << 4 | 3])][kind]
            reads.append(Read(**{**dict(record=s, begin=begin, runs=runs, slot=slot), **bent}))
        else:
            reads.append(Read(s, begin, runs, slot))
    return Case(reads, text, ends, alphabet, C=C, max_ops=max_ops)
