"""Shared by the longest-suffix-match tests (test_longest_match.py on the host, test_gpu_longest_match.py on the device): the
small texts, the query mixes, and two checkers that share no code with the library's batch calls -- a brute force over
sorted suffixes that knows nothing of FM indexes, and the walk over the public single-step functions, one ctypes call per
letter (include/awfm_gpu.h: the definition verbatim)."""
import bisect
import ctypes as C

import numpy as np

DNA = b"acgt"
AMINO = b"acdefghiklmnpqrstvwy"


def letters_of(amino):
    return AMINO if amino else DNA


def random_text(rng, n, letters):
    return bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), n)])


def small_texts(seed=11):
    """name -> (text, amino): random a,c,g,t; a repetitive two-letter text; one with runs of n; an amino text with a few x"""
    rng = np.random.default_rng(seed)
    plain = random_text(rng, 3000, DNA)
    repeat = b"ac" * 900 + random_text(rng, 700, b"ac") + b"ca" * 250
    runs = bytearray(random_text(rng, 3200, DNA))
    for at in rng.integers(0, 3100, 25):
        n = int(rng.integers(1, 40))
        runs[at:at + n] = b"n" * n
    amino = bytearray(random_text(rng, 3000, AMINO))
    for at in rng.integers(0, 3000, 12):
        amino[at] = ord("x")
    return {"random": (plain, False), "two-letter": (repeat, False), "n-runs": (bytes(runs[:3200]), False), "amino": (bytes(amino), True)}


def mutate(rng, piece, letters, rate):
    piece = bytearray(piece)
    for i in np.flatnonzero(rng.random(len(piece)) < rate):
        piece[i] = letters[int(rng.integers(0, len(letters)))]
    return bytes(piece)


def make_queries(rng, text, amino, count):
    """list of (query bytes, pure): pure = made of the alphabet's own letters only (either case), the brute force's domain"""
    letters = letters_of(amino)
    n = len(text)
    out = [b"", text[-1:], text[:1], text[5:6].upper(), b"n", b"x", b"b", b"z", b"N", b"j", b"o"]
    out += [bytes([c]) for c in letters] + [bytes([c]).upper() for c in letters[:3]]
    for _ in range(count):
        kind = int(rng.integers(0, 6))
        m = int(rng.integers(1, 60))
        at = int(rng.integers(0, max(n - m, 1)))
        if kind == 0:
            q = random_text(rng, m, letters)
        elif kind == 1:
            q = mutate(rng, text[at:at + m], letters, 0.05)
        elif kind == 2:
            q = text[at:at + m]  # occurs in full, unless it crosses an ambiguity letter of the text (which matches itself all the same)
        elif kind == 3:  # long: beyond the 32-character window, twice
            m = int(rng.integers(60, 150))
            at = int(rng.integers(0, max(n - m, 1)))
            q = mutate(rng, text[at:at + m], letters, 0.01)
        elif kind == 4:  # ambiguity letters, either case
            q = bytearray(mutate(rng, text[at:at + m], letters, 0.05))
            for i in np.flatnonzero(rng.random(len(q)) < 0.08):
                q[i] = ord("x") if amino else ord("n")
            q = bytes(q).upper() if rng.random() < 0.5 else bytes(q)
        else:
            q = mutate(rng, text[at:at + m], letters, 0.15).upper()
        out.append(q)
    out.append(text)                          # the whole text
    out.append(text[-40:] + text[-40:])       # ends with a suffix of the text
    out.append(random_text(rng, 8, letters) + text)  # longer than the text
    core = set(letters) | set(letters.upper())
    return [(q, all(c in core for c in q)) for q in out]


def pack(queries):
    """queries -> (chars uint8, starts uint64, ends uint64), each query followed by one byte that belongs to no query"""
    chars, starts, ends = bytearray(), [], []
    for q in queries:
        starts.append(len(chars))
        chars += q
        ends.append(len(chars))
        chars += b"#"
    return np.frombuffer(bytes(chars), np.uint8).copy(), np.array(starts, np.uint64), np.array(ends, np.uint64)


# ---- checker 1: no FM code at all ----
class BruteForce:
    """suffixes of the text sorted with the alphabet's letters in index order and everything else after them; row i of the
    sorted suffixes is BWT position i + 1 (the sentinel's row comes first)"""

    def __init__(self, text, amino):
        letters = letters_of(amino)
        table = bytearray([len(letters)] * 256)
        for i, c in enumerate(letters):
            table[c] = i
            table[c - 32] = i
        self.table = bytes(table)
        self.text = bytes(text).translate(self.table)
        order = sorted(range(len(self.text)), key=lambda i: self.text[i:])
        self.suffixes = [self.text[i:] for i in order]

    def match(self, query):
        q = bytes(query).translate(self.table)
        m = len(q)
        for length in range(m, 0, -1):  # suffixes of decreasing length against the text
            if q[m - length:] in self.text:
                pattern = q[m - length:]
                lo = bisect.bisect_left(self.suffixes, pattern)
                hi = bisect.bisect_left(self.suffixes, pattern + b"\xff")
                return length, (lo + 1, hi)
        return 0, (1, 0)

    def occurrences(self, pattern):
        p = bytes(pattern).translate(self.table)
        lo = bisect.bisect_left(self.suffixes, p)
        return bisect.bisect_left(self.suffixes, p + b"\xff") - lo


# ---- checker 2: the public step functions, one call per letter ----
def step_walk(lib, index, query):
    """lib / index: the product's (_lib.lib(), api.Index) or the reference's own (oracle.reference.lib(), its Index) -- the
    same walk over either library's range and step functions"""
    from avxwindowfmindex_amd import _lib
    amino = index.is_amino
    if hasattr(lib, "awfmNucAsciiToIndex"):
        to_index = lib.awfmAminoAsciiToIndex if amino else lib.awfmNucAsciiToIndex
    else:  # the reference's names (src/AwFmLetter.h)
        to_index = lib.awFmAsciiAminoAcidToLetterIndex if amino else lib.awFmAsciiNucleotideToLetterIndex
    to_index.restype, to_index.argtypes = C.c_uint8, [C.c_uint8]
    step = lib.awFmAminoIterativeStepBackwardSearch if amino else lib.awFmNucleotideIterativeStepBackwardSearch
    m = len(query)
    if m == 0:
        return 0, (1, 0)
    r = lib.awFmCreateInitialQueryRangeFromChar(index.ptr, query[m - 1:m])
    assert isinstance(r, _lib.AwFmSearchRange)
    kept, length = (1, 0), 0
    while r.startPtr <= r.endPtr:
        kept, length = (int(r.startPtr), int(r.endPtr)), length + 1
        if length == m:
            break
        step(index.ptr, C.byref(r), to_index(query[m - 1 - length]))
    return length, kept
