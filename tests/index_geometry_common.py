"""Small texts whose index geometry is chosen, not met by chance (tests/test_index_geometry.py on the host,
tests/test_gpu_index_geometry.py on the device).

A device block (csrc/awfm_device.h) covers 128 BWT positions in 4 slices of 32; the host library and the reference use
blocks of 256.  Two things decide whether a backward step's sp - 1 and ep meet the edges of that layout: the length L of
the BWT, i.e. where it ends relative to a block, and the row r that holds the sentinel, which is never ranked and enters
the count of the ambiguity letter as `before - acgt - (sentinelPos < before)`.  r is 1 plus the rank of the whole text among
its suffixes, in the order of longest_match_common.BruteForce: the alphabet's letters in index order, everything else
after them, and the sentinel's own suffix at row 0.

TABLE lists, per flavour, (L, seed, r): text(flavour, L, seed) is a text of L - 1 characters whose sentinel row is r.  The
seeds were found by scanning (`python tests/index_geometry_common.py` prints the table again: the scan is scan() below);
a test run does not scan, it derives L, r and the class of every entry again and asserts them, and asserts the coverage of
the list as a whole (check_coverage).  Texts, queries and classes use neither the library nor the oracle nor numpy's
generators: they come from a 64-bit linear congruential generator written out below, so they are the same everywhere.

What a batch of queries has to touch on such a text is asserted from the expected ranges by check_touches().  Only
Expected, at the end, calls the oracle and the host library: the answers both test modules compare with."""
import bisect
import itertools

import longest_match_common as lm

DEVICE_BLOCK = 128
LENGTHS = (128, 129, 256, 257, 385, 512, 513)
LOCALS = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127)  # r % 128: every slice edge of a device block from both sides
FLAVOURS = ("nucleotide", "nucleotide-n", "amino-x")
# where the sentinel's device block lies: the first block, one with blocks on both sides, the last block when that one is
# full, the last block when it is partial (L = 129, 257, 385, 513: it then holds the single row L - 1, local position 0)
BLOCK_CLASSES = ("first", "interior", "last-full", "last-partial")
# r >= 1, so local position 0 needs r >= 128: the one combination that cannot occur
IMPOSSIBLE = {(128, 0)}


class Lcg:
    """Knuth's MMIX generator, the upper 32 bits of each state"""

    def __init__(self, seed):
        self.state = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & 0xFFFFFFFFFFFFFFFF
        for _ in range(4):
            self.next()

    def next(self):
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        return self.state >> 32

    def below(self, n):
        return self.next() % n


def is_amino(flavour):
    return flavour == "amino-x"


def text(flavour, L, seed):
    """the text of L - 1 characters of this flavour and seed"""
    rng = Lcg(seed * 8 + FLAVOURS.index(flavour))
    n = L - 1
    letters = lm.letters_of(is_amino(flavour))
    out = bytearray(letters[rng.below(len(letters))] for _ in range(n))
    if flavour == "nucleotide-n":  # a few runs of n, 1 to 40 long
        for _ in range(2 + rng.below(3)):
            at, run = rng.below(n), 1 + rng.below(40)
            out[at:at + run] = b"n" * len(out[at:at + run])
    elif flavour == "amino-x":  # a few x
        for _ in range(2 + rng.below(4)):
            out[rng.below(n)] = ord("x")
    return bytes(out)


def translate_table(amino):
    letters = lm.letters_of(amino)
    table = bytearray([len(letters)] * 256)
    for i, c in enumerate(letters):
        table[c] = i
        table[c - 32] = i
    return bytes(table)


def sentinel_row(txt, amino):
    """1 + the number of proper suffixes that sort before the whole text"""
    t = txt.translate(translate_table(amino))
    return 1 + sum(1 for i in range(1, len(t)) if t[i:] < t)


def block_class(L, r):
    block, last = r // DEVICE_BLOCK, (L - 1) // DEVICE_BLOCK
    if block == last and L % DEVICE_BLOCK:
        return "last-partial"
    if block == 0:
        return "first"  # (of L = 128 the only block, first and last at once)
    return "last-full" if block == last else "interior"


class Entry:
    """one text of the table with everything derived from it"""

    def __init__(self, flavour, L, seed, r=None):
        self.flavour, self.L, self.seed = flavour, L, seed
        self.amino = is_amino(flavour)
        self.text = text(flavour, L, seed)
        assert len(self.text) == L - 1 and L in LENGTHS
        self.r = sentinel_row(self.text, self.amino)
        assert r is None or self.r == r, (flavour, L, seed, "sentinel row", self.r, "the table says", r)
        self.local = self.r % DEVICE_BLOCK
        self.block = self.r // DEVICE_BLOCK
        self.block_class = block_class(L, self.r)
        self.block_rows = (self.block * DEVICE_BLOCK, min(self.block * DEVICE_BLOCK + DEVICE_BLOCK - 1, L - 1))
        assert 1 <= self.r <= L - 1 and self.local in LOCALS and (L, self.local) not in IMPOSSIBLE
        self._queries = None

    def __repr__(self):
        return f"{self.flavour} L={self.L} seed={self.seed} r={self.r} ({self.block_class}, local {self.local})"

    def must_touch(self):
        """rows that the sp - 1 and ep of the batch's non-empty ranges have to contain"""
        rows = {self.r - 1, self.r, self.L - 1, *self.block_rows}
        if self.r + 1 <= self.L - 1:
            rows.add(self.r + 1)
        return rows

    def queries(self):
        """list of (query, pure), built once"""
        if self._queries is None:
            self._queries = make_queries(self)
        return self._queries


def make_queries(e):
    """every distinct substring of 1..8 characters; every string of 1..4 characters over the letters plus n (amino: x, every
    string of 1 or 2, and 2000 drawn strings of 3 or 4); each substring of 4..8 characters once with a wrong letter in front and
    once with one inside, so that walks die at every depth; a few in upper case; the empty query.  Every suffix of a query that
    occurs in the text is itself a query (a substring of at most 8 characters, or the whole query), so the ranges of the
    queries that occur are the ranges of every prefix a backward search passes through."""
    rng = Lcg(e.seed * 8 + 5)
    txt, n = e.text, len(e.text)
    letters = lm.letters_of(e.amino)
    wide = letters + (b"x" if e.amino else b"n")
    substrings = sorted({txt[i:i + m] for m in range(1, 9) for i in range(n - m + 1)})
    out = [b""] + substrings
    if e.amino:
        out += [bytes(p) for m in (1, 2) for p in itertools.product(wide, repeat=m)]
        out += [bytes(wide[rng.below(len(wide))] for _ in range(3 + rng.below(2))) for _ in range(2000)]
    else:
        out += [bytes(p) for m in (1, 2, 3, 4) for p in itertools.product(wide, repeat=m)]
    nine = {txt[i:i + 9] for i in range(n - 8)} | set(substrings)
    for s in substrings:
        if len(s) < 4:
            continue
        first = rng.below(len(letters))
        for k in range(len(letters)):  # a letter in front that the text never has there, if there is one
            front = letters[(first + k) % len(letters):(first + k) % len(letters) + 1] + s
            if front not in nine:
                break
        out.append(front)
        p = 1 + rng.below(len(s) - 2)  # inside: neither the first nor the last character
        others = [c for c in letters if c != s[p]]
        out.append(s[:p] + bytes([others[rng.below(len(others))]]) + s[p + 1:])
    out += [q.upper() for q in out[1::97]]
    core = set(letters) | set(letters.upper())
    return [(q, all(c in core for c in q)) for q in out]


def touched_rows(sp, ep):
    """the sp - 1 and ep of the non-empty ranges"""
    rows = set()
    for a, b in zip(sp, ep):
        a, b = int(a), int(b)
        if a <= b:
            rows.add(a - 1)
            rows.add(b)
    return rows


def check_touches(e, sp, ep):
    """a condition on the inputs: the expected ranges of the entry's queries meet the sentinel row from both sides, both ends of
    its device block, and the end of the BWT"""
    missing = e.must_touch() - touched_rows(sp, ep)
    assert not missing, (e, "no expected range has its sp - 1 or ep at rows", sorted(missing))


class Suffixes:
    """sorted suffixes with the ambiguity letter as one more letter behind the alphabet's: the ranges of any query in plain
    Python, for the scan (the tests take their ranges from the oracle and from BruteForce)"""

    def __init__(self, txt, amino):
        self.table = translate_table(amino)
        t = txt.translate(self.table)
        self.suffixes = sorted(t[i:] for i in range(len(t)))

    def range(self, query):
        q = query.translate(self.table)
        lo = bisect.bisect_left(self.suffixes, q)
        return lo + 1, bisect.bisect_left(self.suffixes, q + b"\xff")


def touches_by_plain_sorting(e):
    s = Suffixes(e.text, e.amino)
    ranges = [s.range(q) for q, _ in e.queries() if q]
    return not (e.must_touch() - touched_rows([a for a, _ in ranges], [b for _, b in ranges]))


def targets():
    """(L, local, block class) wanted of every flavour: each local position twice, at two lengths and in two block classes
    taken in rotation from the ones that length allows; then the last partial block of every length that has one"""
    out = []
    for i, local in enumerate(LOCALS):
        for j in range(2):
            k = 2 * i + j
            while True:
                L = LENGTHS[k % len(LENGTHS)]
                rows = [b * DEVICE_BLOCK + local for b in range((L - 1) // DEVICE_BLOCK + 1) if 1 <= b * DEVICE_BLOCK + local <= L - 1]
                classes = sorted({block_class(L, r) for r in rows} - {"last-partial"})
                if classes and not any((L, local) == t[:2] for t in out):
                    break
                k += 1
            out.append((L, local, classes[(i + j) % len(classes)]))
    out += [(L, 0, "last-partial") for L in LENGTHS if L % DEVICE_BLOCK]
    return out


def scan(flavour, limit=200000):
    """the first seed of every target whose text has that geometry and whose queries touch it"""
    found = []
    for L, local, wanted in targets():
        amino = is_amino(flavour)
        for seed in range(limit):
            r = sentinel_row(text(flavour, L, seed), amino)
            if r % DEVICE_BLOCK != local or block_class(L, r) != wanted or (L, seed, r) in found:
                continue
            if touches_by_plain_sorting(Entry(flavour, L, seed, r)):
                found.append((L, seed, r))
                break
        else:
            raise AssertionError((flavour, L, local, wanted, "no seed below", limit))
    return found


# flavour -> [(L, seed, r)]
TABLE = {
    "nucleotide": [
        (256, 504, 128), (257, 48, 128), (256, 191, 129), (257, 14, 1), (385, 261, 31), (512, 280, 31),
        (513, 50, 160), (128, 28, 32), (129, 298, 33), (256, 162, 161), (257, 102, 191), (385, 105, 63),
        (512, 232, 64), (513, 120, 448), (128, 65, 65), (129, 65, 65), (256, 125, 95), (257, 118, 223),
        (385, 412, 224), (512, 173, 224), (513, 326, 97), (128, 338, 97), (129, 101, 127), (256, 48, 127),
        (129, 42, 128), (257, 42, 256), (385, 42, 384), (513, 836, 512),
    ],
    "nucleotide-n": [
        (256, 822, 128), (257, 6872, 128), (256, 244, 129), (257, 220, 1), (385, 393, 31), (512, 190, 31),
        (513, 179, 288), (128, 39, 32), (129, 6745, 33), (256, 263, 161), (257, 11339, 191), (385, 31, 63),
        (512, 345, 64), (513, 36, 192), (128, 43, 65), (129, 7327, 65), (256, 175, 95), (257, 3117, 223),
        (385, 679, 224), (512, 385, 352), (513, 33, 97), (128, 1294, 97), (129, 41361, 127), (256, 23, 127),
        (129, 4923, 128), (257, 24514, 256), (385, 15804, 384), (513, 52403, 512),
    ],
    "amino-x": [
        (256, 107, 128), (257, 236, 128), (256, 236, 129), (257, 487, 1), (385, 1148, 31), (512, 1960, 31),
        (513, 56, 160), (128, 73, 32), (129, 74, 33), (256, 162, 161), (257, 401, 191), (385, 611, 63),
        (512, 465, 64), (513, 18, 192), (128, 33, 65), (129, 33, 65), (256, 168, 95), (257, 507, 223),
        (385, 46, 352), (512, 123, 352), (513, 114, 97), (128, 67, 97), (129, 394, 127), (256, 752, 127),
        (129, 77, 128), (257, 230, 256), (385, 1223, 384), (513, 828, 512),
    ],
}


def check_coverage(table):
    """what the list as a whole has to cover; a list shortened by a class fails here, on the CPU"""
    for flavour in FLAVOURS:
        entries = [Entry(flavour, *row) for row in table[flavour]]
        assert len({(e.L, e.seed) for e in entries}) == len(entries), (flavour, "a text is listed twice")
        for local in LOCALS:
            full = [e for e in entries if e.local == local and e.block_class != "last-partial"]
            assert len([e for e in entries if e.local == local]) >= 2 and full, (flavour, "local position", local)
        # the last partial block holds row L - 1 alone: local position 0 is the only one that can occur in it
        for L in LENGTHS:
            assert len([e for e in entries if e.L == L]) >= 2, (flavour, "L", L)
            if L % DEVICE_BLOCK:
                assert any(e.L == L and e.block_class == "last-partial" and e.local == 0 for e in entries), (flavour, "partial", L)
        for name in BLOCK_CLASSES:
            assert any(e.block_class == name for e in entries), (flavour, name)
        assert any(e.L == 128 for e in entries if e.block_class == "first"), (flavour, "the only block of L = 128")
    return True


_entries = {}


def entries(flavour):
    """the flavour's texts, derived and asserted once"""
    if flavour not in _entries:
        _entries[flavour] = [Entry(flavour, *row) for row in TABLE[flavour]]
    return _entries[flavour]


# ---- what the tests expect of a text: computed once per text, shared by both modules, left unchanged ----
RATIOS = (1, 3, 8, 255)
_expected = {}


def seed_k_of(e):
    """{1, 4} for nucleotide, {1, 2} for amino, alternating over the flavour's texts"""
    odd = entries(e.flavour).index(e) % 2
    return (1, 2)[odd] if e.amino else (1, 4)[odd]


def brute_suffix_array(e):
    """text position of every BWT row, from a plain sort: row 0 is the sentinel's own suffix"""
    t = e.text.translate(translate_table(e.amino))
    n = len(t)
    return [n] + sorted(range(n), key=lambda i: t[i:])


class Expected:
    """index, packed batch, and the answers of the oracle and of the host twins for one text (tests/test_index_geometry.py pins
    them to the brute force, the step walks and the compiled reference)"""

    def __init__(self, awfm, oracle, e):
        import numpy as np
        import one_substitution_common as osc
        self.entry = e
        self.alphabet = 1 if e.amino else 2
        assert (awfm.AwFmAlphabetAmino, awfm.AwFmAlphabetDna) == (1, 2)
        self.seed_k = seed_k_of(e)
        self.ratio = RATIOS[entries(e.flavour).index(e) % len(RATIOS)]
        self.queries = [q for q, _ in e.queries()]
        self.pure = np.array([pure for _, pure in e.queries()])
        self.chars, self.offsets = osc.pack(self.queries)
        self.starts, self.ends = self.offsets[:-1].copy(), self.offsets[1:].copy()
        self.oracle_index = oracle.Index.from_text(e.text, self.alphabet, self.ratio, self.seed_k)
        self.sp, self.ep, self.count, _ = self.oracle_index.batch_search(self.chars, self.offsets)
        self.hit_offsets, self.positions, _ = self.oracle_index.batch_locate(self.sp, self.ep)
        self.index = awfm.create_index(e.text, self.alphabet, self.ratio, self.seed_k)
        assert self.index.bwt_length == self.oracle_index.bwt_length == e.L
        self.longest = {m: awfm.longest_suffix_matches_host(self.index, self.chars, self.starts, self.ends, min_length=m) for m in (0, 3)}
        self.one_substitution = {x: awfm.one_substitution_search_host(self.index, self.chars, self.offsets, include_exact=x)
                                 for x in (True, False)}
        self.suffix_array = np.array(brute_suffix_array(e), np.uint64)
        assert int(self.suffix_array[e.r]) == 0  # the sentinel row is the row of the whole text
        check_touches(e, self.sp, self.ep)


def walks_that_end_on_the_sentinel(x, ratio):
    """rows whose locate walk steps onto the sentinel's row, having met no sampled row (every ratio-th row) before it"""
    e = x.entry
    import numpy as np
    row_of = np.empty(e.L, np.int64)
    row_of[x.suffix_array.astype(np.int64)] = np.arange(e.L)
    assert int(row_of[0]) == e.r
    rows = []
    for position in range(1, e.L):
        if row_of[position] % ratio == 0:
            break
        rows.append(int(row_of[position]))
    return rows


def expected(awfm, oracle, e):
    key = (e.flavour, e.L, e.seed)
    if key not in _expected:
        _expected[key] = Expected(awfm, oracle, e)
    return _expected[key]


if __name__ == "__main__":
    print("TABLE = {")
    for name in FLAVOURS:
        rows = scan(name)
        print(f'    "{name}": [')
        for at in range(0, len(rows), 6):
            print("        " + ", ".join(str(row) for row in rows[at:at + 6]) + ",")
        print("    ],")
    print("}")
else:
    check_coverage(TABLE)
