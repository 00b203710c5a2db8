"""Which letter is this byte?  The definition once, in plain Python, for the tests that send every byte value through every
kernel that reads letters (tests/test_byte_values.py on the CPU, tests/test_gpu_byte_values.py on the device).

The five tables below are written from the statement of the mapping (ref src/AwFmLetter.c, include/awfm_gpu.h), not read from
the library: tests/test_byte_values.py holds the host library, the oracle and -- where it is built -- the reference to them on
all 256 values.

    nucleotide   a A -> 0, c C -> 1, g G -> 2, t T u U -> 3, '$' and 0x04 (whose | 0x20 is '$') -> 5, the other 244 -> 4
    amino        '$' -> 21; otherwise the low five bits alone: 1 .. 26 name a .. z, the twenty proper letters get 0 .. 19 in
                 the order acdefghiklmnpqrstvwy, everything else 20 (b j o u x z, and 0, 27 .. 31)
    ambiguous    nucleotide: everything but a c g t u in either case; amino: b x z in either case -- six bytes out of the 96
                 of index 20: the other 90 are no letters, and the reference still takes them through its k-mer table

A CLASS is the set of bytes with one (letter index, ambiguous?): the unit of "must behave the same".  The SENTINEL CLASS
('$' and 0x04, '$') is kept out of every query that walks an index -- a backward step with the sentinel's letter index is not
defined by the reference -- and appears in the reads and texts of the alignment kernels only, where it is just no proper letter.
"""
import numpy as np

DNA, AMINO = 2, 1  # AwFmAlphabetDna, AwFmAlphabetAmino
AMINO_LETTERS = "acdefghiklmnpqrstvwy"  # the twenty proper letters in the order of their indices
NUC_AMBIGUITY, NUC_SENTINEL, AMINO_AMBIGUITY, AMINO_SENTINEL = 4, 5, 20, 21


def _tables():
    nuc = [NUC_AMBIGUITY] * 256
    for index, letters in enumerate(("aA", "cC", "gG", "tTuU")):
        for ch in letters:
            nuc[ord(ch)] = index
    nuc[ord("$")] = nuc[0x04] = NUC_SENTINEL
    amino = [AMINO_AMBIGUITY] * 256
    for c in range(256):
        low = c & 31
        if 1 <= low <= 26 and chr(96 + low) in AMINO_LETTERS:
            amino[c] = AMINO_LETTERS.index(chr(96 + low))
    amino[ord("$")] = AMINO_SENTINEL
    # the sanitisers (what a text's byte is stored as): nucleotide lowers the case of a c g t u and of the sentinel class and turns
    # the rest into x; amino turns b, x (either case) and NUL into z and keeps EVERY other byte as it is
    nuc_clean = [ord("x") if nuc[c] == NUC_AMBIGUITY else c | 0x20 for c in range(256)]
    amino_clean = [ord("z") if c in (0, ord("b"), ord("B"), ord("x"), ord("X")) else c for c in range(256)]
    nuc_ambiguous = [c not in b"acgtuACGTU" for c in range(256)]
    amino_ambiguous = [c in b"bxzBXZ" for c in range(256)]
    return (np.array(nuc, np.uint8), np.array(amino, np.uint8), np.array(nuc_clean, np.uint8), np.array(amino_clean, np.uint8),
            {DNA: np.array(nuc_ambiguous, bool), AMINO: np.array(amino_ambiguous, bool)})


NUC_INDEX, AMINO_INDEX, NUC_SANITIZED, AMINO_SANITIZED, AMBIGUOUS = _tables()
INDEX = {DNA: NUC_INDEX, AMINO: AMINO_INDEX}
SANITIZED = {DNA: NUC_SANITIZED, AMINO: AMINO_SANITIZED}
CARDINALITY = {DNA: 4, AMINO: 20}
SENTINEL_INDEX = {DNA: NUC_SENTINEL, AMINO: AMINO_SENTINEL}
# the counts of the statement, so that a slip in _tables cannot pass for the definition
assert [int((NUC_INDEX == k).sum()) for k in range(6)] == [2, 2, 2, 4, 244, 2]
assert int((AMINO_INDEX < 20).sum()) == 159 and int((AMINO_INDEX == 20).sum()) == 96 and int((AMINO_INDEX == 21).sum()) == 1
assert [int((AMINO_INDEX == k).sum()) for k in range(20)] == [8, 8, 7] + [8] * 17
assert int(AMBIGUOUS[AMINO].sum()) == 6 and int(AMBIGUOUS[DNA].sum()) == 246


def classes(alphabet, _made={}):
    """{(letter index, ambiguous?): the bytes of that class, ascending}"""
    if alphabet not in _made:
        out = {}
        for c in range(256):
            out.setdefault((int(INDEX[alphabet][c]), bool(AMBIGUOUS[alphabet][c])), []).append(c)
        _made[alphabet] = out
    return {key: list(members) for key, members in _made[alphabet].items()}


def class_of(alphabet, c):
    return int(INDEX[alphabet][c]), bool(AMBIGUOUS[alphabet][c])


def sentinel_class(alphabet):
    return [c for c in range(256) if INDEX[alphabet][c] == SENTINEL_INDEX[alphabet]]


def query_bytes(alphabet):
    """every byte value that may stand in a query that walks an index: all but the sentinel class"""
    return [c for c in range(256) if INDEX[alphabet][c] != SENTINEL_INDEX[alphabet]]


class Variant:
    """one string of a byte-rich list: base[source] with byte `value` at `position` (None: the base string itself)"""
    __slots__ = ("string", "source", "position", "value")

    def __init__(self, string, source, position, value):
        self.string, self.source, self.position, self.value = string, source, position, value


def byte_rich(base, values=range(256), lanes=4):
    """From a list of strings: variants in which ONE position holds byte b, for every b of `values`, the position rotating.  Byte
    b gets 4 * lanes variants in a row, variant (r, l) at a position that is r mod 4 (a string too short to have one is passed
    over for that variant) and at a list index that is l mod lanes -- with lanes = 4 the four k-mers a thread of
    encodeCodes4Kernel decodes together; over the bytes the position moves on through the string and the base string through
    the list.  Strings of length 0 are passed over.  -> [Variant]; check_coverage asserts what this promises."""
    base = [bytes(s) for s in base]
    usable = [k for k, s in enumerate(base) if len(s)]
    assert any(len(s) >= 4 for s in base), "byte_rich needs a string of four characters"
    out, turn = [], 0
    for b in values:
        for r in range(4):
            for lane in range(lanes):
                assert len(out) % lanes == lane
                while len(base[usable[turn % len(usable)]]) <= r:  # too short to have such a position: the next string
                    turn += 1
                source = usable[turn % len(usable)]
                s = base[source]
                slots = list(range(r, len(s), 4))
                position = slots[(turn // len(usable) + b + lane) % len(slots)]
                out.append(Variant(s[:position] + bytes([b]) + s[position + 1:], source, position, b))
                turn += 1
    return out


def check_coverage(variants, values=range(256), lanes=4, fixed_length=0, first=0):
    """every byte of `values` stands at every position mod 4 of a string, and -- fixed_length != 0: all strings have that length
    -- at every position mod 4 in each of the `lanes` k-mers that are decoded together (list index mod lanes; `first`: the list
    index of variants[0] in the batch)"""
    seen = set()
    for k, v in enumerate(variants):
        if v.position is None:
            continue
        assert v.string[v.position] == v.value
        if fixed_length:
            assert len(v.string) == fixed_length
        seen.add((v.value, v.position % 4, (first + k) % lanes))
    missing = [(b, r, lane) for b in values for r in range(4) for lane in range(lanes) if (b, r, lane) not in seen]
    assert not missing, ("byte values that do not stand at every position mod 4 of every lane", missing[:8], len(missing))


def alias_pairs(base, alphabet, values=range(256)):
    """for every byte b of `values` one (base string, the same string with a byte of b's class replaced by b), the string and the
    place moving on from byte to byte: the two must get the same answer from anything that reads letters.  -> [Variant]; a class
    no base string holds is an error"""
    base = [bytes(s) for s in base]
    places = {}
    for k, s in enumerate(base):
        for p, c in enumerate(s):
            places.setdefault(class_of(alphabet, c), []).append((k, p))
    out = []
    for b in values:
        have = places.get(class_of(alphabet, b))
        assert have, ("no base string holds a byte of the class of", b, class_of(alphabet, b))
        k, p = have[(b * 7) % len(have)]
        out.append(Variant(base[k][:p] + bytes([b]) + base[k][p + 1:], k, p, b))
    return out


def csr(strings):
    """-> (chars uint8, offsets uint64[n + 1]); one spare byte when there is no character at all"""
    offsets = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum([len(s) for s in strings], out=offsets[1:])
    joined = b"".join(strings)
    return np.frombuffer(joined, np.uint8).copy() if joined else np.zeros(1, np.uint8), offsets


# ---- what a search must return ----------------------------------------------------------------------------------------------
def table_index(alphabet, seed):
    """the reference's k-mer table index of the last seed_k characters (ref src/AwFmKmerTable.c:21-51): the letter indices as
    digits, first character most significant -- an index of 20 carries into the next digit"""
    index = 0
    for c in seed:
        index = index * CARDINALITY[alphabet] + int(INDEX[alphabet][c])
    return index


def overflows(alphabet, query, seed_k):
    """True for a query whose reference table index is not below the table's length (the seed's leading digits are 19 .. 19, 20):
    the reference and the oracle read past the table there; the product starts such a k-mer from its last letter instead
    (csrc/awfm_search_kernel.h, `index < ix.seedLen`; include/awfm_gpu.h at awfmGpuSearch)"""
    if seed_k == 0 or len(query) < seed_k:
        return False
    seed = query[len(query) - seed_k:]
    if any(AMBIGUOUS[alphabet][c] for c in seed):
        return False
    return table_index(alphabet, seed) >= CARDINALITY[alphabet] ** seed_k


def carries(alphabet, query, k):
    """True when one of the last k characters is no proper letter and not ambiguous either (amino: the 90 bytes)"""
    return len(query) >= k > 0 and any(INDEX[alphabet][c] >= CARDINALITY[alphabet] and not AMBIGUOUS[alphabet][c] for c in query[len(query) - k:])


def stepwise(oi, alphabet, query):
    """the plain letter-by-letter backward search (ref src/AwFmSearch.c:317-358) from the oracle's single step and prefix sums"""
    letters = INDEX[alphabet]
    prefix = oi.prefix_sums()
    assert not any(letters[c] == SENTINEL_INDEX[alphabet] for c in query), "a sentinel-class byte in a query that walks an index"
    a = int(letters[query[-1]])
    sp, ep = int(prefix[a]), int(prefix[a + 1]) - 1
    for c in reversed(query[:-1]):
        if sp > ep:
            break
        sp, ep = oi.step(sp, ep, int(letters[c]))
    return sp, ep


def expected_search(oi, alphabet, seed_k, strings, threads=4):
    """(sp, ep, counts, overflowing: bool[n]) of the batch search: the oracle's (the reference's seed table and extension) for
    every query whose table index stays inside the table, the letter-by-letter search for the others, which the oracle is never
    given"""
    over = np.array([overflows(alphabet, s, seed_k) for s in strings], bool)
    inside = [s for s, o in zip(strings, over) if not o]
    sp, ep = np.zeros(len(strings), np.uint64), np.zeros(len(strings), np.uint64)
    if inside:
        chars, offsets = csr(inside)
        sp[~over], ep[~over], _, _ = oi.batch_search(chars, offsets, threads=threads)
    for k in np.flatnonzero(over):
        sp[k], ep[k] = stepwise(oi, alphabet, strings[k])
    counts = np.where(sp <= ep, ep - sp + np.uint64(1), np.uint64(0)).astype(np.uint32)
    return sp, ep, counts, over


# ---- texts and queries --------------------------------------------------------------------------------------------------------
def well_formed_text(seed, n, alphabet, ambiguity_runs=6):
    """a text an index may be walked on: nucleotide a c g t with a few runs of n; amino the twenty letters in lower case with a
    few runs of x and single b (the sanitiser's z) -- one case, no other byte (tests/test_reference_parity.py, module docstring)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer((b"acgt" if alphabet == DNA else AMINO_LETTERS.encode()), np.uint8)
    text = rng.choice(letters, n).astype(np.uint8)
    for at in rng.integers(8, max(n - 8, 9), ambiguity_runs):
        text[at:at + int(rng.integers(1, 4))] = ord("n") if alphabet == DNA else ord("x")
    if alphabet == AMINO and n > 64:
        text[rng.integers(8, n - 8, ambiguity_runs)] = ord("b")
    return text


def stored_ambiguity_places(text, alphabet):
    return np.flatnonzero(INDEX[alphabet][text] >= CARDINALITY[alphabet])


def base_queries(seed, text, alphabet, count, lengths, keep_clear=0):
    """well-formed queries: two thirds cut from the text (half of those across one of its ambiguity runs), one third random letters,
    upper case in a third of the characters.  For the amino alphabet every sixth planted query that holds a stored ambiguity
    letter gets it replaced by 'j' where it lies ahead of the last keep_clear characters: a byte of index 20 that is not
    ambiguous, on a query that still has hits.  lengths: an int (fixed) or (lo, hi) inclusive"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer((b"acgt" if alphabet == DNA else AMINO_LETTERS.encode()), np.uint8)
    odd = stored_ambiguity_places(text, alphabet)
    out = []
    for k in range(count):
        m = lengths if isinstance(lengths, int) else int(rng.integers(lengths[0], lengths[1] + 1))
        m = min(m, len(text))
        if k % 3 == 2 or m == 0:
            q = bytearray(rng.choice(letters, m).tobytes())
        else:
            if k % 3 == 0 and len(odd):
                at = int(rng.choice(odd)) - int(rng.integers(0, m))
            else:
                at = int(rng.integers(0, len(text) - m + 1))
            at = min(max(at, 0), len(text) - m)
            q = bytearray(text[at:at + m].tobytes())
            if alphabet == AMINO and k % 6 == 0:
                for p in range(m - keep_clear):
                    if AMBIGUOUS[AMINO][q[p]]:
                        q[p] = ord("j")
        for p in range(m):
            if rng.random() < 1 / 3 and 97 <= q[p] <= 122:
                q[p] &= 0xDF
        out.append(bytes(q))
    return out


def search_batch(seed, text, alphabet, lengths, base_count=60, lanes=4, keep_clear=0, fill=0):
    """the byte-rich batch of the search tests: base queries, their byte-rich variants (every byte but the sentinel class), an
    alias pair for every such byte, and `fill` more well-formed queries behind them -> (strings, base, variants, aliases, first
    index of the variants, first index of the aliases); the base strings come first"""
    base = base_queries(seed, text, alphabet, base_count, lengths, keep_clear)
    while len(base) % lanes:
        base.append(base[0])
    values = query_bytes(alphabet)
    variants = byte_rich(base, values, lanes)
    aliases = alias_pairs(base, alphabet, values)
    strings = base + [v.string for v in variants] + [v.string for v in aliases] + base_queries(seed + 1, text, alphabet, fill, lengths, keep_clear)
    return strings, base, variants, aliases, len(base), len(base) + len(variants)


def zones(variants, alphabet, seed_k, deep_k):
    """{(class, zone)} of the variants' bytes: zone 0 among the last seed_k characters, 1 among the last deep_k but not the last
    seed_k, 2 ahead of both"""
    found = set()
    for v in variants:
        back = len(v.string) - v.position  # 1: the last character
        found.add((class_of(alphabet, v.value), 0 if back <= seed_k else 1 if back <= deep_k else 2))
    return found


def assert_alias_property(aliases, first, sp, ep, what=""):
    """a query and its copy with one byte replaced by another byte of the same class return the same range"""
    for k, v in enumerate(aliases):
        got, want = (int(sp[first + k]), int(ep[first + k])), (int(sp[v.source]), int(ep[v.source]))
        if got[0] > got[1] and want[0] > want[1]:
            continue  # both empty (the hits-only calls promise some empty range, not which)
        assert got == want, (what, "byte", v.value, "at", v.position, "of base string", v.source, got, want)


def classes_with_hits(alphabet, strings, counts):
    """the classes that stand in a query with hits"""
    found = set()
    for s, c in zip(strings, counts):
        if c:
            found.update(class_of(alphabet, b) for b in s)
    return found


def all_query_classes(alphabet):
    return {key for key in classes(alphabet) if key[0] != SENTINEL_INDEX[alphabet]}


# ---- the read path: reads and texts with a third of their bytes drawn from all 256 ---------------------------------------
_ORDER = np.random.default_rng(256).permutation(256).astype(np.uint8)
_OTHERS = {}


def enrich(seed, data, alphabet, share=1 / 3):
    """a copy of the byte array with about `share` of its bytes replaced: two in three by the next byte value of a fixed order
    of all 256 -- counted per position mod 4 and begun a quarter of the way on from residue to residue, so that every value is
    there once 64 bytes of every residue are replaced, and at every position mod 4 once 256 are --, the third by another byte
    of the class it had (still equal up to alias)"""
    rng = np.random.default_rng(seed)
    data = np.array(data, np.uint8)
    hit = np.flatnonzero(rng.random(data.size) < share)
    turn = [0, 0, 0, 0]
    for k, p in enumerate(hit):
        if k % 3 == 2:
            data[p] = alias_of(alphabet, rng, int(data[p]))
        else:
            r = int(p) % 4
            data[p] = _ORDER[(turn[r] + 64 * r) % 256]
            turn[r] += 1
    return data


def values_by_residue(data, begin=0):
    """{(byte value, position mod 4)} of a buffer whose first byte lies `begin` bytes into its allocation"""
    data = np.asarray(data, np.uint8)
    return set(zip(data.tolist(), ((np.arange(data.size) + begin) % 4).tolist()))


def assert_every_value(data, what, by_residue=False):
    if by_residue:
        have = values_by_residue(data)
        missing = [(b, r) for b in range(256) for r in range(4) if (b, r) not in have]
    else:
        missing = sorted(set(range(256)) - set(np.asarray(data).tolist()))
    assert not missing, (what, "byte values that never stand there", missing[:8], len(missing))


def alias_of(alphabet, rng, c):
    """another byte of c's class where there is one (a proper letter: always)"""
    if alphabet not in _OTHERS:
        _OTHERS[alphabet] = [[b for b in members if b != c] for c in range(256) for members in [classes(alphabet)[class_of(alphabet, c)]]]
    same = _OTHERS[alphabet][c]
    return int(same[int(rng.integers(0, len(same)))]) if same else c


def enrich_case(case, seed):
    """a case of the read path's common modules with its read buffer and its text enriched (the records' ends, the offsets and
    the slots stay: a text's terminators are positions no record owns, whatever byte stands there)"""
    case.read_chars = enrich(seed, case.read_chars, case.alphabet)
    case.text = enrich(seed + 1, case.text, case.alphabet)
    if hasattr(case, "reads"):
        case.reads = [bytes(case.read_chars[int(a):int(z)]) if a <= z else b"" for a, z in zip(case.offsets[:-1], case.offsets[1:])]
    return case


# the explicit pairs: a read that agrees with its text only up to alias, and equal non-letters that face each other
ALIAS_TEXT = {DNA: b"acgtacgtttgacatgcatgcaat", AMINO: (AMINO_LETTERS + "acdw").encode()}
ALIAS_READ = {DNA: b"ACGUACGUUUGACAUGCAUGCAAU",                     # t against U, the case changed
              AMINO: bytes((c & 31) | 0xC0 for c in ALIAS_TEXT[AMINO])}  # a against 0xC1: the low five bits alone
# no proper letter among them; the sentinel class, the ambiguity letters and bytes of 0x80 and above are
NON_LETTERS = {DNA: b"nN$\x04-*7\x80\xff\x00xRyK@[`{\xe1\xc3\xe7\xf4\xd5\x9f",
               AMINO: b"zZxXbB$joUJO@5\x00\x1b\x1f\x7f\x80\xa0\xe0\xff\xfb\xea"}
for _a in (DNA, AMINO):
    assert len(ALIAS_TEXT[_a]) == len(ALIAS_READ[_a]) == len(NON_LETTERS[_a]) == 24
    assert all(INDEX[_a][p] == INDEX[_a][q] < CARDINALITY[_a] and p != q for p, q in zip(ALIAS_TEXT[_a], ALIAS_READ[_a]))
    assert all(INDEX[_a][c] >= CARDINALITY[_a] for c in NON_LETTERS[_a])
PAIR_RECORDS = {a: [ALIAS_TEXT[a], NON_LETTERS[a]] for a in (DNA, AMINO)}
