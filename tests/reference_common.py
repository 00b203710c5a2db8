"""Shared by the tests that compare with the reference itself (test_reference_parity.py, live on the CPU against
oracle/_ref/libawfm_ref.so) and with what it recorded (test_gpu_reference_parity.py against tests/golden/ref_*.npz,
written by scripts/make_reference_golden.py): the texts, the query mix and the fixture cases."""
import os

import numpy as np

DNA = b"acgt"
AMINO = b"acdefghiklmnpqrstvwy"
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SA_PAD_BYTES = 8  # bytes the .awfmi format appends to the sampled suffix array; it gives them no meaning


def letters_of(amino):
    return AMINO if amino else DNA


def random_text(rng, n, letters):
    return bytes(np.frombuffer(bytes(letters), np.uint8)[rng.integers(0, len(letters), n)])


TEXT_KINDS = ("random", "two-letter", "homopolymer", "ambiguity-runs", "all-ambiguous", "ambiguous-ends", "upper", "mixed-case",
              "foreign-bytes")


def make_text(kind, rng, n, amino):
    """n characters of one of TEXT_KINDS"""
    letters = letters_of(amino)
    amb = b"x" if amino else b"n"
    if kind == "random":
        return random_text(rng, n, letters)
    if kind == "two-letter":
        two = letters[:2]
        return (two * n)[:n // 2] + random_text(rng, n // 4, two) + (two[::-1] * n)[:n - n // 2 - n // 4]
    if kind == "homopolymer":
        return letters[2:3] * n
    if kind == "ambiguity-runs":
        t = bytearray(random_text(rng, n, letters))
        for at in rng.integers(0, n, max(n // 120, 2)):
            m = int(rng.integers(1, 40))
            t[at:at + m] = (amb * m)[:len(t[at:at + m])]
        return bytes(t)
    if kind == "all-ambiguous":
        return (b"xzbjou*" if amino else b"nxrykm-") * (n // 7) + amb * (n % 7)
    if kind == "ambiguous-ends":
        t = bytearray(random_text(rng, n, letters))
        t[0] = t[-1] = amb[0]
        return bytes(t)
    if kind == "upper":
        return random_text(rng, n, letters).upper()
    if kind == "mixed-case":
        t = bytearray(random_text(rng, n, letters))
        for i in np.flatnonzero(rng.random(n) < 0.5):
            t[i] -= 32
        return bytes(t)
    if kind == "foreign-bytes":
        t = bytearray(random_text(rng, n, letters))
        for i in np.flatnonzero(rng.random(n) < 0.05):
            t[i] = (0, ord("7"), 255, ord(" "), ord("0"), 127)[int(rng.integers(0, 6))]
        return bytes(t)
    raise ValueError(kind)


def make_queries(rng, text, amino, seed_k, count):
    """queries of 1 .. 60 characters: planted, mutated and random; shorter than, equal to and longer than the seed;
    ambiguity letters inside and outside the seed (the last seed_k characters); either case.  Never empty: the
    reference computes kmerLength - 1 on an empty query."""
    letters = letters_of(amino)
    n = len(text)
    amb = (b"x", b"z", b"b", b"X") if amino else (b"n", b"x", b"N", b"r")
    out = [bytes([c]) for c in letters] + [bytes([c]).upper() for c in letters] + list(amb)
    out += [text[:1], text[-1:], text[:seed_k], text[-seed_k:], text[:min(n, 60)], text[-min(n, 60):]]
    for i in range(count):
        kind = i % 7
        if kind == 0:
            m = int(rng.integers(1, seed_k + 1))           # up to the seed length
        elif kind == 1:
            m = seed_k if rng.random() < 0.5 else seed_k + 1
        else:
            m = int(rng.integers(1, 61))
        m = max(1, min(m, n))
        at = int(rng.integers(0, n - m + 1))
        q = bytearray(text[at:at + m])
        if kind == 2:
            q = bytearray(random_text(rng, m, letters))
        elif kind == 3:                                    # one mutation
            q[int(rng.integers(0, m))] = letters[int(rng.integers(0, len(letters)))]
        elif kind == 4:                                    # an ambiguity letter inside the seed
            q[m - 1 - int(rng.integers(0, min(seed_k, m)))] = amb[int(rng.integers(0, len(amb)))][0]
        elif kind == 5 and m > seed_k:                     # ... and outside it
            q[int(rng.integers(0, m - seed_k))] = amb[int(rng.integers(0, len(amb)))][0]
        q = bytes(q)
        if rng.random() < 0.25:
            q = q.upper() if rng.random() < 0.5 else q.lower()
        out.append(q)
    return [q for q in out if len(q)]


def pack(queries):
    """-> (chars uint8, offsets uint64[n+1])"""
    lens = np.fromiter((len(q) for q in queries), np.uint64, len(queries))
    offsets = np.zeros(len(queries) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    return np.frombuffer(b"".join(queries), np.uint8).copy(), offsets


def sa_payload_bytes(bwt_length, ratio):
    """bytes of the sampled suffix array that hold sample bits (the section minus its 8 padding bytes)"""
    width = max(1, (bwt_length - 1).bit_length())
    samples = (bwt_length + ratio - 1) // ratio
    return (samples * width + 7) // 8


def sa_samples(packed, bwt_length, ratio):
    """the samples of a packed suffix array decoded in plain Python integers (no window loads, no masks of fixed width)"""
    width = max(1, (bwt_length - 1).bit_length())
    samples = (bwt_length + ratio - 1) // ratio
    stream = int.from_bytes(bytes(packed[:sa_payload_bytes(bwt_length, ratio)]), "little")
    mask = (1 << width) - 1
    return np.array([(stream >> (i * width)) & mask for i in range(samples)], dtype=np.uint64)


def with_padding(blob, byte):
    """an .awfmi file's bytes with the 8 padding bytes behind the last sample (the end of the file: no FASTA section)
    set to `byte`"""
    out = bytearray(blob)
    out[-SA_PAD_BYTES:] = bytes([byte]) * SA_PAD_BYTES
    return bytes(out)


# name, alphabet, text kind, text length, sa ratio, seed k, queries -- what scripts/make_reference_golden.py records.
# 4095 characters: a BWT of exactly 256*16 positions; 4096: 256*16 + 1.  1300 characters -> 11-bit samples, 5000 -> 13-bit:
# with ratio 3 / 8 the last sample ends mid-byte.  2999 characters, ratio 1 -> 3000 samples of 12 bits, and 2503 -> 2504 of 12:
# the last sample ends exactly on a byte boundary, so the bit behind it is the first padding bit, and the BWT length is no
# power of two (a sample that kept one bit too many would vanish in the reduction modulo the BWT length).  Seed tables
# stay at 4^6 / 20^2 entries or fewer (file size).
FIXTURE_CASES = [
    ("ref_dna_r1", "dna", "random", 2999, 1, 4, 600),
    ("ref_dna_r3_midbyte", "dna", "ambiguity-runs", 1300, 3, 3, 600),
    ("ref_dna_r8_256m", "dna", "mixed-case", 4095, 8, 6, 700),
    ("ref_dna_r8_256m1", "dna", "random", 4096, 8, 5, 700),
    ("ref_dna_r255", "dna", "foreign-bytes", 9000, 255, 4, 500),
    ("ref_dna_two_letter", "dna", "two-letter", 3300, 3, 2, 600),
    ("ref_amino_r1", "amino", "random", 2503, 1, 2, 600),
    ("ref_amino_r8_midbyte", "amino", "ambiguity-runs", 5000, 8, 1, 700),
]


def fixture_inputs(case):
    """the seeded text and queries of a fixture case"""
    name, alpha, kind, n, ratio, seed_k, nq = case
    rng = np.random.default_rng([FIXTURE_CASES.index(case), 20260])
    amino = alpha == "amino"
    text = make_text(kind, rng, n, amino)
    queries = make_queries(rng, text, amino, seed_k, nq)
    return text, queries


def longest_match_expected(walk, min_length):
    """what awfmLongestSuffixMatches reports for step-walk results [(length, (sp, ep))] -> (lengths, ranges, counts)"""
    lengths = np.array([w[0] for w in walk], np.uint32)
    ranges = np.array([w[1] if w[0] >= max(min_length, 1) else (1, 0) for w in walk], np.uint64).reshape(-1, 2)
    counts = np.where(ranges[:, 0] <= ranges[:, 1], ranges[:, 1] - ranges[:, 0] + np.uint64(1), np.uint64(0)).astype(np.uint32)
    return lengths, ranges, counts
