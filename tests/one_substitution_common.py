"""Shared by the one-substitution tests (test_one_substitution.py on the host, test_gpu_one_substitution.py on the device): the
query mix, the enumeration of a query's variants in plain Python (include/awfm_gpu.h: the definition verbatim -- position p
replaced by a proper letter c other than q[p]'s own, edit = p * 32 + c), and the host twin's records as a set."""
import ctypes as C

import numpy as np

import longest_match_common as lm

EDIT_NONE = 0xFFFFFFFF
MAX_POSITION = 1 << 27


def letter_table(amino):
    """ASCII code -> letter index of the library's mapping (awfmNucAsciiToIndex / awfmAminoAsciiToIndex), 256 entries"""
    from avxwindowfmindex_amd import _lib
    f = _lib.lib().awfmAminoAsciiToIndex if amino else _lib.lib().awfmNucAsciiToIndex
    f.restype, f.argtypes = C.c_uint8, [C.c_uint8]
    return [int(f(c)) for c in range(256)]


def variants(query, amino, table):
    """(edit, variant string) of every variant of the query, in the order of the edits"""
    letters = lm.letters_of(amino)
    q = bytes(query)
    for p in range(min(len(q), MAX_POSITION)):
        own = table[q[p]]
        for c in range(len(letters)):
            if c != own:
                yield p * 32 + c, q[:p] + letters[c:c + 1] + q[p + 1:]


def one_off(rng, text, letters, m, where):
    """text[at:at+m] with exactly one position (chosen by `where(m)`) replaced by another of the alphabet's letters -> (query,
    cut from a piece made of the alphabet's letters only)"""
    at = int(rng.integers(0, len(text) - m))
    piece = bytearray(text[at:at + m])
    core = set(letters)
    pure = all(c in core for c in piece)
    p = where(m)
    others = [c for c in letters if c != piece[p]]
    piece[p] = others[int(rng.integers(0, len(others)))]
    return bytes(piece), pure


def make_mix(rng, text, amino, seed_k, deep_k):
    """list of (query, pure, planted): 400 of longest_match_common.make_queries; 400 one-off queries of 1..60 characters, a third
    with the substitution left of the last deep_k letters (m > deep_k + 4), a third inside the last seed_k letters; 50 of 33..150
    characters that cross the 32-character register window.  pure: proper letters only; planted: a one-off query cut from a
    pure piece, which therefore has the record that undoes its substitution."""
    letters = lm.letters_of(amino)
    out = [(q, pure, False) for q, pure in lm.make_queries(rng, text, amino, 400)]
    for i in range(400):
        kind = i % 3
        if kind == 0:
            m = int(rng.integers(deep_k + 5, 61))
            q, pure = one_off(rng, text, letters, m, lambda m: int(rng.integers(0, m - deep_k)))
        elif kind == 1:
            m = int(rng.integers(1, 61))
            q, pure = one_off(rng, text, letters, m, lambda m: m - 1 - int(rng.integers(0, min(seed_k, m))))
        else:
            m = int(rng.integers(1, 61))
            q, pure = one_off(rng, text, letters, m, lambda m: int(rng.integers(0, m)))
        out.append((q, pure, pure))
    for _ in range(50):
        m = int(rng.integers(33, 151))
        q, pure = one_off(rng, text, letters, m, lambda m: int(rng.integers(0, m)))
        out.append((q, pure, pure))
    core = set(letters) | set(letters.upper())
    out = [(q, all(c in core for c in q), planted) for q, _, planted in out]
    assert 2 * sum(pure for _, pure, _ in out) >= len(out)
    return out


def pack(queries):
    """-> (chars uint8, offsets uint64[n + 1])"""
    lens = np.fromiter((len(q) for q in queries), np.uint64, len(queries))
    offsets = np.zeros(len(queries) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    return np.frombuffer(b"".join(queries), np.uint8).copy(), offsets


def as_set(queries, edits, ranges):
    """records as a set of (query, edit, sp, ep); asserts that they are distinct"""
    rows = set(zip(queries.tolist(), edits.tolist(), ranges[:, 0].tolist(), ranges[:, 1].tolist()))
    assert len(rows) == len(queries)
    return rows


def per_query(records, n):
    """(variants uint32[n], occurrences uint64[n]) recomputed from a set of records"""
    variants_, occurrences = np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    for q, _, sp, ep in records:
        variants_[q] += 1
        occurrences[q] += np.uint64(ep - sp + 1)
    return variants_, occurrences
