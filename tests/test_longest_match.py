"""awfmLongestSuffixMatches (include/awfm_gpu.h, csrc/awfm_search_host.c): the host twin of the batched longest-suffix-match
search against two checkers that share no code with it (longest_match_common.py): a brute force over sorted suffixes
for the queries made of the alphabet's own letters, and the walk over the public step functions -- the definition -- for all
of them.  Every query is compared with every checker that applies to it; none is skipped."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_match_common as lm  # noqa: E402

TEXTS = lm.small_texts()


def _index(awfm, name, seed_k):
    text, amino = TEXTS[name]
    return awfm.create_index(text, awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 4, seed_k), text, amino


def _lib():
    from avxwindowfmindex_amd import _lib
    return _lib.lib()


def _run(awfm, ix, queries, **kw):
    chars, starts, ends = lm.pack(queries)
    return awfm.longest_suffix_matches_host(ix, chars, starts, ends, **kw)


def _check_all(awfm, ix, text, amino, queries):
    lengths, ranges, counts = _run(awfm, ix, [q for q, _ in queries])
    brute = lm.BruteForce(text, amino)
    lib = _lib()
    compared = 0
    for i, (q, pure) in enumerate(queries):
        got = (int(lengths[i]), (int(ranges[i, 0]), int(ranges[i, 1])))
        assert got == lm.step_walk(lib, ix, q), (i, q)
        if pure:
            assert got == brute.match(q), (i, q)
            compared += 1
        size = got[1][1] - got[1][0] + 1 if got[0] else 0
        assert int(counts[i]) == size and (size > 0) == (got[0] > 0), (i, q)
        if got[0]:  # the plain search of the matched suffix ends in exactly the match range
            assert ix.find_search_range_for_string(q[len(q) - got[0]:]) == got[1], (i, q)
    assert compared >= len(queries) // 3
    return lengths, ranges, counts


@pytest.mark.parametrize("name,seed_k", [("random", 1), ("random", 4), ("random", 8), ("random", 12), ("two-letter", 4), ("n-runs", 8),
                                         ("amino", 1), ("amino", 2)])
def test_host_twin_against_both_checkers(awfm, name, seed_k):
    ix, text, amino = _index(awfm, name, seed_k)
    rng = np.random.default_rng(100 + seed_k)
    queries = lm.make_queries(rng, text, amino, 400)
    lengths, _, _ = _check_all(awfm, ix, text, amino, queries)
    by_query = {q: int(length) for (q, _), length in zip(queries, lengths)}
    assert by_query[b""] == 0 and by_query[text[-1:]] == 1 and by_query[text] == len(text)  # m = 0, m = 1, the whole text
    assert by_query[queries[-1][0]] >= len(text) and len(queries[-1][0]) > len(text)         # a query longer than the text
    assert (lengths > 32).any() and (lengths == np.array([len(q) for q, _ in queries]))[1:].any()
    if name == "two-letter":
        assert by_query[b"g"] == 0 and by_query[b"t"] == 0  # letters the text does not contain
    ix.dealloc()


@pytest.mark.parametrize("seed_k", [4, 8])
def test_matches_that_end_at_and_around_the_table_depth(awfm, seed_k):
    # a text short enough that strings of seed_k - 1 letters are missing from it
    text = TEXTS["random"][0][:4 ** (seed_k - 1) // 2 + 30]
    ix = awfm.create_index(text, awfm.AwFmAlphabetDna, 4, seed_k)
    rng = np.random.default_rng(seed_k)
    queries, want = [], []
    for depth in (seed_k - 1, seed_k, seed_k + 1):
        made = 0
        while made < 20:
            at = int(rng.integers(0, len(text) - depth))
            piece = text[at:at + depth]
            before = [bytes([c]) for c in lm.DNA if bytes([c]) + piece not in text]
            if not before:
                continue
            queries.append((lm.random_text(rng, int(rng.integers(0, 30)), lm.DNA) + before[0] + piece, True))
            want.append(depth)
            made += 1
    lengths, _, _ = _check_all(awfm, ix, text, False, queries)
    assert lengths.tolist() == want
    ix.dealloc()


def test_windows_forms_threshold_and_threads(awfm):
    ix, text, _ = _index(awfm, "random", 8)
    rng = np.random.default_rng(5)
    read = np.frombuffer(lm.mutate(rng, text[700:850], lm.DNA, 0.05), np.uint8)
    ends = np.arange(4, read.size + 1, 4, dtype=np.uint64)
    starts = np.where(ends > 64, ends - 64, 0).astype(np.uint64)
    # overlapping windows over one read = the same windows copied out as separate queries
    over = awfm.longest_suffix_matches_host(ix, read, starts, ends)
    copied = _run(awfm, ix, [bytes(read[int(s):int(e)]) for s, e in zip(starts, ends)])
    for a, b in zip(over, copied):
        assert np.array_equal(a, b)
    assert over[0].max() > 16 and (over[0] < (ends - starts)).any()
    # CSR offsets = starts/ends; a fixed length = its offsets
    offsets = np.arange(0, read.size + 1, 10, dtype=np.uint64)
    csr = awfm.longest_suffix_matches_host(ix, read, offsets[:-1], offsets[1:])
    fixed = awfm.longest_suffix_matches_host(ix, read[:offsets[-1]], fixed_length=10)
    for a, b in zip(csr, fixed):
        assert np.array_equal(a, b) and a.shape[0] == offsets.size - 1
    # threads
    one = awfm.longest_suffix_matches_host(ix, read, starts, ends, threads=1)
    for a, b in zip(over, one):
        assert np.array_equal(a, b)
    # minLength at l - 1, l, l + 1 of one query, with every other query of the batch on either side of it
    lengths, ranges, counts = over
    pick = int(np.argmax(lengths))
    for threshold in (int(lengths[pick]) - 1, int(lengths[pick]), int(lengths[pick]) + 1):
        l2, r2, c2 = awfm.longest_suffix_matches_host(ix, read, starts, ends, min_length=threshold)
        assert np.array_equal(l2, lengths)  # the length is the true one either way
        keep = lengths >= max(threshold, 1)
        assert bool(keep[pick]) == (threshold <= int(lengths[pick]))
        assert np.array_equal(r2[keep], ranges[keep]) and np.array_equal(c2[keep], counts[keep])
        assert (r2[~keep] == np.array([1, 0], np.uint64)).all() and (c2[~keep] == 0).all()
    # an end before its start is an empty query
    l3, r3, c3 = awfm.longest_suffix_matches_host(ix, read, np.array([9], np.uint64), np.array([3], np.uint64))
    assert l3.tolist() == [0] and r3.tolist() == [[1, 0]] and c3.tolist() == [0]
    ix.dealloc()


def test_dropping_the_first_character(awfm):
    """l stays unless the whole query matched; then it is m - 1 and its range holds at least the old one's occurrences (every
    occurrence of cP is one of P one position on: the rows are other rows of the BWT, so it is the sizes that nest)"""
    ix, text, _ = _index(awfm, "random", 4)
    rng = np.random.default_rng(8)
    queries = [q for q, _ in lm.make_queries(rng, text, False, 300) if len(q) >= 2]
    full = _run(awfm, ix, queries)
    less = _run(awfm, ix, [q[1:] for q in queries])
    whole = 0
    for i, q in enumerate(queries):
        if int(full[0][i]) == len(q):
            whole += 1
            assert int(less[0][i]) == len(q) - 1
            assert int(less[2][i]) >= int(full[2][i]) >= 1
        else:
            assert int(less[0][i]) == int(full[0][i]) and np.array_equal(less[1][i], full[1][i])
    assert 20 <= whole <= len(queries) - 20
    ix.dealloc()


def test_null_outputs_and_return_codes(awfm):
    from avxwindowfmindex_amd import _lib
    ix, text, _ = _index(awfm, "random", 4)
    L = _lib.lib()
    chars, starts, ends = lm.pack([text[10:40], b"acgtn", text[100:101]])
    n = starts.size
    want = awfm.longest_suffix_matches_host(ix, chars, starts, ends)

    def call(index, c, s, e, fixed, count, lengths, ranges, counts):
        return L.awfmLongestSuffixMatches(index, c, s, e, fixed, count, 0, lengths, ranges, counts, 2)

    for missing in range(3):  # each output NULL in turn: the other two are written as before
        outs = [np.full(n, 77, np.uint32), np.full((n, 2), 77, np.uint64), np.full(n, 77, np.uint32)]
        args = [o.ctypes.data for o in outs]
        args[missing] = None
        assert call(ix.ptr, chars.ctypes.data, starts.ctypes.data, ends.ctypes.data, 0, n, *args) == awfm.AwFmSuccess
        for k in range(3):
            assert np.array_equal(outs[k], want[k]) if k != missing else (outs[k] == 77).all()
    outs = [np.full(n, 77, np.uint32), np.full((n, 2), 77, np.uint64), np.full(n, 77, np.uint32)]
    args = [o.ctypes.data for o in outs]
    null_ptr = -4  # AwFmNullPtrError
    assert call(None, chars.ctypes.data, starts.ctypes.data, ends.ctypes.data, 0, n, *args) == null_ptr
    assert call(ix.ptr, None, starts.ctypes.data, ends.ctypes.data, 0, n, *args) == null_ptr
    assert call(ix.ptr, chars.ctypes.data, starts.ctypes.data, None, 0, n, *args) == null_ptr      # starts without ends
    assert call(ix.ptr, chars.ctypes.data, None, None, 0, n, *args) == null_ptr                    # no way to find the queries
    assert call(ix.ptr, None, None, None, 0, 0, None, None, None) == awfm.AwFmSuccess              # nothing to do: touches nothing
    assert all((o == 77).all() for o in outs)
    ix.dealloc()
