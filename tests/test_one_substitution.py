"""awfmOneSubstitutionSearch (include/awfm_gpu.h, csrc/awfm_search_host.c): the host twin of the batched one-substitution search,
against checkers that share no code with it -- a brute force over sorted suffixes, the library's single-string search on every
variant string spelled out in Python, and the compiled reference's awFmFindSearchRangeForString -- and against itself: order,
threads, capacity, include_exact, NULL outputs."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_match_common as lm  # noqa: E402
import one_substitution_common as osc  # noqa: E402

SEED_K = {"random": 8, "two-letter": 4, "n-runs": 8, "amino": 2}
DEEP_K = {"random": 10, "two-letter": 7, "n-runs": 10, "amino": 3}
NAMES = sorted(SEED_K)
_cache = {}


def case(awfm, name):
    """index, mix and the twin's full answer for one small text: computed once, shared, left unchanged"""
    if name not in _cache:
        text, amino = lm.small_texts()[name]
        ix = awfm.create_index(text, awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 4, SEED_K[name])
        mix = osc.make_mix(np.random.default_rng(len(name) + 5), text, amino, SEED_K[name], DEEP_K[name])
        chars, offsets = osc.pack([q for q, _, _ in mix])
        got = awfm.one_substitution_search_host(ix, chars, offsets)
        _cache[name] = (text, amino, ix, mix, chars, offsets, got, osc.as_set(*got[:3]))
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_every_variant_string_has_the_range_of_the_single_string_search(awfm, name):
    text, amino, ix, mix, chars, offsets, got, records = case(awfm, name)
    table = osc.letter_table(amino)
    want = set()
    for i, (q, _, _) in enumerate(mix):
        for edit, s in osc.variants(q, amino, table):
            sp, ep = ix.find_search_range_for_string(s)
            if sp <= ep:
                want.add((i, edit, sp, ep))
        if len(q):
            sp, ep = ix.find_search_range_for_string(q)
            if sp <= ep:
                want.add((i, osc.EDIT_NONE, sp, ep))
    assert records == want, (sorted(records - want)[:5], sorted(want - records)[:5])
    assert got[3] == len(want)
    v, o = osc.per_query(want, len(mix))
    assert np.array_equal(got[4], v) and np.array_equal(got[5], o)
    # by construction: a one-off query cut from a pure piece has the record that undoes its substitution
    has_variant = np.zeros(len(mix), bool)
    for q, edit, _, _ in want:
        has_variant[q] |= edit != osc.EDIT_NONE
    assert all(has_variant[i] for i, (_, _, planted) in enumerate(mix) if planted)


@pytest.mark.parametrize("name", NAMES)
def test_occurrences_of_every_variant_of_every_pure_query_by_brute_force(awfm, name):
    text, amino, ix, mix, chars, offsets, got, records = case(awfm, name)
    brute = lm.BruteForce(text, amino)
    table = osc.letter_table(amino)
    size = {(q, edit): ep - sp + 1 for q, edit, sp, ep in records}
    checked = 0
    for i, (q, pure, _) in enumerate(mix):
        if not pure:
            continue
        for edit, s in osc.variants(q, amino, table):
            assert brute.occurrences(s) == size.get((i, edit), 0), (i, q, edit)
            checked += 1
        if len(q):
            assert brute.occurrences(q) == size.get((i, osc.EDIT_NONE), 0), (i, q)
    assert checked > 10000


@pytest.mark.parametrize("name", NAMES)
def test_the_compiled_reference_gives_the_same_ranges(awfm, name):
    from oracle import reference as R
    if not R.available():
        pytest.skip("oracle/_ref/libawfm_ref.so is not built")
    R.lib()
    text, amino, ix, mix, chars, offsets, got, records = case(awfm, name)
    table = osc.letter_table(amino)
    ri = R.Index.from_text(text, 1 if amino else 2, 4, SEED_K[name])
    ranges = {(q, edit): (sp, ep) for q, edit, sp, ep in records}
    rng = np.random.default_rng(9)
    chosen = [int(i) for i in rng.choice(len(mix), 200, replace=False) if 0 < len(mix[int(i)][0]) <= 150]
    for i in chosen:
        for edit, s in osc.variants(mix[i][0], amino, table):
            sp, ep = ri.range_for_string(s)
            assert ranges.get((i, edit)) == ((sp, ep) if sp <= ep else None), (i, mix[i][0], edit)
    ri.free()


@pytest.mark.parametrize("name", NAMES)
def test_order_threads_capacity_and_include_exact(awfm, name):
    text, amino, ix, mix, chars, offsets, got, records = case(awfm, name)
    queries, edits, ranges, total, variants, occurrences = got
    assert total == queries.size > 0
    key = queries.astype(np.uint64) << np.uint64(32) | edits.astype(np.uint64)
    assert (key[1:] > key[:-1]).all()  # sorted by (query, edit), no duplicates; the unedited query last among its own
    for threads in (1, 4):
        again = awfm.one_substitution_search_host(ix, chars, offsets, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(again[:3], got[:3])) and again[3] == total
        assert np.array_equal(again[4], variants) and np.array_equal(again[5], occurrences)
    # a capacity below the number of records: the first of the order, the true total, complete per-query arrays
    cap = total // 3
    few = awfm.one_substitution_search_host(ix, chars, offsets, capacity=cap)
    assert few[3] == total and few[0].size == cap
    assert all(np.array_equal(a, b[:cap]) for a, b in zip(few[:3], got[:3]))
    assert np.array_equal(few[4], variants) and np.array_equal(few[5], occurrences)
    # include_exact off: the same records without the unedited queries
    keep = edits != osc.EDIT_NONE
    assert keep.any() and not keep.all()
    off = awfm.one_substitution_search_host(ix, chars, offsets, include_exact=False)
    assert all(np.array_equal(a, b[keep]) for a, b in zip(off[:3], got[:3])) and off[3] == int(keep.sum())
    exact = np.bincount(queries[~keep], minlength=len(mix))
    assert np.array_equal(off[4], variants - exact.astype(np.uint32))
    # the fixed-length form
    fixed = np.frombuffer(text[:2100], np.uint8)
    a = awfm.one_substitution_search_host(ix, fixed, fixed_length=21)
    b = awfm.one_substitution_search_host(ix, fixed, np.arange(0, 2101, 21, dtype=np.uint64))
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] >= 100


def test_null_and_zero_cases(awfm):
    from avxwindowfmindex_amd import _lib
    text, amino, ix, mix, chars, offsets, got, records = case(awfm, "random")
    L = _lib.lib()
    n = len(mix)
    total = C.c_uint64(77)
    # nothing to do: succeeds and touches nothing, whatever else is missing
    assert L.awfmOneSubstitutionSearch(ix.ptr, None, None, 0, 0, 1, None, None, None, 0, C.byref(total), None, None, 2) == 1
    assert total.value == 77
    # every output NULL
    assert L.awfmOneSubstitutionSearch(ix.ptr, chars.ctypes.data, offsets.ctypes.data, 0, n, 1, None, None, None, 0, None, None, None, 2) == 1
    # counts only
    variants = np.zeros(n, np.uint32)
    assert L.awfmOneSubstitutionSearch(ix.ptr, chars.ctypes.data, offsets.ctypes.data, 0, n, 1, None, None, None, 0, C.byref(total),
                                       variants.ctypes.data, None, 2) == 1
    assert total.value == got[3] and np.array_equal(variants, got[4])
    # one list alone
    edits = np.zeros(got[3], np.uint32)
    assert L.awfmOneSubstitutionSearch(ix.ptr, chars.ctypes.data, offsets.ctypes.data, 0, n, 1, None, edits.ctypes.data, None, got[3],
                                       None, None, None, 2) == 1
    assert np.array_equal(edits, got[1])
    # no way to find the queries; no index; too many queries for 32-bit query numbers
    assert L.awfmOneSubstitutionSearch(ix.ptr, None, offsets.ctypes.data, 0, n, 1, None, None, None, 0, None, None, None, 2) == -4
    assert L.awfmOneSubstitutionSearch(ix.ptr, chars.ctypes.data, None, 0, n, 1, None, None, None, 0, None, None, None, 2) == -4
    assert L.awfmOneSubstitutionSearch(None, chars.ctypes.data, offsets.ctypes.data, 0, n, 1, None, None, None, 0, None, None, None, 2) == -4
    assert L.awfmOneSubstitutionSearch(ix.ptr, chars.ctypes.data, offsets.ctypes.data, 0, 1 << 32, 1, None, None, None, 0, None, None, None, 2) < 0
    # an empty query and a query of one letter
    empty = awfm.one_substitution_search_host(ix, np.zeros(0, np.uint8), np.zeros(2, np.uint64))
    assert empty[3] == 0 and empty[4].tolist() == [0]
    one = awfm.one_substitution_search_host(ix, b"a", fixed_length=1)
    assert one[1].tolist() == [1, 2, 3, osc.EDIT_NONE] and one[0].tolist() == [0] * 4
