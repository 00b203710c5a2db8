"""The texts of index_geometry_common.py on the host: what tests/test_gpu_index_geometry.py expects of the kernels -- the
oracle's ranges and positions, the host twins' longest suffix matches and one-substitution records -- pinned here to checkers
that share no code with them, at exactly these inputs: a brute force over sorted suffixes for every query made of the
alphabet's own letters, the walk over the product's step functions for the others, the walk over the compiled reference's
step functions for all of them, and the suffix array of a plain sort for every BWT row.  No tolerance, nothing skipped.

The texts are lower case with n (nucleotide) or x (amino) as their only other bytes, so none of them is one of the amino text
kinds on which the reference's index is ill-formed (tests/test_reference_parity.py); the empty query never reaches the
reference (longest_match_common.step_walk answers it itself)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_geometry_common as igc  # noqa: E402
import longest_match_common as lm  # noqa: E402
import one_substitution_common as osc  # noqa: E402
import reference_common as rc  # noqa: E402
from oracle import reference as R  # noqa: E402


@pytest.fixture(autouse=True)
def watchdog():
    """as in tests/test_reference_parity.py: the reference has inputs on which it does not return, and no test may hang the
    suite.  It ends the pytest process, not just the test."""
    import faulthandler
    faulthandler.dump_traceback_later(600, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def ref():
    if not R.available():
        if R.sources_present():
            pytest.fail("the reference's sources are present but oracle/_ref/libawfm_ref.so is not built "
                        "(python -c 'import __graft_entry__ as g; g.build()')")
        pytest.skip("neither oracle/_ref/libawfm_ref.so nor the reference's sources exist on this machine")
    R.lib()
    return R


def test_the_table_covers_every_class_and_a_shortened_one_does_not():
    assert igc.check_coverage(igc.TABLE)
    for flavour in igc.FLAVOURS:
        have = igc.entries(flavour)
        assert {e.local for e in have} == set(igc.LOCALS) and {e.L for e in have} == set(igc.LENGTHS)
        assert {e.block_class for e in have} == set(igc.BLOCK_CLASSES)
        for drop in [lambda e: e.local == 31, lambda e: e.L == 385, lambda e: e.block_class == "interior",
                     lambda e: e.block_class == "last-partial" and e.L == 513]:
            less = dict(igc.TABLE)
            less[flavour] = [(e.L, e.seed, e.r) for e in have if not drop(e)]
            assert len(less[flavour]) < len(have)
            with pytest.raises(AssertionError):
                igc.check_coverage(less)


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_the_batches_touch_the_geometry(awfm, oracle, flavour):
    """of the oracle's ranges (the other tests pin them); and the kinds of queries a batch has to have"""
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)
        igc.check_touches(e, x.sp, x.ep)  # (Expected() has asserted it already: a text that fails it cannot be used at all)
        assert e.must_touch() >= {e.r - 1, e.r, e.L - 1, e.block * 128} and int(x.suffix_array[e.r]) == 0
        lengths = x.longest[0][0]
        m = np.diff(x.offsets).astype(np.uint32)
        assert x.queries[0] == b"" and (~x.pure).any() and any(q != q.lower() for q in x.queries)
        for depth in range(1, 9):  # walks that die at every depth, and walks that do not
            assert ((lengths == depth) & (m > depth)).any() and ((lengths == depth) & (m == depth)).any(), (e, depth)


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_brute_force_against_the_oracle_and_the_host_twins(awfm, oracle, flavour):
    table = osc.letter_table(igc.is_amino(flavour))
    compared = 0
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)
        brute = lm.BruteForce(e.text, e.amino)
        lengths, ranges, counts = x.longest[0]
        for i, (q, pure) in enumerate(e.queries()):
            if not pure:
                continue
            length, (sp, ep) = brute.match(q)
            # the oracle's search: the brute force's range where the whole query occurs, an empty one where it does not
            if length == len(q) and q:
                assert (int(x.sp[i]), int(x.ep[i])) == (sp, ep) and int(x.count[i]) == ep - sp + 1, (e, q)
            else:
                assert int(x.sp[i]) > int(x.ep[i]) and int(x.count[i]) == 0, (e, q)
            # the host twin of the longest suffix match
            assert (int(lengths[i]), int(ranges[i, 0]), int(ranges[i, 1])) == (length, sp, ep), (e, q)
            assert int(counts[i]) == (ep - sp + 1 if length else 0), (e, q)
            compared += 1
        # min_length: the lengths stay, ranges and counts of the shorter matches become "none"
        l3, r3, c3 = x.longest[3]
        keep = lengths >= 3
        assert np.array_equal(l3, lengths) and np.array_equal(r3[keep], ranges[keep]) and np.array_equal(c3[keep], counts[keep]), e
        assert (r3[~keep] == np.array([1, 0], np.uint64)).all() and (c3[~keep] == 0).all() and keep.any() and (~keep).any(), e
        check_one_substitution(e, x, brute, table)
    assert compared > 3000 * len(igc.entries(flavour))


def variant_batch(x, amino, table):
    """every variant string of every query (one_substitution_common.variants, in numpy: the batches have 10^5 to 10^6 of them)
    -> (query numbers, edits, chars, offsets)"""
    letters = np.frombuffer(lm.letters_of(amino), np.uint8)
    own = np.array(table, np.int64)
    m = np.diff(x.offsets).astype(np.int64)
    numbers, edits, rows = [], [], []
    for length in np.unique(m[m > 0]):
        which = np.flatnonzero(m == length)
        strings = x.chars[x.offsets[which].astype(np.int64)[:, None] + np.arange(length)[None, :]]  # (queries, length)
        q, p, c = np.meshgrid(np.arange(which.size), np.arange(length), np.arange(letters.size), indexing="ij")
        differs = own[strings[q, p]] != c
        q, p, c = q[differs], p[differs], c[differs]
        made = strings[q].copy()
        made[np.arange(q.size), p] = letters[c]
        numbers.append(which[q])
        edits.append(p * 32 + c)
        rows.append(made)
    lengths = np.concatenate([np.full(r.shape[0], r.shape[1], np.uint64) for r in rows])
    offsets = np.zeros(lengths.size + 1, np.uint64)
    np.cumsum(lengths, out=offsets[1:])
    return np.concatenate(numbers), np.concatenate(edits), np.concatenate([r.reshape(-1) for r in rows]), offsets


def check_one_substitution(e, x, brute, table):
    """the pattern of tests/test_one_substitution.py: the records are exactly the edited strings that occur, each with the range
    of the single-string search of that string -- here the oracle's, in one batch; the strings of the records of pure queries
    go through the brute force as well (an edited string of at most 8 characters that occurs is a substring of the text, hence
    a query of the batch itself, checked against the brute force as such)"""
    queries, edits, ranges, total, variants, occurrences = x.one_substitution[True]
    numbers, made_edits, chars, offsets = variant_batch(x, e.amino, table)
    sp, ep, _, _ = x.oracle_index.batch_search(chars, offsets)
    occurs = sp <= ep
    want = set(zip(numbers[occurs].tolist(), made_edits[occurs].tolist(), sp[occurs].tolist(), ep[occurs].tolist()))
    exact = np.flatnonzero((x.sp <= x.ep) & (np.diff(x.offsets) > 0))
    want_exact = set(zip(exact.tolist(), [osc.EDIT_NONE] * exact.size, x.sp[exact].tolist(), x.ep[exact].tolist()))
    records = osc.as_set(queries, edits, ranges)
    assert records == want | want_exact, (e, sorted(records - want - want_exact)[:5], sorted((want | want_exact) - records)[:5])
    assert total == len(records)
    v, o = osc.per_query(records, len(x.queries))
    assert np.array_equal(variants, v) and np.array_equal(occurrences, o), e
    letters = lm.letters_of(e.amino)
    checked = 0
    for query, edit, a, b in records:
        if not x.pure[query]:
            continue
        s = x.queries[query]
        if edit != osc.EDIT_NONE:
            p, c = edit >> 5, edit & 31
            assert table[s[p]] != c, (e, s, edit)
            s = s[:p] + letters[c:c + 1] + s[p + 1:]
        assert brute.match(s) == (len(s), (a, b)), (e, x.queries[query], edit)
        checked += 1
    assert checked > 1000
    # include_exact off: the same records without the unedited queries
    off = x.one_substitution[False]
    assert osc.as_set(*off[:3]) == want and off[3] == len(want), e
    v, o = osc.per_query(want, len(x.queries))
    assert np.array_equal(off[4], v) and np.array_equal(off[5], o), e


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_step_walk_of_the_queries_that_are_not_pure(awfm, oracle, flavour):
    from avxwindowfmindex_amd import _lib
    lib = _lib.lib()
    walked = 0
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)
        lengths, ranges, _ = x.longest[0]
        for i, q in enumerate(x.queries):
            if x.pure[i]:
                continue
            length, (sp, ep) = lm.step_walk(lib, x.index, q)
            assert (int(lengths[i]), int(ranges[i, 0]), int(ranges[i, 1])) == (length, sp, ep), (e, q)
            if length == len(q) and q:
                assert (int(x.sp[i]), int(x.ep[i])) == (sp, ep), (e, q)
            else:
                assert int(x.sp[i]) > int(x.ep[i]), (e, q)
            walked += 1
    assert walked > 100 * len(igc.entries(flavour))


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_the_compiled_reference_walks_to_the_same_ranges(awfm, oracle, ref, flavour):
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)
        ri = ref.Index.from_text(e.text, x.alphabet, x.ratio, x.seed_k)
        assert ri.bwt_length == e.L
        walk = [lm.step_walk(ref.lib(), ri, q) for q in x.queries]
        for min_length in (3, 0):
            want = rc.longest_match_expected(walk, min_length)
            for k in range(3):
                assert np.array_equal(x.longest[min_length][k], want[k]), (e, min_length, k)
        whole = np.array([w[0] == len(q) and len(q) > 0 for w, q in zip(walk, x.queries)])
        assert np.array_equal(np.stack([x.sp, x.ep], axis=1)[whole], want[1][whole]) and (x.sp[~whole] > x.ep[~whole]).all(), e
        ri.free()


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_every_row_locates_to_the_suffix_array_of_a_plain_sort(awfm, oracle, flavour):
    from avxwindowfmindex_amd import _lib
    lib = _lib.lib()
    code = C.c_int(0)
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)
        assert np.array_equal(np.sort(x.suffix_array), np.arange(e.L, dtype=np.uint64))
        rows = np.arange(e.L, dtype=np.uint64)
        ending = [len(igc.walks_that_end_on_the_sentinel(x, ratio)) for ratio in igc.RATIOS]
        assert ending[0] == 0 and max(ending) > 0, (e, ending)  # at some ratio, walks step onto the sentinel's row and end there
        for ratio in igc.RATIOS:
            oi = oracle.Index.from_text(e.text, x.alphabet, ratio, x.seed_k)
            _, positions, _ = oi.batch_locate(rows, rows)
            assert np.array_equal(positions, x.suffix_array), (e, ratio, "oracle")
            hi = awfm.create_index(e.text, x.alphabet, ratio, x.seed_k)
            got = [lib.awFmFindDatabaseHitPositionSingle(hi.ptr, int(p), C.byref(code)) for p in rows]
            assert np.array_equal(np.array(got, np.uint64), x.suffix_array), (e, ratio, "host")
            hi.dealloc()
        # the located hits of the batch: the rows of every range, in order
        want = np.concatenate([x.suffix_array[int(a):int(b) + 1] for a, b in zip(x.sp, x.ep) if a <= b])
        assert np.array_equal(x.positions, want), e
