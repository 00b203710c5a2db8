"""The reference itself against the oracle and the host library, live on the CPU.

oracle/_ref/libawfm_ref.so is the reference's src directory compiled where it lies (oracle/Makefile, oracle/ref_shim); this
module compares, wherever all three exist: reference, oracle (oracle/awfm_oracle.c) and host library (awfm_build.c,
awfm_search_host.c, awfm_file.c, awfm_sa.c, awfm_letters.c).  Where the reference's sources are present a missing
library is a failure; the module may skip only where neither the library nor the sources exist.

What the comparison found about the reference, and what this module therefore leaves out: for amino acids the
reference's sanitiser (src/AwFmLetter.c, awFmAsciiAminoLetterSanitize) turns only b, x and NUL into the ambiguity letter
and keeps every other byte as it is, case included, while its letter indexes ignore case and give every non-letter the
ambiguity index.  The suffix array is then sorted by raw bytes ('W' before 'a', '7' before everything, 'j' between 'i'
and 'k') and the BWT is read through the case-blind indexes, so an amino text of mixed case, or one with non-letters
other than b / x / NUL, gets an index whose LF mapping is not a permutation: rows 29 -> 143 -> 251 -> 29 form a cycle
in the mixed-case text of 256 characters below, and a locate from them never ends -- in the reference, in the oracle and
in the host library alike, which build that index byte for byte like the reference (the nucleotide sanitiser lowers
case and has no such effect).  Search ranges on such an index run past the BWT (the reference and the oracle both
ended in a segmentation fault on the all-ambiguous amino text).  For these three amino text kinds (ILL_FORMED_AMINO) the
module compares the construction, which is well defined and equal in all three, and nothing that walks the index.
Empty texts and empty queries are left out as well (clz(0) and kmerLength - 1 in the reference).  Every test runs under
a watchdog as a last resort against such inputs: after 600 s in one test it prints a traceback and ends the whole pytest
process, the results of the other modules with it, instead of hanging the suite for ever."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

import longest_match_common as lm
import reference_common as rc
from oracle import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def watchdog():
    """the reference has inputs on which it does not return (module docstring): no test of this module may hang the suite.
    It ends the pytest process, not just the test."""
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


def three(ref, oracle, awfm, text, amino, ratio, k, **kw):
    alpha = 1 if amino else 2
    return (ref.Index.from_text(text, alpha, ratio, k), oracle.Index.from_text(text, alpha, ratio, k),
            awfm.create_index(np.frombuffer(text, np.uint8), alpha, ratio, k, **kw))


def assert_same_index(ri, oi, hi, tag):
    """blocks, prefix sums, seed table byte-equal; the suffix array equal in its payload bytes and in its decoded samples"""
    for name in ("blocks", "prefix_sums", "seed_table"):
        a = getattr(ri, name)()
        assert np.array_equal(a, getattr(oi, name)()), (tag, name, "oracle")
        assert np.array_equal(a, getattr(hi, name)()), (tag, name, "host")
    n, ratio = ri.bwt_length, ri.sa_ratio
    payload = rc.sa_payload_bytes(n, ratio)
    pa, pb, pc = ri.packed_sa(), oi.packed_sa(), hi.packed_sa()
    assert len(pa) == len(pb) == len(pc) == payload + rc.SA_PAD_BYTES, tag
    assert ri.sa_width == hi.sa_width == max(1, (n - 1).bit_length()), tag
    assert np.array_equal(pa[:payload], pb[:payload]) and np.array_equal(pa[:payload], pc[:payload]), (tag, "sa payload")
    want = oi.full_sa()[::ratio]
    assert np.array_equal(rc.sa_samples(pa, n, ratio), want), (tag, "samples")


ILL_FORMED_AMINO = ("mixed-case", "all-ambiguous", "foreign-bytes")  # see the module docstring


def index_is_well_formed(amino, kind):
    return not (amino and kind in ILL_FORMED_AMINO)


# ---- a. the committed goldens have reference provenance ----
def golden_cases():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_golden
    return make_golden


@pytest.mark.parametrize("case_number", range(7))
def test_goldens_are_what_the_reference_computes(ref, oracle, case_number):
    mg = golden_cases()
    case = mg.CASES[case_number]
    name, alpha, _, n, ratio, k = case[:6]
    txt, chars, offsets = mg.build_case(case)
    g = np.load(os.path.join(rc.GOLDEN_DIR, name + ".npz"))
    ri = ref.Index.from_text(txt.tobytes(), 1 if alpha == "amino" else 2, ratio, k)
    sp, ep, cnt, _ = ri.batch_search(chars, offsets)
    hit_off, pos, code = ri.batch_locate(chars, offsets, 4)
    assert code == 1
    assert np.array_equal(sp, g["sp"]) and np.array_equal(ep, g["ep"]) and np.array_equal(cnt, g["count"])
    assert np.array_equal(hit_off, g["hit_offsets"]) and np.array_equal(pos, g["positions"])
    assert np.array_equal(ri.prefix_sums(), g["prefix_sums"]) and ri.bwt_length == int(g["bwt_length"])
    digests = g["digests"]
    assert oracle.fnv1a(ri.blocks()) == digests[0] and oracle.fnv1a(ri.prefix_sums()) == digests[1]
    assert oracle.fnv1a(ri.seed_table()) == digests[2]
    # the suffix array: the golden digest covers the oracle's bytes (zero padding); the reference's equal them in the payload
    packed = ri.packed_sa()
    payload = rc.sa_payload_bytes(ri.bwt_length, ratio)
    zero_padded = packed.copy()
    zero_padded[payload:] = 0
    assert oracle.fnv1a(zero_padded) == digests[3]
    ri.free()


# ---- b + c. construction grid and batch search ----
LENGTHS = (254, 255, 256, 257, 511, 512, 513, 767, 768, 769, 2600, 5003)
RATIOS = (1, 2, 3, 8, 16, 200, 255)


def grid():
    """the cross product alphabet x text kind x length x ratio x seed length, sampled with a fixed seed: every value of
    every axis occurs, every (alphabet, kind) pair occurs at least four times"""
    rng = np.random.default_rng(20260)
    out = []
    for amino in (False, True):
        seeds = (1, 2, 3) if amino else (1, 2, 3, 4, 5, 6, 7, 8)
        for kind in rc.TEXT_KINDS:
            for i in range(7):
                n = LENGTHS[int(rng.integers(0, len(LENGTHS)))] if i >= 2 else LENGTHS[(len(out) * 5 + i) % len(LENGTHS)]
                ratio = RATIOS[(len(out) + i) % len(RATIOS)]
                k = seeds[(len(out) + i) % len(seeds)]
                if k >= 7 or (amino and k == 3):
                    n = min(n, 769)  # seed tables of 4^7, 4^8, 20^3 entries: keep the table the dominant cost only briefly
                out.append((amino, kind, n, ratio, k))
    return out


GRID = grid()


def test_grid_covers_every_axis_value():
    assert {g[2] for g in GRID} == set(LENGTHS) and {g[3] for g in GRID} == set(RATIOS)
    assert {g[4] for g in GRID if not g[0]} == set(range(1, 9)) and {g[4] for g in GRID if g[0]} == {1, 2, 3}
    assert {(g[0], g[1]) for g in GRID} == {(a, k) for a in (False, True) for k in rc.TEXT_KINDS}


@pytest.mark.parametrize("amino,kind,n,ratio,k", GRID, ids=lambda v: str(v))
def test_construction_and_batch_search(ref, oracle, awfm, amino, kind, n, ratio, k):
    rng = np.random.default_rng([n, ratio, k, int(amino)])
    text = rc.make_text(kind, rng, n, amino)
    tag = (amino, kind, n, ratio, k)
    ri, oi, hi = three(ref, oracle, awfm, text, amino, ratio, k)
    assert ri.bwt_length == oi.bwt_length == hi.bwt_length == n + 1
    assert_same_index(ri, oi, hi, tag)
    if not index_is_well_formed(amino, kind):
        ri.free()
        hi.dealloc()
        return
    queries = rc.make_queries(rng, text, amino, k, 3000)
    chars, offsets = rc.pack(queries)
    for threads in (1, 4):
        rsp, rep, rcnt, _ = ri.batch_search(chars, offsets, threads)
        osp, oep, ocnt, _ = oi.batch_search(chars, offsets, threads)
        bad = np.flatnonzero((rsp != osp) | (rep != oep))
        assert bad.size == 0, (tag, threads, [(queries[i], rsp[i], rep[i], osp[i], oep[i]) for i in bad[:3]])
        assert np.array_equal(rcnt, ocnt), (tag, threads)
        rho, rpos, code = ri.batch_locate(chars, offsets, threads)
        oho, opos, _ = oi.batch_locate(osp, oep, threads)
        assert code == 1 and np.array_equal(rho, oho) and np.array_equal(rpos, opos), (tag, threads)
    ri.free()
    hi.dealloc()


# ---- d. single-query and step functions ----
@pytest.mark.parametrize("amino,kind,n,ratio,k", [(False, "ambiguity-runs", 700, 3, 3), (False, "foreign-bytes", 513, 8, 2),
                                                   (False, "two-letter", 600, 2, 4), (True, "ambiguity-runs", 700, 3, 2),
                                                   (True, "upper", 512, 16, 1)], ids=lambda v: str(v))
def test_single_query_and_step_functions(ref, oracle, awfm, amino, kind, n, ratio, k):
    from avxwindowfmindex_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n + k)
    text = rc.make_text(kind, rng, n, amino)
    ri, oi, hi = three(ref, oracle, awfm, text, amino, ratio, k)
    queries = rc.make_queries(rng, text, amino, k, 600)
    host_step = L.awFmAminoIterativeStepBackwardSearch if amino else L.awFmNucleotideIterativeStepBackwardSearch
    host_prev = L.awFmAminoBacktraceReturnPreviousLetterIndex if amino else L.awFmNucleotideBacktraceReturnPreviousLetterIndex
    for q in queries:
        want = ri.range_for_string(q)
        assert want == oi.range_for_string(q) == hi.find_search_range_for_string(q), q
        a = L.awFmCreateInitialQueryRange(hi.ptr, q, len(q))
        assert ri.initial_range(q) == (a.startPtr, a.endPtr), q
        b = L.awFmCreateInitialQueryRangeFromChar(hi.ptr, q[-1:])
        assert ri.initial_range_from_char(q[-1:]) == (b.startPtr, b.endPtr), q
    # steps from valid and from already-empty ranges, every letter index the alphabet has (ambiguity included)
    n_letters = 21 if amino else 5
    starts = [ri.initial_range_from_char(bytes([c])) for c in rc.letters_of(amino)] + [(1, n), (5, 4), (n, 1), (1, 0), (n + 1, n)]
    for q in queries[:150]:
        starts.append(ri.range_for_string(q))
    for sp, ep in starts:
        for letter in range(n_letters):
            want = ri.step(sp, ep, letter)
            r = _lib.AwFmSearchRange(sp, ep)
            host_step(hi.ptr, C.byref(r), letter)
            assert (r.startPtr, r.endPtr) == want, (sp, ep, letter, "host")
            assert oi.step(sp, ep, letter) == want, (sp, ep, letter, "oracle")
    # every BWT position: its text position and its previous letter
    code = C.c_int(0)
    for p in range(n + 1):
        want = ri.locate_one(p)
        assert L.awFmFindDatabaseHitPositionSingle(hi.ptr, p, C.byref(code)) == want == oi.locate_one(p), p
        pos = C.c_uint64(p)
        letter = host_prev(hi.ptr, C.byref(pos))
        assert (letter, pos.value) == ri.previous_letter(p), p
    ri.free()
    hi.dealloc()


# ---- e. longest suffix match against the walk over the reference's own step functions ----
@pytest.mark.parametrize("name", ["random", "two-letter", "n-runs", "amino"])
def test_longest_suffix_matches_equal_the_reference_step_walk(ref, awfm, name):
    from avxwindowfmindex_amd import _lib
    text, amino = lm.small_texts()[name]
    alpha = 1 if amino else 2
    ri = ref.Index.from_text(text, alpha, 4, 2 if amino else 4)
    hi = awfm.create_index(np.frombuffer(text, np.uint8), alpha, 4, 2 if amino else 4)
    queries = [q for q, _ in lm.make_queries(np.random.default_rng(5), text, amino, 400)]
    walk = [lm.step_walk(ref.lib(), ri, q) for q in queries]
    assert walk == [lm.step_walk(_lib.lib(), hi, q) for q in queries]
    chars, starts, ends = lm.pack(queries)
    for min_length in (0, 1, 2, 12, 33):
        lengths, ranges, counts = awfm.longest_suffix_matches_host(hi, chars, starts, ends, min_length=min_length)
        want = rc.longest_match_expected(walk, min_length)
        assert np.array_equal(lengths, want[0]) and np.array_equal(ranges, want[1]) and np.array_equal(counts, want[2]), min_length
    for q, w in zip(queries, walk):
        if len(q) and w[0] == len(q):  # the whole query occurs: its range is the search range
            assert ri.range_for_string(q) == w[1] == hi.find_search_range_for_string(q)
    ri.free()
    hi.dealloc()


# ---- f. files, both directions ----
@pytest.mark.parametrize("amino,n,ratio,k", [(False, 3000, 8, 4), (False, 1300, 3, 3), (True, 2000, 1, 2), (True, 5000, 8, 1)])
def test_files_travel_both_ways(ref, awfm, tmp_path, amino, n, ratio, k):
    from avxwindowfmindex_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    text = rc.make_text("ambiguity-runs", rng, n, amino)
    alpha = 1 if amino else 2
    queries = rc.make_queries(rng, text, amino, k, 300)
    code = C.c_int(0)
    for store in (False, True):
        ref_path, own_path = str(tmp_path / f"ref{int(store)}.awfmi"), str(tmp_path / f"own{int(store)}.awfmi")
        ri = ref.Index.from_text(text, alpha, ratio, k, file_src=ref_path, store_sequence=store)
        hi = awfm.create_index(np.frombuffer(text, np.uint8), alpha, ratio, k, store_sequence=store, file_src=own_path)
        # the byte relation of the two writers' files: equal everywhere except inside the final 8 padding bytes of the
        # suffix-array section, which ends the file
        a, b = open(ref_path, "rb").read(), open(own_path, "rb").read()
        assert len(a) == len(b)
        assert a[:-rc.SA_PAD_BYTES] == b[:-rc.SA_PAD_BYTES]
        assert b[-rc.SA_PAD_BYTES:] == bytes(rc.SA_PAD_BYTES)  # the host writer's padding is zero
        want_pos = ri.locate_all()
        # reference writes -> product reads
        for keep in (True, False):
            back = awfm.read_index_from_file(ref_path, keep_sa_in_memory=keep)
            for name in ("blocks", "prefix_sums", "seed_table"):
                assert np.array_equal(getattr(back, name)(), getattr(ri, name)()), name
            if keep:
                assert np.array_equal(back.packed_sa(), ri.packed_sa())  # the reference's padding bytes included
            for q in queries:
                assert back.find_search_range_for_string(q) == ri.range_for_string(q), q
            got = [L.awFmFindDatabaseHitPositionSingle(back.ptr, p, C.byref(code)) for p in range(n + 1)]
            assert np.array_equal(np.array(got, np.uint64), want_pos), keep
            buf = C.create_string_buffer(41)
            got_rc = L.awFmReadSequenceFromFile(back.ptr, 7, 40, buf)
            want_rc, want_seq = ri.read_sequence(7, 40)
            assert got_rc == want_rc
            if store:
                assert got_rc == awfm.AwFmFileReadOkay and buf.raw[:40] == want_seq == text[7:47]
            back.dealloc()
        # product writes -> reference reads
        for keep in (True, False):
            back = ref.Index.from_file(own_path, keep)
            for name in ("blocks", "prefix_sums", "seed_table"):
                assert np.array_equal(getattr(back, name)(), getattr(hi, name)()), name
            if keep:
                assert np.array_equal(back.packed_sa(), hi.packed_sa())
            for q in queries[:100]:
                assert back.range_for_string(q) == ri.range_for_string(q), q
            assert np.array_equal(back.locate_all(), want_pos), keep
            if store:
                assert back.read_sequence(7, 40) == (awfm.AwFmFileReadOkay, text[7:47])
            back.free()
        ri.free()
        hi.dealloc()


# ---- g. a file with non-zero bytes right behind the last sample ----
@pytest.mark.parametrize("amino,n,ratio,k", [(False, 1300, 1, 3), (False, 1300, 3, 3), (False, 5000, 8, 4), (False, 255, 3, 2),
                                             (True, 5000, 8, 1), (True, 1300, 3, 2), (False, 2047, 1, 2), (False, 700, 255, 2),
                                             # the last sample ends on a byte boundary and the BWT length is no power of two: the
                                             # first padding bit lies right behind it and a surplus bit survives the modulo
                                             (False, 1599, 1, 2), (True, 2399, 3, 1)])
def test_host_decoder_ignores_the_padding_bytes(ref, awfm, tmp_path, amino, n, ratio, k):
    """the reference leaves leftovers of the full suffix array in the padding; 0xFF there is as legal.  Every BWT position
    0 .. n located by the product from such a file, suffix array in memory and on disk, equals the reference's answer."""
    from avxwindowfmindex_amd import _lib
    L = _lib.lib()
    text = rc.make_text("random", np.random.default_rng(n + ratio), n, amino)
    ref_path = str(tmp_path / "ref.awfmi")
    ri = ref.Index.from_text(text, 1 if amino else 2, ratio, k, file_src=ref_path)
    want = ri.locate_all()
    assert np.array_equal(np.sort(want), np.arange(n + 1, dtype=np.uint64))
    code = C.c_int(0)
    for byte in (0xFF, 0x00, 0xA5):
        path = str(tmp_path / f"pad{byte:02x}.awfmi")
        open(path, "wb").write(rc.with_padding(open(ref_path, "rb").read(), byte))
        for keep in (True, False):
            back = awfm.read_index_from_file(path, keep_sa_in_memory=keep)
            got = [L.awFmFindDatabaseHitPositionSingle(back.ptr, p, C.byref(code)) for p in range(n + 1)]
            assert np.array_equal(np.array(got, np.uint64), want), (byte, keep)
            back.dealloc()
        # and the reference reading the same file
        back = ref.Index.from_file(path, True)
        assert np.array_equal(back.locate_all(), want), byte
        back.free()
    ri.free()


# ---- the fixtures the GPU suite uses are what the live reference says ----
def test_reference_fixtures_are_current(ref):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import make_reference_golden as mrg
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(rc.GOLDEN_DIR, "ref_*.npz")))
    assert names == sorted(c[0] for c in rc.FIXTURE_CASES)
    total = 0
    for case in rc.FIXTURE_CASES:
        path = os.path.join(rc.GOLDEN_DIR, case[0] + ".npz")
        size = os.path.getsize(path)
        assert size <= 256 * 1024, case[0]
        total += size
        have, fresh = np.load(path), mrg.record(case)
        assert sorted(have.files) == sorted(fresh), case[0]
        for key in fresh:
            assert np.array_equal(have[key], fresh[key]), (case[0], key)
    assert total <= 1024 * 1024
