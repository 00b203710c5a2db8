"""tests/locate_chain_common.py, the host model of the stage from ranges to positions, pinned: by values worked out by hand, by
the oracle's batch_locate on a searched batch (the model's "hit order" is the product's), and by the thresholds it mirrors,
read again out of csrc/awfm_gpu_locate.hip and csrc/awfm_gpu_ordered.hip -- a retuned kernel fails here, before it moves out
from under tests/test_gpu_locate_chain.py."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_chain_common as lc  # noqa: E402

from avxwindowfmindex_amd import synth  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avxwindowfmindex_amd", "csrc")
SA = np.array([50, 40, 30, 20, 10, 0, 60, 70], np.uint64)  # a "suffix array" for the hand values
P = lc.PATTERN64


def u64(*values):
    return np.array(values, np.uint64)


def test_empty_batch_and_one_range():
    assert lc.lengths(np.zeros((0, 2), np.uint64)).size == 0
    assert lc.offsets(u64()).tolist() == [0]
    assert lc.window(SA, np.zeros((0, 2), np.uint64), u64(0), 0, 0, 0, 0).size == 0
    r = u64(3, 5).reshape(1, 2)
    assert lc.lengths(r).tolist() == [3]
    off = lc.offsets(lc.lengths(r))
    assert off.tolist() == [0, 3]
    assert lc.window(SA, r, off, 0, 1, 0, 3).tolist() == [20, 10, 0]
    assert lc.window(SA, r, off, 0, 1, 0, 5).tolist() == [20, 10, 0, P, P]  # behind the hits: untouched


def test_every_empty_form_has_length_zero():
    r = u64(1, 0, 5, 4, 0, lc.MASK64, 0, 0, 7, 7, lc.MASK64, lc.MASK64, 2, 1).reshape(-1, 2)
    assert lc.lengths(r).tolist() == [0, 0, 0, 1, 1, 1, 0]  # {0, 2^64 - 1}: sp <= ep and the length wraps to 0
    assert [lc.empty_range(f, sp=5) for f in range(3)] == [(1, 0), (5, 4), (0, lc.MASK64)]
    assert lc.offsets(lc.lengths(r)).tolist() == [0, 0, 0, 0, 1, 2, 3, 3]


def test_offsets_stay_exact_beyond_32_bits():
    lens = np.full(40000, 1 << 17, np.uint64)
    off = lc.offsets(lens)
    assert int(off[32768]) == 1 << 32 and int(off[-1]) == 40000 << 17 == lc.exact_total(lens)
    assert lc.exact_total(u64(lc.MASK64 >> 2, lc.MASK64 >> 2, 5)) == 2 * (lc.MASK64 >> 2) + 5
    with pytest.raises(AssertionError):
        lc.offsets(u64(1 << 62, 1 << 62))


def test_a_window_that_begins_and_ends_inside_one_list():
    r = u64(2, 6, 1, 0, 0, 1).reshape(-1, 2)  # lists of 5, 0 and 2 hits: hits 0..4 = SA[2..6], hits 5, 6 = SA[0..1]
    off = lc.offsets(lc.lengths(r))
    assert off.tolist() == [0, 5, 5, 7]
    assert lc.window(SA, r, off, 0, 3, 1, 4).tolist() == [20, 10, 0]
    assert lc.window(SA, r, off, 0, 3, 0, 7).tolist() == [30, 20, 10, 0, 60, 50, 40]
    assert lc.window(SA, r, off, 0, 3, 4, 6).tolist() == [60, 50]
    assert lc.window(SA, r, off, 1, 3, 3, 7).tolist() == [P, P, 50, 40]  # the first k-mer is not among the queries
    assert lc.window(SA, r, off, 0, 1, 3, 7).tolist() == [0, 60, P, P]
    assert lc.covered(off, 0, 1, 1, 4) and lc.covered(off, 2, 3, 5, 7) and not lc.covered(off, 1, 3, 3, 7) and not lc.covered(off, 0, 1, 3, 7)
    assert not lc.covered(off, 0, 3, 5, 8)  # beyond the total
    assert {c[1:] for c in lc.window_cases(off)} >= {(0, 3, 0, 7), (0, 1, 0, 1), (2, 3, 5, 6), (0, 3, 4, 7), (0, 1, 1, 3)}


def test_list_tail_by_hand():
    kmers = np.array([9, 4, 7, lc.NO_KMER], np.uint32)
    ranges = u64(0, 1, 5, 5, 2, 4, 1, 0).reshape(-1, 2)  # k-mer 9: SA[0..1], 4: SA[5], 7: SA[2..4]
    k, r, off, pos = lc.list_tail(SA, kmers, ranges, 3, 4, 8)
    assert k.tolist() == [4, 7, 9, lc.NO_KMER] and r.tolist() == [[5, 5], [2, 4], [0, 1], [1, 0]]
    assert off.tolist() == [0, 1, 4, 6, 6] and pos.tolist() == [0, 30, 20, 10, 50, 40, P, P]
    # the position buffer ends inside the second entry
    assert lc.list_tail(SA, kmers, ranges, 3, 4, 3)[3].tolist() == [0, 30, 20]
    assert lc.list_tail(SA, kmers, ranges, 3, 4, 0)[3].size == 0
    # more hits than the list holds: the first `cap` entries stored, in k-mer order; nothing behind them
    k, r, off, pos = lc.list_tail(SA, kmers, ranges, 5, 2, 4)
    assert k.tolist() == [4, 9] and r.tolist() == [[5, 5], [0, 1]] and off.tolist() == [0, 1, 3] and pos.tolist() == [0, 50, 40, P]
    # no entries
    k, r, off, pos = lc.list_tail(SA, kmers, ranges, 0, 3, 2)
    assert k.tolist() == [lc.NO_KMER] * 3 and r.tolist() == [[1, 0]] * 3 and off.tolist() == [0] * 4 and pos.tolist() == [P, P]


def test_sorts_by_hand():
    kmers = np.array([9, 4, 7, 1, lc.NO_KMER], np.uint32)
    ranges = u64(0, 1, 5, 5, 2, 4, 3, 3, 1, 0).reshape(-1, 2)
    k, r = lc.sort_on_device(kmers, ranges, 3, 5)
    assert k.tolist() == [4, 7, 9, 1, lc.NO_KMER] and r.tolist() == [[5, 5], [2, 4], [0, 1], [3, 3], [1, 0]]
    k, r = lc.sort_on_device(kmers, ranges, 7, 4)  # count > cap
    assert k.tolist() == [1, 4, 7, 9, lc.NO_KMER] and r[0].tolist() == [3, 3]
    k, r = lc.sort_on_host(kmers[::-1], ranges[::-1], 5)
    assert k.tolist() == [1, 4, 7, 9, lc.NO_KMER] and r[-1].tolist() == [1, 0]
    assert kmers.tolist() == [9, 4, 7, 1, lc.NO_KMER]  # the inputs stay


def test_branches_by_hand():
    assert [lc.entry_branch(h) for h in (0, 1, 32, 33, 4096, 4097)] == ["none", "lane", "lane", "wave", "wave", "workgroup"]
    assert lc.entry_branch(5000, huge_slot_free=False) == "wave"
    assert [lc.scan_path(n) for n in (1, 1024, 1025, 16384, 16385, 1 << 20, (1 << 20) + 1, 1 << 24, (1 << 24) + 1)] == [
        "one-tile", "one-tile", "small", "small", "two-level-tile", "two-level-tile", "two-level-small", "two-level-small", "three-level"]
    assert lc.expand_kernel(640, 10, True) == "long" and lc.expand_kernel(639, 10, True) == "hits" and lc.expand_kernel(640, 10, False) == "hits"
    assert [lc.sort_path(n) for n in (1, 4096 * 1024, 4096 * 1024 + 1)] == ["rank-scan-one-trip", "rank-scan-one-trip", "rank-scan-carry"]
    c = lc.ListCase("by hand", (), 1 << 20, 64, 3, [5, 700000, 6], [40, 9000, 3], cut=("inside", "workgroup"))
    assert c.capacity_hits() == 43 + 4500  # in k-mer order: 40, 3, 9000 hits; half of the huge entry
    got = lc.list_tail_branches(c)
    assert {"grid=capacity/16", "cut-huge", "one-launch", "slots", "keys-vector", "all-ranges"} <= got and "sub-ranges" not in got


def test_coverage_is_asserted_for_every_threshold():
    lc.check_coverage()
    assert lc.SCAN_SIZES == [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, (1 << 20) - 1, 1 << 20, (1 << 20) + 1,
                             (1 << 24) - 1, 1 << 24, (1 << 24) + 1]
    assert set(lc.ENTRY_HITS) >= {0, 1, 31, 32, 33, 63, 64, 65, 4096, 4097, 16383, 16384, 16385, 4 * 16384}
    assert {c.cap for c in lc.list_cases()} >= {1, 15, 16, 17, 16384, 16385, 1 << 18, (1 << 18) + 1}
    assert lc.SORT_QUERIES == [4096, 4097, 4194304, 4194305, 2 * 4194304 + 1]
    with pytest.raises(AssertionError):  # a machine on which the hand-made lists would miss their branches is noticed
        lc.check_coverage(num_cus=8)


def test_model_hit_order_is_the_oracle_s(oracle):
    txt = synth.text(5, 3000, synth.DNA_ALPHABET).copy()
    txt[100:160] = np.frombuffer(b"acg" * 20, np.uint8)  # lists of many hits
    txt[[7, 2000]] = ord("n")
    oi = oracle.Index.from_text(txt.tobytes(), oracle.DNA, 4, 4)
    sa = oi.full_sa()
    assert sa.size == len(txt) + 1 and np.array_equal(np.sort(sa), np.arange(sa.size))
    q = [bytes(txt[o:o + 9]) for o in (0, 50, 500, 2990)] + [b"acgacg", b"cg", b"ttttttttttttt", b"a", b"gacga", b"nn"]
    sp, ep, cnt, _ = oi.search_list(q, threads=1)
    ranges = np.stack((sp, ep), axis=1)
    lens = lc.lengths(ranges)
    assert np.array_equal(lens, cnt.astype(np.uint64)) and (lens == 0).any() and int(lens.max()) > 64
    hit_off, pos, _ = oi.batch_locate(sp, ep, threads=1)
    off = lc.offsets(lens)
    assert np.array_equal(off, hit_off)
    total = int(off[-1])
    assert np.array_equal(lc.window(sa, ranges, off, 0, len(q), 0, total), pos)
    for name, qb, qe, hb, he in lc.window_cases(off):
        assert np.array_equal(lc.window(sa, ranges, off, qb, qe, hb, he), pos[hb:he]), name
    # ... and a list of them
    kmers = np.flatnonzero(cnt > 0)[::-1].astype(np.uint32)
    k, r, loff, lpos = lc.list_tail(sa, kmers, ranges[kmers], kmers.size, kmers.size + 2, total)
    assert np.array_equal(k[:kmers.size], kmers[::-1]) and np.array_equal(lpos, pos) and int(loff[-1]) == total


def _constant(source, name):
    found = re.findall(rf"\b{name}\s*=\s*([^,;]+)[,;]", source)
    assert len(found) == 1, (name, found)
    return int(eval(re.sub(r"(?<=\d)(ull|u)\b", "", found[0]), {"__builtins__": {}}))


def test_mirrored_thresholds_are_the_sources():
    with open(os.path.join(CSRC, "awfm_gpu_locate.hip")) as f:
        locate = f.read()
    with open(os.path.join(CSRC, "awfm_gpu_ordered.hip")) as f:
        ordered = f.read()
    want = dict(kScanThreads=lc.SCAN_THREADS, kScanItems=lc.SCAN_ITEMS, kScanSmallThreads=lc.SCAN_SMALL_THREADS, kScanSmallItems=lc.SCAN_SMALL_ITEMS,
                kLongChunk=lc.LONG_CHUNK, kLongStage=lc.LONG_STAGE, kListTailThreads=lc.LIST_TAIL_THREADS, kListTailSlots=lc.LIST_TAIL_SLOTS,
                kListTailMaxEntries=lc.LIST_TAIL_MAX_ENTRIES, kHuge=lc.HUGE, kHugeSlots=lc.HUGE_SLOTS, kPer=8, kGroups=2)
    for name, value in want.items():
        assert _constant(locate, name) == value, name
    assert _constant(ordered, "kRankBlockWords") == lc.RANK_BLOCK_WORDS
    assert lc.LIST_TAIL_PER_TRIP == lc.LIST_TAIL_THREADS * 8 * 2 and lc.RANK_BLOCK == 64 * lc.RANK_BLOCK_WORDS
    assert "kScanTile = kScanThreads * kScanItems" in locate and "kScanSmall = kScanSmallThreads * kScanSmallItems" in locate
    # the literals: lane or wave (both kernels), the rule that picks the expand kernel, its unrolled loop, the list tail's choices
    assert re.findall(r"isLong = count > (\d+)ull;", locate) == [str(lc.LANE_MAX)]
    assert re.findall(r"isLong = countHere > (\d+)ull && !isHuge;", locate) == [str(lc.LANE_MAX)]
    assert re.findall(r"totalHits < (\d+)ull \* numQueries", locate) == [str(lc.LONG_RULE)]
    assert re.findall(r"__launch_bounds__\((\d+)\)\s+expandLongKernel", locate) == [str(lc.LONG_THREADS)]
    assert re.findall(r"for \(; h \+ (\d+)ull < hi; h \+= (\d+)ull\)", locate) == [(str(lc.LONG_UNROLL), str(4 * lc.LONG_THREADS))]
    assert re.findall(r"allRanges = cap <= (\d+)u;", locate) == [str(lc.LIST_TAIL_ALL_RANGES)]
    assert re.findall(r"unsigned grid = capacity / (\d+)u;", locate) == [str(lc.LIST_TAIL_GRID_DIVISOR)]
    assert re.findall(r"__launch_bounds__\((\d+)\) rankBlockScanKernel", ordered) == [str(lc.RANK_SCAN_THREADS)]
    assert re.findall(r"base < numBlocks; base \+= (\d+)u\)", ordered) == [str(lc.RANK_SCAN_THREADS)]


def _bitmap_ranks(kmers, num_queries, carry):
    """the rank of every listed k-mer as the bitmap sort forms it: listed k-mers per block of RANK_BLOCK, the blocks' exclusive
    sums in trips of RANK_SCAN_THREADS with a carry from trip to trip (carry=False: a scan that forgot it), the listed k-mers
    below it in its own block"""
    k = np.asarray(kmers, np.int64)
    blocks = -(-num_queries // lc.RANK_BLOCK)
    counts = np.bincount(k // lc.RANK_BLOCK, minlength=blocks)
    start, carried = np.zeros(blocks, np.int64), 0
    for base in range(0, blocks, lc.RANK_SCAN_THREADS):
        trip = counts[base:base + lc.RANK_SCAN_THREADS]
        start[base:base + trip.size] = carried + np.cumsum(trip) - trip
        carried = carried + int(trip.sum()) if carry else 0
    order = np.argsort(k)
    below = np.empty(k.size, np.int64)
    below[order] = np.arange(k.size) - (np.cumsum(counts) - counts)[k[order] // lc.RANK_BLOCK]
    return start[k // lc.RANK_BLOCK] + below


@pytest.mark.parametrize("num_queries", lc.SORT_QUERIES)
def test_sort_entries_tell_a_scan_without_its_carry(num_queries):
    """the lists of the sort test are such that a block scan that lost its carry between trips would put them in another order
    exactly where there is more than one trip"""
    kmers = lc.sort_entries(num_queries)
    want = np.empty(kmers.size, np.int64)
    want[np.argsort(kmers)] = np.arange(kmers.size)
    assert np.array_equal(_bitmap_ranks(kmers, num_queries, carry=True), want)
    several_trips = lc.sort_path(num_queries) == "rank-scan-carry"
    assert np.array_equal(_bitmap_ranks(kmers, num_queries, carry=False), want) == (not several_trips)
