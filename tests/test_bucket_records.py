"""The host model of the seed order's 8-byte records (tests/bucket_records_common.py) against figures worked out by hand,
against the codes of awfm.pack_kmers, and the fit rule at every k-mer length; and dist.py's bucket arithmetic (bucket_cuts /
merge_bucket_slices / full_bucket_start) where a rank gets no bucket with anything in it.  tests/test_gpu_bucket_records.py
holds the kernels to this model."""
import os
import sys

import numpy as np
import pytest

from avxwindowfmindex_amd import dist as shard

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bucket_records_common as br  # noqa: E402


def _kmers(*words):
    return np.array([np.frombuffer(w.encode(), np.uint8) for w in words])


# (k-mer, depth, bucket), by hand: the code string of the LAST `depth` letters, its leading min(11, 2 * depth) bits
HAND_BUCKETS = [
    ("a" * 21, 8, 0),
    ("t" * 21, 8, 2047),
    ("aaacgtacgt", 8, 216),           # acgtacgt = 00 01 10 11 00 01 10 11 = 6939; 16 - 11 = 5 bits dropped: 6939 >> 5
    ("tggggg", 5, 682),               # ggggg = 10 10 10 10 10: all 10 bits are the bucket's; the letter in front does not count
    ("acgt", 1, 3),
    ("ACGA", 1, 0),
    ("c", 1, 1),
    ("acgU", 1, 3),                   # u is t
    ("cccccc", 6, 682),               # 0101 0101 0101 = 1365; one bit dropped
    ("cccccg", 6, 683),               # 1366 >> 1
    ("ccccct", 6, 683),               # 1367 >> 1: the last letter's low bit is below the bucket's
    ("t" + "a" * 11, 12, 1536),       # 11 then 22 zero bits: the leading 11 bits are 110 0000 0000
    ("g" + "a" * 31, 10, 0),          # a 32-mer whose code string has bit 63 set: the bucket is that of aaaaaaaaaa
    ("c" + "a" * 31, 16, 0),          # ... and the one whose code string is bit 62 alone
    ("a" * 31 + "t", 16, 0),          # 30 zero bits, then 11: nothing of it in the leading 11 bits
    ("a" * 16 + "t" + "a" * 15, 16, 1536),
    ("acgtn", 1, -1),                 # a character outside acgtu anywhere: the general tail
    ("xcgta", 1, -1),
]


@pytest.mark.parametrize("word,depth,bucket", HAND_BUCKETS)
def test_bucket_of_a_kmer_by_hand(word, depth, bucket):
    assert br.bucket_of(_kmers(word), depth).tolist() == [bucket]


def test_shards_by_hand():
    # depth 1: four buckets, by the last letter
    q = _kmers("aa", "ac", "cg", "gt", "tn", "ca")
    assert br.expected_bucket_start(q, 1).tolist() == [0, 2, 3, 4, 5, 6, 1]
    per, tail = br.expected_numbers(q, 1, 100)
    assert per == {0: {100, 105}, 1: {101}, 2: {102}, 3: {103}} and tail == {104}
    # numbers at the top of the 32-bit range stay python integers
    per, tail = br.expected_numbers(q, 1, (1 << 32) - 2 - 6)
    assert per[3] == {(1 << 32) - 5} and tail == {(1 << 32) - 4}
    # a shard whose k-mers are all ambiguous; one in the last bucket only; one in a single bucket
    assert br.expected_bucket_start(_kmers("an", "nn", "xa"), 1).tolist() == [0, 0, 0, 0, 0, 3, 3]
    assert br.expected_bucket_start(_kmers("at", "tt", "gu"), 1).tolist() == [0, 0, 0, 0, 3, 3, 0]
    assert br.expected_bucket_start(_kmers("ac", "cc"), 1).tolist() == [0, 0, 2, 2, 2, 2, 0]
    # depth 2: 16 buckets by the last two letters (first of them most significant)
    start = br.expected_bucket_start(_kmers("aca", "ttt", "gac", "cac", "nac"), 2)
    assert start[[0, 1, 2, 15, 16, 17, 18]].tolist() == [0, 0, 2, 3, 4, 5, 1]
    assert start[1:16].tolist() == [0, 2, 2, 2] + [3] * 11  # ac = 1 (twice), ca = 4, tt = 15


def test_model_codes_are_those_of_pack_kmers():
    from avxwindowfmindex_amd import api
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"acgtACGTuU", np.uint8)
    for K in (1, 5, 16, 21, 31, 32):
        q = letters[rng.integers(0, len(letters), (257, K))]
        q[0], q[1] = ord("t"), ord("a")
        if K == 32:
            q[2] = np.frombuffer(b"c" + b"a" * 31, np.uint8)
            q[3] = np.frombuffer(b"g" + b"a" * 31, np.uint8)
        words = br.packed_words(q)
        assert np.array_equal(words, api.pack_kmers(q)), K
        assert int(words[0]) == (1 << (2 * K)) - 1 and int(words[1]) == 0
        if K == 32:
            assert int(words[2]) == 1 << 62 and int(words[3]) == 1 << 63
        for depth in sorted({1, min(5, K), min(16, K)}):
            # the bucket from the packed word: its low 2 * depth bits are the table index
            index = words & np.uint64((1 << (2 * depth)) - 1)
            assert np.array_equal((index >> np.uint64(2 * depth - br.bucket_bits(depth))).astype(np.int64), br.bucket_of(q, depth))


# the longest k-mer whose record fits, by hand: floor((64 + bucketBits - indexBits) / 2), at most 32
LONGEST = {
    1: {1: 32, 11: 27, 12: 27, 16: 25, 32: 17},    # 4 buckets: 2 bits
    5: {1: 32, 11: 31, 12: 31, 16: 29, 32: 21},    # 1024 buckets: 10 bits
    6: {1: 32, 11: 32, 12: 31, 16: 29, 32: 21},    # 2048 buckets from here on: 11 bits
    10: {1: 32, 11: 32, 12: 31, 16: 29, 32: 21},
    16: {1: 32, 11: 32, 12: 31, 16: 29, 32: 21},
}
TOTALS = {1: (1, 2), 11: (1025, 2048), 12: (2049, 4096), 16: (32769, 65536), 32: ((1 << 31) + 1, (1 << 32) - 2)}


@pytest.mark.parametrize("depth", sorted(LONGEST))
@pytest.mark.parametrize("bits", sorted(TOTALS))
def test_fit_rule_at_every_length(depth, bits):
    for total in TOTALS[bits]:
        assert br.index_bits(total) == bits
        for K in range(1, 33):
            expect = depth <= K <= LONGEST[depth][bits]
            assert br.fits(K, depth, total) == expect, (K, depth, total)
            assert br.buckets(K, depth, total) == ((1 << min(11, 2 * depth)) if expect else 0)
    for K in range(1, 33):  # the batch sizes themselves: 1 .. 2^32 - 2
        assert not br.fits(K, depth, 0) and not br.fits(K, depth, (1 << 32) - 1) and not br.fits(K, depth, 1 << 32)


def test_largest_total_is_the_last_that_fits():
    assert br.largest_total(32, 10) == 2048 and br.largest_total(32, 5) == 1024 and br.largest_total(32, 1) == 4
    assert br.largest_total(31, 1) == 16 and br.largest_total(21, 5) == (1 << 32) - 2 and br.largest_total(7, 8) == 0
    assert br.largest_total(27, 1) == 1 << 12 and br.largest_total(28, 1) == 1 << 10
    for depth in (1, 5, 6, 10, 16):
        for K in range(1, 33):
            top = br.largest_total(K, depth)
            if top == 0:
                assert not any(br.fits(K, depth, t) for t in (1, 2, 3, 1 << 16, (1 << 32) - 2))
                continue
            assert br.fits(K, depth, top) and br.fits(K, depth, 1)
            assert not br.fits(K, depth, top + 1)


def test_bucket_arithmetic_with_more_ranks_than_buckets_in_use():
    import torch
    buckets, world = 16, 8
    cuts = shard.bucket_cuts(buckets, world)
    assert cuts == [0, 2, 4, 6, 8, 10, 12, 14, 16]
    assert shard.bucket_cuts(4, 8) == [0, 0, 1, 1, 2, 2, 3, 3, 4]  # more ranks than buckets: every other rank has no bucket
    # three senders; only the buckets 3, 4 and 15 hold anything, so the ranks 0, 3, 4, 5 and 6 receive nothing
    rng = np.random.default_rng(1)
    counts = np.zeros((3, buckets), np.int64)
    counts[0, 3], counts[0, 15] = 5, 1
    counts[1, 4] = 7            # (sender 2 has nothing at all: every slice of it is empty)
    starts = np.concatenate([np.zeros((3, 1), np.int64), np.cumsum(counts, axis=1)], axis=1)
    records = [torch.from_numpy(rng.integers(-2**62, 2**62, int(starts[j, -1]))) for j in range(3)]
    seen = []
    for r in range(world):
        lo, hi = cuts[r], cuts[r + 1]
        slices = [records[j][int(starts[j, lo]): int(starts[j, hi])] for j in range(3)]
        rel = [starts[j, lo: hi + 1] - starts[j, lo] for j in range(3)]
        merged, mstart = shard.merge_bucket_slices(slices, rel, lo, hi)
        assert mstart.tolist() == [0] + np.cumsum(counts[:, lo:hi].sum(0)).tolist()
        full = shard.full_bucket_start(mstart, lo, hi, buckets)
        assert full.dtype == torch.int32 and full.numel() == buckets + 3
        if r in (0, 3, 4, 5, 6):
            assert merged.numel() == 0 and full.tolist() == [0] * (buckets + 3)
            continue
        m = merged.numel()
        assert full[:lo + 1].tolist() == [0] * (lo + 1) and full[hi: buckets + 2].tolist() == [m] * (buckets + 2 - hi) and int(full[buckets + 2]) == 0
        for b in range(lo, hi):  # a bucket's runs lie next to each other, sender by sender, each in its own order
            want = torch.cat([records[j][int(starts[j, b]): int(starts[j, b + 1])] for j in range(3)])
            assert torch.equal(merged[int(full[b]): int(full[b + 1])], want)
        seen.append(merged)
    assert sorted(torch.cat(seen).tolist()) == sorted(torch.cat(records).tolist())
