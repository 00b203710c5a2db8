"""A host model of the seed order's 8-byte records (awfm_ordered_kernel.h: bucketFormat / bucketFits; include/awfm_gpu.h: the
seed-bucket sharding calls), in plain numpy and written from the words of those headers, not from the kernels:

  a record is {rest of the 2K-bit code string : 64 - indexBits, number in the whole batch : indexBits};
  bucketBits = min(11, 2 * depth), depth = the characters the table lookup consumes (the deeper table's when the k-mer has
  that many, the index's seed table's otherwise); indexBits = bits(totalQueries - 1), between 1 and 32;
  a record fits iff K >= depth and 2K - bucketBits + indexBits <= 64; totalQueries is 1 .. 2^32 - 2.

The bucket of a k-mer is the leading bucketBits bits of its table index.  The backward search starts at the END of a k-mer, so
the table index is the 2-bit code string of its LAST `depth` letters (the first of them most significant), which are the first
letters the search consumes.  What a record's bits look like is not modelled: records are opaque between the calls, and inside a
bucket any order is allowed -- the model says which NUMBERS a bucket holds, as a set."""
import numpy as np

BUCKET_BITS_MAX = 11
MAX_TOTAL = (1 << 32) - 2  # a batch has 1 .. 2^32 - 2 k-mers (include/awfm_gpu.h)

# a, c, g, t/u = 0..3 in either case; everything else: -1 (the k-mer is the general kernel's)
CODE = np.full(256, -1, np.int64)
for _letters, _code in (("aA", 0), ("cC", 1), ("gG", 2), ("tTuU", 3)):
    for _ch in _letters:
        CODE[ord(_ch)] = _code


def index_bits(total_queries):
    """bits of a query number: bits(totalQueries - 1), between 1 and 32"""
    return min(32, max(1, int(total_queries - 1).bit_length()))


def bucket_bits(depth):
    return min(BUCKET_BITS_MAX, 2 * depth)


def table_depth(K, seed_k, deep_k):
    """characters the table lookup of a K-mer consumes on an image with these two tables (deep_k 0: no deeper table)"""
    return deep_k if deep_k and K >= deep_k else seed_k


def fits(K, depth, total_queries):
    """does the record of a K-mer of a batch of total_queries fit 8 bytes?"""
    if not (1 <= K <= 32 and 1 <= total_queries <= MAX_TOTAL):
        return False
    return K >= depth and 2 * K - bucket_bits(depth) + index_bits(total_queries) <= 64


def buckets(K, depth, total_queries):
    """what awfmGpuOrderBuckets answers: 2^bucketBits when the record fits, 0 otherwise"""
    return 1 << bucket_bits(depth) if fits(K, depth, total_queries) else 0


def largest_total(K, depth):
    """the largest totalQueries whose records fit (the one that makes indexBits exactly 64 - 2K + bucketBits, capped at
    2^32 - 2); 0: no batch of K-mers fits at this depth"""
    if K < depth:
        return 0
    room = 64 - 2 * K + bucket_bits(depth)
    if room < 1:
        return 0
    return min(1 << min(room, 32), MAX_TOTAL)


def kmer_codes(kmers):
    """int64[n, K] codes of uint8[n, K] ASCII k-mers (-1: not a, c, g, t, u)"""
    return CODE[np.asarray(kmers, np.uint8)]


def clean(kmers):
    """bool[n]: the k-mer has only a, c, g, t, u (either case) -- the others go to the general tail"""
    return (kmer_codes(kmers) >= 0).all(axis=1)


def packed_words(kmers):
    """uint64[n]: the 2K-bit code string of clean k-mers, first character most significant, last in bits 1..0 (python
    integers: a 32-mer fills the word)"""
    codes = kmer_codes(kmers)
    out = np.zeros(len(codes), np.uint64)
    for i, row in enumerate(codes):
        word = 0
        for c in row:
            assert c >= 0, "packed_words: a clean k-mer"
            word = (word << 2) | int(c)
        out[i] = word
    return out


def bucket_of(kmers, depth):
    """int64[n]: the bucket of every k-mer (the leading min(11, 2 * depth) bits of the code string of its last `depth`
    letters); -1 for a k-mer with a character outside acgtu"""
    codes = kmer_codes(kmers)
    n, K = codes.shape
    assert K >= depth
    index = np.zeros(n, np.int64)
    for j in range(K - depth, K):
        index = index * 4 + np.maximum(codes[:, j], 0)
    out = index >> (2 * depth - bucket_bits(depth))
    out[~(codes >= 0).all(axis=1)] = -1
    return out


def expected_bucket_start(kmers, depth):
    """the buckets + 3 words awfmGpuOrderKmers leaves for a shard: [b] = clean k-mers in the buckets before b, [buckets] =
    clean k-mers, [buckets + 1] = numQueries, [buckets + 2] = k-mers with a character outside acgtu"""
    b = bucket_of(kmers, depth)
    nb = 1 << bucket_bits(depth)
    counts = np.bincount(b[b >= 0], minlength=nb)
    out = np.zeros(nb + 3, np.int64)
    out[1:nb + 1] = np.cumsum(counts)
    out[nb + 1] = len(b)
    out[nb + 2] = int((b < 0).sum())
    return out


def expected_numbers(kmers, depth, first_number):
    """({bucket: set of numbers in the whole batch}, set of the numbers in the general tail) of a shard whose first k-mer
    has the number first_number; empty buckets are left out"""
    b = bucket_of(kmers, depth)
    per = {}
    tail = set()
    for i, bucket in enumerate(b.tolist()):
        if bucket < 0:
            tail.add(first_number + i)
        else:
            per.setdefault(bucket, set()).add(first_number + i)
    return per, tail


def _check_hits_contract(ranges, counts, sp, ep, cnt):
    """awfmGpuSearchHits: exact range and count for queries with hits, count 0 and an empty range otherwise"""
    hit = cnt > 0
    assert np.array_equal(counts, cnt), "counts differ"
    assert np.array_equal(ranges[hit, 0], sp[hit]) and np.array_equal(ranges[hit, 1], ep[hit]), "ranges of hits differ"
    assert np.all(ranges[~hit, 0] > ranges[~hit, 1]), "a query without hits must have an empty range"
