"""The seed order's 8-byte records at the limits of their format (awfm_ordered_kernel.h: bucketFormat / bucketFits): the
seed-bucket sharding calls (awfmGpuOrderBuckets / OrderKmers / MergeBucketRuns / SearchOrderedRecords[Counts] /
SearchGeneralRecords) and the unsharded awfmGpuSearchHits* calls with the seed order forced, on images with 4, 1024 and 2048
buckets, with and without a deeper table.

Bucket starts and the numbers a bucket holds come from the host model (tests/bucket_records_common.py, pinned by hand in
tests/test_bucket_records.py), ranges and positions from the oracle; everything is compared exactly, and every output lies
between guard words.  Which case holds which limit of the format:

  bit 63 / bit 62 of a 32-mer's code word   test_largest_batch_of_every_length[K = 32] and test_unsharded_32mers: k-mers that
                                            begin with g, t, u (bit 63) and c + 31 x a (bit 62 alone), planted in the text
  indexBits = 32, numbers >= 2^31           test_small_shards_of_a_huge_batch (totalQueries 2^32 - 2, shards at 2^31 - 3, 2^31
                                            and at the top; the general tail reads characters through such numbers)
  a full 64-bit record                      test_largest_batch_of_every_length: every case (the largest totalQueries that fits
                                            fills the word; K = 21 at depth 5 with 2^32 - 2 k-mers: 32 + 32 bits)
  empty rest (K = depth)                    test_largest_batch_of_every_length[K = seed / deeper depth], test_unsharded_lengths
  fewer than 2048 buckets                   the geometries (5, none) and (1, none): 1024 and 4 buckets, lowBits = 0
  first refusal                             test_largest_batch_of_every_length: totalQueries + 1 (2^32 - 1 where 32 bits fit)
  empty rank                                test_worlds[40] and the one-k-mer shards of test_small_shards_of_a_huge_batch
  empty / all-ambiguous shard               test_shard_shapes
  just past the limit (16-byte records)     test_unsharded_32mers[2049], test_unsharded_32mers_on_other_geometries and
                                            test_clean_batches_below_2048_kmers (8 to 31 workgroups of the search kernel)
"""
import os
import sys
import types

import numpy as np
import pytest

from avxwindowfmindex_amd import dist as shard
from avxwindowfmindex_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bucket_records_common as br  # noqa: E402
from bucket_records_common import _check_hits_contract  # noqa: E402

pytestmark = pytest.mark.gpu

TEXT_LENGTH = 200_000
GEOMETRIES = {"8-10": (8, 10), "5": (5, 0), "6-9": (6, 9), "1": (1, 0), "12-16": (12, 16)}
SPECIAL = [b"c" + b"a" * 31, b"a" * 32, b"t" * 32, b"a" * 11 + b"tttttgacgt"]  # planted at 1000, 2000, ...: they have hits
GUARD = 64            # words before and behind every output
PATTERN = 0x5A


def _text():
    txt = synth.text(4711, TEXT_LENGTH).copy()
    txt[5000:5012] = ord("n")
    for i, word in enumerate(SPECIAL):
        txt[1000 * (i + 1): 1000 * (i + 1) + len(word)] = np.frombuffer(word, np.uint8)
    return txt


class _Host:
    """what the widths of a geometry share: the index, the oracle's twin and the oracle's answers"""

    def __init__(self, awfm, oracle, name):
        self.seed_k, self.deep_k = GEOMETRIES[name]
        self.txt = _text()
        self.ix = awfm.create_index(self.txt, awfm.AwFmAlphabetDna, 8, self.seed_k)
        self.oi = oracle.Index.wrap(oracle.DNA, 8, self.seed_k, self.ix.bwt_length, self.ix.blocks(), self.ix.prefix_sums(),
                                    self.ix.seed_table(), self.ix.packed_sa())
        self.refs = {}

    def reference(self, q, locate=True):
        """(sp, ep, counts, hit offsets, positions) of the k-mers uint8[n, K], computed once per batch (locate=False: no
        positions -- a batch of very short k-mers has too many)"""
        key = (q.shape, q.tobytes(), locate)
        if key not in self.refs:
            chars, offsets = synth.fixed_csr(q)
            sp, ep, cnt, _ = self.oi.batch_search(chars, offsets, threads=4)
            hit_off, pos = (None, None)
            if locate:
                hit_off, pos, _ = self.oi.batch_locate(sp, ep, threads=4)
            self.refs[key] = (sp, ep, cnt, hit_off, pos)
        return self.refs[key]


@pytest.fixture(scope="module")
def images(awfm):
    """one index per geometry and one device image per geometry and width, for the whole module"""
    store = types.SimpleNamespace(hosts={}, gpus={})
    yield store
    for g in store.gpus.values():
        g.destroy()
    for host in store.hosts.values():
        host.ix.dealloc()


def _env(images, awfm, oracle, request, name):
    import torch
    width = request.node.callspec.params["wide"]
    if name not in images.hosts:
        images.hosts[name] = _Host(awfm, oracle, name)
    host = images.hosts[name]
    if (name, width) not in images.gpus:  # ($AWFM_GPU_FORCE_WIDE and the diag hooks are read when the image is created)
        g = awfm.GpuIndex(host.ix)
        g.set_ordered(1)
        if host.deep_k:
            g.set_deep_seed(host.deep_k)
        images.gpus[(name, width)] = g
    return types.SimpleNamespace(g=images.gpus[(name, width)], host=host, awfm=awfm, txt=host.txt, seed_k=host.seed_k, deep_k=host.deep_k,
                                 dev=torch.device("cuda"), reference=host.reference)


class Guarded:
    """n words of `dtype` filled with `fill`, between GUARD words of a pattern on either side"""

    def __init__(self, n, dtype, fill, dev):
        import torch
        self.n, self.fill = n, fill
        self.whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.whole[:GUARD] = PATTERN
        self.whole[GUARD + n:] = PATTERN
        self.view = self.whole[GUARD: GUARD + n]
        self.ptr = self.whole.data_ptr() + GUARD * self.whole.element_size()

    def check(self):
        assert bool((self.whole[:GUARD] == PATTERN).all()) and bool((self.whole[GUARD + self.n:] == PATTERN).all()), "a guard word was overwritten"

    def untouched(self):
        self.check()
        return bool((self.view == self.fill).all())

    def host(self):
        return self.view.cpu().numpy()


def _upload(q, dev, skew=0):
    """the characters of uint8[n, K] on the device, `skew` bytes past a 256-byte boundary, with room on either side (the general
    kernel reads the aligned words that hold a k-mer)"""
    import torch
    flat = np.ascontiguousarray(q).reshape(-1)
    buf = torch.zeros(flat.size + 512, dtype=torch.uint8, device=dev)
    buf[256 + skew: 256 + skew + flat.size] = torch.from_numpy(flat).to(dev)
    return buf, buf.data_ptr() + 256 + skew


def _batch_size(K, want=3000):
    """k-mers of a batch whose positions are all compared: short k-mers occur a great many times"""
    each = max(1, TEXT_LENGTH // 4 ** min(K, 12))
    return int(min(want, max(16, 1_500_000 // each)))


def _kmers(txt, K, n, seed, ambiguous=True):
    """n K-mers: most from the text, a fifth random, a third of the letters in upper case, some t as u, and (ambiguous) an x as
    the first, a middle or the last character of a few"""
    q = synth.planted_queries(seed, n, K, txt).copy()
    q[::5] = synth.random_queries(seed + 1, len(q[::5]), K)
    rng = np.random.default_rng(seed)
    flat = q.reshape(-1)
    t = (flat == ord("t")) & (rng.random(flat.size) < 0.1)
    flat[t] = ord("u")
    up = rng.random(flat.size) < 0.3
    flat[up] = flat[up] & 0xDF
    if ambiguous:
        q[3::41, 0] = ord("x")
        q[7::43, K // 2] = ord("x")
        q[11::47, K - 1] = ord("x")
    else:
        q[(br.kmer_codes(q) < 0)] = ord("a")  # (the text's run of n)
    return q


def _first_letters_32(txt, n):
    """the batch of 32-mers in which every first letter a, c, g, t, u and their upper case occurs, with the 32-mers whose code
    words are the marks the ordering once kept inside them (c + 31 x a: bit 62 alone; g, t, u in front: bit 63), repeated to n"""
    rows = [np.frombuffer(w, np.uint8) for w in SPECIAL[:3]]
    planted = synth.planted_queries(99, 400, 32, txt)
    for letter in b"acgt":
        rows += list(planted[planted[:, 0] == letter][:6])
    rows += list(synth.random_queries(98, 8, 32))
    q = np.array(rows).copy()
    upper = q[3:27].copy()
    upper[:, 0] &= 0xDF
    as_u = q[(q[:, 0] == ord("t"))][:4].copy()
    as_u[:, 0] = ord("u")
    as_u[2:, 0] = ord("U")
    bad = q[3:6].copy()
    bad[0, 0], bad[1, 16], bad[2, 31] = ord("x"), ord("x"), ord("x")
    q = np.concatenate([q, upper, as_u, bad])
    first = set(q[:, 0].tolist())
    assert set(b"acgtuACGTU") <= first
    return np.ascontiguousarray(q[np.arange(n) % len(q)])


def _refused(env, K, total, q):
    """a batch whose records do not fit: 0 buckets, AwFmIllegalPositionError from the three calls, nothing written"""
    g, dev = env.g, env.dev
    import torch
    assert br.buckets(K, br.table_depth(K, env.seed_k, env.deep_k), total) == 0
    assert g.order_buckets(K, total) == 0
    q = q[:min(len(q), total)]  # (a shard that lies inside the batch: the format alone is what is refused)
    n = len(q)
    _buf, chars = _upload(q, dev)
    rec, bs = Guarded(n, torch.int64, 7, dev), Guarded(2048 + 3, torch.int32, 7, dev)
    kmers, ranges, counts = Guarded(n, torch.int32, 7, dev), Guarded(2 * n, torch.int64, 7, dev), Guarded(n, torch.int32, 7, dev)
    first = min(total, br.MAX_TOTAL) - n
    calls = (lambda: g.order_kmers(chars, K, n, first, total, rec.ptr, bs.ptr),
             lambda: g.search_ordered_records(rec.ptr, bs.ptr, 0, 1, K, total, kmers.ptr, ranges.ptr, d_order_counts=counts.ptr),
             lambda: g.search_general_records(chars, K, n, first, total, rec.ptr, bs.ptr, kmers.ptr, ranges.ptr))
    for call in calls:
        with pytest.raises(env.awfm.AwFmError) as err:
            call()
        assert err.value.rc == env.awfm.AwFmIllegalPositionError
    torch.cuda.synchronize()
    for out in (rec, bs, kmers, ranges, counts):
        assert out.untouched()


def _positions(env, ranges_ptr, m):
    """hit offsets and positions of the m ranges at ranges_ptr (device): the list of positions of every entry"""
    import torch
    g, dev = env.g, env.dev
    d_off = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    d_scratch = torch.zeros(env.awfm.GpuIndex.scan_scratch_bytes(m), dtype=torch.uint8, device=dev)
    hits = g.hit_offsets(ranges_ptr, m, d_off.data_ptr(), d_scratch.data_ptr())
    d_pos = Guarded(max(hits, 1), torch.int64, -1, dev)
    g.locate(ranges_ptr, d_off.data_ptr(), m, hits, d_pos.ptr)
    torch.cuda.synchronize()
    d_pos.check()
    off = d_off.cpu().numpy()
    p = d_pos.host().view(np.uint64)
    assert int(off[m]) == hits
    return [p[off[i]: off[i + 1]] for i in range(m)]


def _sharded(env, K, total, shards, ranges):
    """The sharding calls over `shards` = [(first number, uint8[n, K])], one emulated rank after the other: every shard is
    ordered and its general tail searched where it is; then for every bucket range [lo, hi) of `ranges` the slices of all
    shards are merged (torch's index arithmetic and the one-launch merge) and searched, with hit offsets and positions on top."""
    import torch
    g, dev = env.g, env.dev
    depth = br.table_depth(K, env.seed_k, env.deep_k)
    nb = g.order_buckets(K, total)
    assert nb == br.buckets(K, depth, total) and nb == 1 << min(11, 2 * depth)
    everything = np.concatenate([q for _, q in shards])
    numbers = np.concatenate([first + np.arange(len(q), dtype=np.int64) for first, q in shards])
    assert len(set(numbers.tolist())) == len(numbers) and numbers.min() >= 0 and numbers.max() < total
    sp, ep, cnt, hit_off, pos = env.reference(everything)
    got_numbers, got_ranges, got_positions = [], [], []
    expect_numbers = []           # with the multiplicity the bucket ranges give a number
    recs, starts, models = [], [], []
    for first, q in shards:
        n = len(q)
        _buf, chars = _upload(q, dev)
        rec, bs = Guarded(n, torch.int64, -1, dev), Guarded(nb + 3, torch.int32, -1, dev)
        g.order_kmers(chars, K, n, first, total, rec.ptr, bs.ptr)
        torch.cuda.synchronize()
        rec.check()
        bs.check()
        start = bs.host().view(np.uint32).astype(np.int64)
        assert np.array_equal(start, br.expected_bucket_start(q, depth)), "bucket starts differ from the model's"
        per, tail = br.expected_numbers(q, depth, first)
        # the general tail: searched where its characters are
        kmers, rr = Guarded(n, torch.int32, -1, dev), Guarded(2 * n, torch.int64, 7, dev)
        g.search_general_records(chars, K, n, first, total, rec.ptr, bs.ptr, kmers.ptr, rr.ptr)
        torch.cuda.synchronize()
        left = int(start[nb])
        assert left == n - len(tail) and int(start[nb + 2]) == len(tail)
        k = kmers.host().view(np.uint32).astype(np.int64)
        r = rr.host().view(np.uint64).reshape(n, 2)
        kmers.check()
        rr.check()
        assert np.all(k[:left] == 0xFFFFFFFF) and np.all(r[:left] == 7), "the general kernel wrote an entry of the ordered k-mers"
        assert sorted(k[left:].tolist()) == sorted(tail), "the numbers in the general tail differ from the model's"
        got_numbers.append(k[left:])
        got_ranges.append(r[left:])
        if n > left:  # (a k-mer with the text's n in it occurs where the text has it: the tail has hits as well)
            got_positions += _positions(env, rr.ptr + 16 * left, n - left)
        expect_numbers += sorted(tail)
        recs.append(rec)
        starts.append(start)
        models.append(per)
    for lo, hi in ranges:  # the exchange, by indexing: this rank gets the buckets [lo, hi) of everybody
        slices = [recs[j].view[int(starts[j][lo]): int(starts[j][hi])] for j in range(len(shards))]
        rel = [torch.from_numpy(starts[j][lo: hi + 1] - starts[j][lo]) for j in range(len(shards))]
        merged, mstart = shard.merge_bucket_slices(slices, rel, lo, hi)
        m = merged.numel()
        full = shard.full_bucket_start(mstart, lo, hi, nb)
        # the same in one launch, as dist.bucket_exchange_on_device calls it (a rank that received nothing included: it passes
        # its own output array for the slices nobody reads)
        received = torch.cat(slices)
        sizes = [int(sl.numel()) for sl in slices]
        d_slice_at = torch.tensor([sum(sizes[:j]) for j in range(len(slices))], dtype=torch.int64).to(dev)
        d_starts = torch.stack([t.to(torch.int32) for t in rel]).to(dev)
        out, bs2 = Guarded(max(m, 1), torch.int64, -1, dev), Guarded(nb + 3, torch.int32, -1, dev)
        g.merge_bucket_runs(received.data_ptr() or out.ptr, d_slice_at.data_ptr(), d_starts.data_ptr(), len(slices), lo, hi, nb, out.ptr, bs2.ptr)
        torch.cuda.synchronize()
        out.check()
        bs2.check()
        assert torch.equal(out.view[:m], merged.to(dev)) and torch.equal(bs2.view.cpu(), full), "the merge kernel and torch's index arithmetic disagree"
        want = sorted((b, number) for per in models for b, held in per.items() if lo <= b < hi for number in held)
        assert m == len(want)
        size = max(m, 1)
        kmers, rr, cc = Guarded(size, torch.int32, -1, dev), Guarded(2 * size, torch.int64, 7, dev), Guarded(size, torch.int32, 7, dev)
        g.search_ordered_records(out.ptr, bs2.ptr, lo, hi, K, total, kmers.ptr, rr.ptr, d_order_counts=cc.ptr)
        torch.cuda.synchronize()
        if m == 0:
            # a rank that received nothing: all its bucket starts are 0, the merge stores no record, and the search of such an
            # array is a successful call that stores nothing
            assert full.tolist() == [0] * (nb + 3) and out.untouched()
            assert kmers.untouched() and rr.untouched() and cc.untouched()
            continue
        kmers.check()
        rr.check()
        cc.check()
        k = kmers.host().view(np.uint32).astype(np.int64)
        r = rr.host().view(np.uint64).reshape(m, 2)
        c = cc.host().view(np.uint32).astype(np.uint64)
        assert np.array_equal(c, np.where(r[:, 0] <= r[:, 1], r[:, 1] - r[:, 0] + np.uint64(1), np.uint64(0))), "the counts in order are not the range sizes"
        held = np.repeat(np.arange(nb), np.diff(full[:nb + 1].numpy().astype(np.int64)))
        assert sorted(zip(held.tolist(), k.tolist())) == want, "the numbers in the buckets of the searched order differ from the model's"
        got_numbers.append(k)
        got_ranges.append(r)
        got_positions += _positions(env, rr.ptr, m)
        expect_numbers += [number for _, number in want]
    got_numbers = np.concatenate(got_numbers)
    got_ranges = np.concatenate(got_ranges)
    order = np.argsort(got_numbers, kind="stable")
    assert np.array_equal(got_numbers[order], np.sort(np.array(expect_numbers, np.int64))), "a k-mer was answered by no rank, or by two"
    by_number = np.argsort(numbers)
    at = by_number[np.searchsorted(numbers[by_number], got_numbers)]  # entry -> its k-mer in the reference's arrays
    hit = cnt[at] > 0
    assert np.array_equal(got_ranges[hit, 0], sp[at][hit]) and np.array_equal(got_ranges[hit, 1], ep[at][hit]), "ranges of k-mers with hits differ from the oracle's"
    assert np.all(got_ranges[~hit, 0] > got_ranges[~hit, 1]), "a k-mer without hits got a range"
    for e in np.flatnonzero(hit):
        assert np.array_equal(got_positions[e], pos[hit_off[at[e]]: hit_off[at[e] + 1]]), f"positions of k-mer {got_numbers[e]}"
    return int(hit.sum())


def _cuts(nb, world):
    cuts = shard.bucket_cuts(nb, world)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def _lengths(name):
    seed_k, deep_k = GEOMETRIES[name]
    return sorted({seed_k, seed_k + 1, 21, 29, 31, 32} | ({deep_k, deep_k + 1} if deep_k else set()))


def _largest_batch(env, K):
    depth = br.table_depth(K, env.seed_k, env.deep_k)
    total = br.largest_total(K, depth)
    assert total > 0
    if total < br.MAX_TOTAL:
        assert 2 * K - br.bucket_bits(depth) + br.index_bits(total) == 64, "the largest batch fills the record"
    else:
        assert br.index_bits(total) == 32 and 2 * K - br.bucket_bits(depth) + 32 <= 64
    nb = 1 << br.bucket_bits(depth)
    world = 3
    if total <= 8192:  # the whole batch, in contiguous shards
        q = _first_letters_32(env.txt, total) if K == 32 else _kmers(env.txt, K, total, 100 + K)
        bounds = [shard.shard_bounds(total, min(world, total), r) for r in range(min(world, total))]
        shards = [(b, q[b:e]) for b, e in bounds if e > b]
    else:  # shards at the bottom, in the middle and at the very top of the batch's numbers
        n = _batch_size(K)
        q = _kmers(env.txt, K, 3 * n, 100 + K)
        shards = [(0, q[:n]), (total // 2 - 1, q[n:2 * n]), (total - n, q[2 * n:])]
    hits = _sharded(env, K, total, shards, _cuts(nb, min(world, nb)))
    assert hits > 0
    refused = total + 1 if total < br.MAX_TOTAL else (1 << 32) - 1  # one more k-mer: one more index bit, or past the API's range
    _refused(env, K, refused, shards[-1][1][:64])


@pytest.mark.parametrize("case", [f"{name}/{K}" for name in ("8-10", "5", "6-9", "1") for K in _lengths(name)])
def test_largest_batch_of_every_length(oracle, awfm, require_gpu, wide, images, request, case):
    """every k-mer length at which the format changes, with the largest totalQueries whose records fit -- the one that fills
    the 64 bits (K = 32 on 2048 buckets: 2048; K = 21 at depth 5: 2^32 - 2, 32 + 32 bits) -- and the refusal of the next"""
    name, K = case.split("/")
    _largest_batch(_env(images, awfm, oracle, request, name), int(K))


def test_largest_batch_with_a_depth_16_table(oracle, awfm, require_gpu, wide):
    """the same on the geometry (12, 16): 21 table-index bits below the bucket's.  Its deeper table is large, so the image
    lives for this test only"""
    import torch
    host = _Host(awfm, oracle, "12-16")
    g = awfm.GpuIndex(host.ix)
    g.set_ordered(1)
    g.set_deep_seed(host.deep_k)
    env = types.SimpleNamespace(g=g, host=host, awfm=awfm, txt=host.txt, seed_k=host.seed_k, deep_k=host.deep_k, dev=torch.device("cuda"),
                                reference=host.reference)
    try:
        for K in _lengths("12-16"):
            _largest_batch(env, K)
    finally:
        g.destroy()
        host.ix.dealloc()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_small_shards_of_a_huge_batch(oracle, awfm, require_gpu, wide, images, request, n):
    """shards of n k-mers of a batch of 2^32 - 2 (indexBits = 32) whose numbers begin at 0, just below 2^31, at 2^31 and end at
    the batch's last number: the numbers come back as unsigned 32-bit, and the general tail reads its characters through them"""
    env = _env(images, awfm, oracle, request, "8-10")
    K, total = 21, br.MAX_TOTAL
    firsts = [0, (1 << 31) - 3, 1 << 31, total - n]
    # (the shards at 2^31 - 3 and at 2^31 overlap from n = 4 on: they are taken in two runs)
    q = _kmers(env.txt, K, 4 * n, 200 + n)
    if n == 1:
        q[2, 0] = ord("x")  # the one k-mer of the shard at 2^31 goes to the general tail: a shard with no ordered k-mer
    nb = 2048
    for picks in ((0, 1, 3), (2,)):
        shards = [(firsts[i], q[i * n:(i + 1) * n]) for i in picks]
        _sharded(env, K, total, shards, _cuts(nb, 4))


@pytest.mark.parametrize("shape", ["all-ambiguous", "none-ambiguous", "single-bucket", "last-bucket", "sorted"])
def test_shard_shapes(oracle, awfm, require_gpu, wide, images, request, shape):
    """a shard whose k-mers are all the general kernel's ([buckets] = 0), one with none, one in a single bucket, one in the last
    bucket only, one that arrives sorted -- each beside an ordinary shard of the same batch"""
    env = _env(images, awfm, oracle, request, "8-10")
    K, n = 21, 1500
    rng = np.random.default_rng(7)
    plain = _kmers(env.txt, K, n, 300)
    if shape == "all-ambiguous":
        q = _kmers(env.txt, K, n, 301)
        q[np.arange(n), rng.integers(0, K, n)] = ord("x")
    elif shape == "none-ambiguous":
        q = _kmers(env.txt, K, n, 302, ambiguous=False)
        assert br.clean(q).all()
    elif shape == "single-bucket":  # the last 10 letters the same: one table entry, hence one bucket
        q = _kmers(env.txt, K, n, 303, ambiguous=False)
        q[:, K - 10:] = q[0, K - 10:]
        assert len(set(br.bucket_of(q, 10).tolist())) == 1
    elif shape == "last-bucket":  # ttttt + g or t: the leading 11 bits of the table index all set
        q = _kmers(env.txt, K, n, 304, ambiguous=False)
        q[:, K - 10: K - 5] = ord("t")
        q[:, K - 5] = np.where(rng.random(n) < 0.5, ord("g"), ord("T"))
        q[::7] = np.frombuffer(SPECIAL[3], np.uint8)  # (planted in the text: the last bucket has hits)
        assert set(br.bucket_of(q, 10).tolist()) == {2047}
    else:
        q = _kmers(env.txt, K, n, 305, ambiguous=False)
        q = q[np.lexsort(br.kmer_codes(q)[:, :K - 11:-1].T)]  # by the table index: whole runs of one bucket after another
    shards = [(0, q), (n, plain)]
    total = 2 * n
    hits = _sharded(env, K, total, shards, _cuts(2048, 3))
    assert hits > 0


@pytest.mark.parametrize("world", [1, 3, 8, 40])
def test_worlds(oracle, awfm, require_gpu, wide, images, request, world):
    """world sizes; with 40 ranks the batch's k-mers lie in three buckets, so most ranks receive nothing: what such a rank does
    (include/awfm_gpu.h: awfmGpuMergeBucketRuns) is asserted in _sharded"""
    env = _env(images, awfm, oracle, request, "8-10")
    K, total = 21, 4001
    q = _kmers(env.txt, K, total, 400)
    if world == 40:
        keep = _kmers(env.txt, K, 3, 401, ambiguous=False)
        q[:, K - 10:] = keep[np.arange(total) % 3][:, K - 10:]
        q[5::50, 2] = ord("x")
    shards = [(b, q[b:e]) for b, e in (shard.shard_bounds(total, world, r) for r in range(world))]
    _sharded(env, K, total, shards, _cuts(2048, world))


@pytest.mark.parametrize("name", ["8-10", "5", "1"])
def test_bucket_ranges(oracle, awfm, require_gpu, wide, images, request, name):
    """bucket ranges of one bucket, of the last bucket, and of all"""
    env = _env(images, awfm, oracle, request, name)
    K, n = 21, 2000
    total = 3 * n
    q = _kmers(env.txt, K, 2 * n, 500)
    q[::9, K - 10:] = ord("t")  # (the last bucket is not empty)
    depth = br.table_depth(K, env.seed_k, env.deep_k)
    nb = 1 << br.bucket_bits(depth)
    one = int(br.bucket_of(q[1:2], depth)[0])
    assert one >= 0
    _sharded(env, K, total, [(0, q[:n]), (2 * n, q[n:])], [(one, one + 1), (nb - 1, nb), (0, nb)])


def _unsharded(env, K, q, skew=0):
    """the unsharded calls of a batch that takes the seed order: search_hits (ranges and counts, ranges only, counts only),
    search_hits_packed, search_hits_sparse, search_hits_compact, search_hits_in_order with counts"""
    import torch
    g, dev = env.g, env.dev
    Q = len(q)
    sp, ep, cnt, _, _ = env.reference(q, locate=False)
    _buf, chars = _upload(q, dev, skew)
    assert g.search_hits_is_ordered(False, K, Q)

    def outputs():
        return Guarded(2 * Q, torch.int64, 7, dev), Guarded(Q, torch.int32, 7, dev)

    def view(rr, cc):
        rr.check()
        cc.check()
        return rr.host().view(np.uint64).reshape(Q, 2), cc.host().view(np.uint32)

    rr, cc = outputs()
    g.search_hits(chars, 0, K, Q, rr.ptr, cc.ptr)
    torch.cuda.synchronize()
    _check_hits_contract(*view(rr, cc), sp, ep, cnt)
    rr2, cc2 = outputs()
    g.search_hits(chars, 0, K, Q, rr2.ptr, 0)
    g.search_hits(chars, 0, K, Q, 0, cc2.ptr)
    torch.cuda.synchronize()
    _check_hits_contract(*view(rr2, cc2), sp, ep, cnt)
    # packed: the k-mers that can be packed
    ok = br.clean(q)
    m = int(ok.sum())
    if m:
        packed = env.awfm.pack_kmers(np.ascontiguousarray(q[ok]))
        assert np.array_equal(packed, br.packed_words(q[ok]))
        d_packed = torch.from_numpy(packed.view(np.int64)).to(dev)
        d_scratch = torch.zeros(m * K + 64, dtype=torch.uint8, device=dev)
        pr, pc = Guarded(2 * m, torch.int64, 7, dev), Guarded(m, torch.int32, 7, dev)
        g.search_hits_packed(d_packed.data_ptr(), K, m, pr.ptr, pc.ptr, d_scratch.data_ptr())
        torch.cuda.synchronize()
        pr.check()
        pc.check()
        _check_hits_contract(pr.host().view(np.uint64).reshape(m, 2), pc.host().view(np.uint32), sp[ok], ep[ok], cnt[ok])
    # sparse: counts for all, ranges of the k-mers with hits
    rr, cc = outputs()
    g.search_hits_sparse(chars, 0, K, Q, rr.ptr, cc.ptr)
    torch.cuda.synchronize()
    r, c = view(rr, cc)
    hit = cnt > 0
    assert np.array_equal(c, cnt) and np.array_equal(r[hit, 0], sp[hit]) and np.array_equal(r[hit, 1], ep[hit])
    # the list of hits
    lk, lr, num = Guarded(Q, torch.int32, 7, dev), Guarded(2 * Q, torch.int64, 7, dev), Guarded(1, torch.int32, 7, dev)
    g.search_hits_compact(chars, 0, K, Q, lk.ptr, lr.ptr, Q, num.ptr)
    torch.cuda.synchronize()
    for out in (lk, lr, num):
        out.check()
    listed = int(num.host()[0])
    assert listed == int(hit.sum())
    ids = lk.host().view(np.uint32).astype(np.int64)
    lr_ = lr.host().view(np.uint64).reshape(Q, 2)
    by = np.argsort(ids[:listed], kind="stable")
    assert np.array_equal(ids[:listed][by], np.flatnonzero(hit)), "the list does not hold every k-mer with hits once"
    assert np.array_equal(lr_[:listed][by, 0], sp[hit]) and np.array_equal(lr_[:listed][by, 1], ep[hit])
    assert np.all(ids[listed:] == 0xFFFFFFFF) and np.all(lr_[listed:, 0] > lr_[listed:, 1])
    # results in search order, with counts
    ok_, orr, occ = Guarded(Q, torch.int32, -1, dev), Guarded(2 * Q, torch.int64, 7, dev), Guarded(Q, torch.int32, 7, dev)
    g.search_hits_in_order(chars, 0, K, Q, ok_.ptr, orr.ptr, d_order_counts=occ.ptr)
    torch.cuda.synchronize()
    for out in (ok_, orr, occ):
        out.check()
    k = ok_.host().view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(k), np.arange(Q)), "search order is not a permutation of the batch"
    r, c = orr.host().view(np.uint64).reshape(Q, 2), occ.host().view(np.uint32)
    home_r, home_c = np.zeros_like(r), np.zeros_like(c)
    home_r[k], home_c[k] = r, c
    _check_hits_contract(home_r, home_c, sp, ep, cnt)


@pytest.mark.parametrize("lookup_first", [None, "0", "1"])
@pytest.mark.parametrize("Q", [1, 2, 1024, 1025, 2048, 2049])
def test_unsharded_32mers(oracle, awfm, require_gpu, wide, images, request, monkeypatch, Q, lookup_first):
    """32-mers around the batch sizes at which their record stops fitting (2048 on 2048 buckets; 2049 takes the 16-byte
    records), with the ordering passes alone, behind the lookup kernel and as the library chooses: c + 31 x a, whose code word is
    the lookup kernel's mark of an unused slot, is in the text and must be found"""
    if lookup_first is None:
        monkeypatch.delenv("AWFM_GPU_LOOKUP_FIRST", raising=False)
    else:
        monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", lookup_first)
    env = _env(images, awfm, oracle, request, "8-10")
    q = _first_letters_32(env.txt, Q)
    cnt = env.reference(q[:1], locate=False)[2]
    assert bytes(q[0]) == SPECIAL[0] and cnt[0] >= 1
    _unsharded(env, 32, q, skew=Q % 4)


@pytest.mark.parametrize("name", ["5", "6-9", "1"])
@pytest.mark.parametrize("Q", [2, 1024, 1025, 2049])
def test_unsharded_32mers_on_other_geometries(oracle, awfm, require_gpu, wide, images, request, name, Q):
    """the same where a 32-mer's record fits up to 1024 k-mers (1024 buckets) or 4 (4 buckets)"""
    env = _env(images, awfm, oracle, request, name)
    _unsharded(env, 32, _first_letters_32(env.txt, Q), skew=(Q + 1) % 4)


@pytest.mark.parametrize("skew", [0, 1, 2, 3])
@pytest.mark.parametrize("case", [f"{name}/{K}" for name in ("8-10", "5", "6-9", "1") for K in sorted({GEOMETRIES[name][0], GEOMETRIES[name][1] or 31, 31})])
def test_unsharded_lengths(oracle, awfm, require_gpu, wide, images, request, case, skew):
    """K = depth (an empty rest) and K = 31 at 4099 k-mers, the query buffer at each of the four byte alignments"""
    name, K = case.split("/")
    env = _env(images, awfm, oracle, request, name)
    K = int(K)
    _unsharded(env, K, _kmers(env.txt, K, 4099, 600 + K), skew=skew)


@pytest.mark.parametrize("name", ["5", "1"])
@pytest.mark.parametrize("Q", [513, 1025, 1956, 2047])
def test_clean_batches_below_2048_kmers(oracle, awfm, require_gpu, wide, images, request, name, Q):
    """32-mers without a single ambiguity character, 513 to 2047 of them, where their records are the 16-byte ones: the search
    kernel then runs 8 to 31 workgroups, fewer per XCD than it has groups of ticket counters, and every chunk of the order must
    still be some wave's (with ambiguous k-mers in the batch the order is shorter and hides a chunk that nobody takes)"""
    env = _env(images, awfm, oracle, request, name)
    q = _kmers(env.txt, 32, Q, 700 + Q, ambiguous=False)
    assert br.clean(q).all()
    _unsharded(env, 32, q, skew=Q % 4)
