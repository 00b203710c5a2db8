"""Every byte value through every kernel that reads letters (tests/byte_values_common.py states which letter a byte is).

The search family -- searchKernel in its four variants with and without a deeper table, orderedSearchKernel behind
encodeCodes4Kernel, lookupSearchKernel<K>, the exact lookup kernel, the mixed-length lookup kernel, aminoLookupSearchKernel<K>,
the longest suffix match, the one-substitution search, pack / unpack and the packed search -- on byte-rich batches: every byte
value but the sentinel class at every position mod 4 of a query, in each of the four k-mers that are decoded together, with the
query buffer 0 to 3 bytes into its allocation; against the oracle, for the k-mers whose reference table index leaves the table
against the letter-by-letter search built from the oracle's single step, and against the alias property.  The library's own
reports say which kernel ran.

The read path -- verification, alignment, affine alignment, slot scores, window scores -- against the host twins, which
tests/test_byte_values.py pins to the plain-Python restatements: reads and texts with a third of their bytes replaced (the
sentinel class among them), bands of 16, 32 and 64 lanes, the read buffer at skews 0 to 3, both alphabets, guarded outputs; the
image's index is built from a well-formed text of the same length (these calls take the image for its text, record table and
alphabet), nothing here walks an index over non-letters.  The reverse complement over all 256 values at every alignment; the
GPU builder on nucleotide texts that hold every byte value but the sentinel class."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import byte_values_common as bv  # noqa: E402
import gap_runs_common as gr  # noqa: E402
import pair_mates_common as pm  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import window_scores_common as ws  # noqa: E402
import test_gpu_align_affine as gaa  # noqa: E402
import test_gpu_align_chains as gac  # noqa: E402
import test_gpu_longest_match as glm  # noqa: E402
import test_gpu_one_substitution as gos  # noqa: E402
import test_gpu_score_chains as gsc  # noqa: E402
import test_gpu_verify_chains as gvc  # noqa: E402
import test_gpu_window_scores as gws  # noqa: E402
from test_gpu_build import _host_build, _same_arrays  # noqa: E402
from test_gpu_parity import _check_hits_contract  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, _upload  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABETS = pytest.mark.parametrize("alphabet", [bv.DNA, bv.AMINO], ids=["dna", "amino"])
SEED_K, DEEP_K = {bv.DNA: 6, bv.AMINO: 2}, {bv.DNA: 9, bv.AMINO: 4}
TEXT_LENGTH, FILL, RATIO = 100_000, 6000, 8
EDGE = 8  # guard words around the outputs of the search calls
_BATCHES, _TEXTS = {}, {}


class Batch:
    """a byte-rich batch on an index of a well-formed text, with what every query must get: computed once, shared by the tests
    and their parameters, never changed"""

    def __init__(self, awfm, oracle, alphabet, lengths):
        self.alphabet, self.lengths, self.fixed = alphabet, lengths, lengths if isinstance(lengths, int) else 0
        self.seed_k, self.deep_k = SEED_K[alphabet], DEEP_K[alphabet]
        if alphabet not in _TEXTS:
            text = bv.well_formed_text(50 + alphabet, TEXT_LENGTH, alphabet, ambiguity_runs=60)
            ix = awfm.create_index(text, alphabet, RATIO, self.seed_k)
            oi = oracle.Index.wrap(alphabet, RATIO, self.seed_k, ix.bwt_length, ix.blocks(), ix.prefix_sums(), ix.seed_table(), ix.packed_sa())
            _TEXTS[alphabet] = (text, ix, oi)
        self.text, self.ix, self.oi = _TEXTS[alphabet]
        self.strings, self.base, self.variants, self.aliases, self.first_variant, self.first_alias = bv.search_batch(
            90 + alphabet, self.text, alphabet, lengths, keep_clear=self.deep_k, fill=FILL)
        self.chars, self.offsets = bv.csr(self.strings)
        self.Q = len(self.strings)
        self.sp, self.ep, self.counts, self.over = bv.expected_search(self.oi, alphabet, self.seed_k, self.strings)
        self.check_coverage()

    def check_coverage(self):
        """what every test of this batch relies on: each byte value at every position mod 4 in each of the four k-mers decoded
        together; the bytes that are no proper letters inside seed_k, inside deep_k only and ahead of both; every class in a query
        that has hits; the k-mers whose table index leaves the table are there (amino) and only there"""
        a, values = self.alphabet, bv.query_bytes(self.alphabet)
        assert 10_000 <= self.Q <= 100_000
        bv.check_coverage(self.variants, values, fixed_length=self.fixed, first=self.first_variant)
        assert {v.value for v in self.aliases} == set(values)
        assert not any(bv.INDEX[a][c] == bv.SENTINEL_INDEX[a] for s in self.strings for c in s)
        have = bv.zones(self.variants, a, self.seed_k, self.deep_k)
        longest = self.fixed or self.lengths[1]
        for key in bv.all_query_classes(a):
            if key[0] >= bv.CARDINALITY[a]:
                assert {(key, z) for z in range(3) if z < 2 or longest > self.deep_k} <= have, key
        assert bv.classes_with_hits(a, self.strings, self.counts) == bv.all_query_classes(a)
        carried = sum(bv.carries(a, s, self.seed_k) for s in self.strings)
        assert (self.over.sum() >= 16 and carried >= 64) if a == bv.AMINO else (not self.over.any() and not carried)
        assert (self.counts > 0).sum() > self.Q // 8 and (self.counts == 0).sum() > self.Q // 8


def batch_of(awfm, oracle, alphabet, lengths):
    key = (alphabet, lengths)
    if key not in _BATCHES:
        _BATCHES[key] = Batch(awfm, oracle, alphabet, lengths)
    return _BATCHES[key]


class Device:
    """a batch on the device: the characters `skew` bytes into their allocation between guard words, and calls whose outputs lie
    between guard words too"""

    def __init__(self, torch, batch, skew):
        self.torch, self.batch, self.skew = torch, batch, skew
        chars = np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), batch.chars, np.full(GUARD, PATTERN, np.uint8)))
        self.chars = torch.from_numpy(chars).to("cuda")
        assert self.chars.data_ptr() % 4 == 0
        self.address = self.chars.data_ptr() + GUARD + skew
        self.offsets = None if batch.fixed else torch.from_numpy(batch.offsets.view(np.int64)).to("cuda")

    def call(self, method, ranges=True, counts=True):
        """g.search or g.search_hits -> (ranges uint64[Q, 2] or None, counts uint32[Q] or None)"""
        torch, Q = self.torch, self.batch.Q
        d_ranges = torch.full((2 * Q + 2 * EDGE,), 7, dtype=torch.int64, device="cuda")
        d_counts = torch.full((Q + 2 * EDGE,), 7, dtype=torch.int32, device="cuda")
        method(self.address, 0 if self.offsets is None else self.offsets.data_ptr(), self.batch.fixed, Q,
               d_ranges.data_ptr() + 8 * EDGE if ranges else 0, d_counts.data_ptr() + 4 * EDGE if counts else 0)
        torch.cuda.synchronize()
        r, c = d_ranges.cpu().numpy(), d_counts.cpu().numpy()
        assert (r[:EDGE] == 7).all() and (r[EDGE + 2 * Q:] == 7).all() and (c[:EDGE] == 7).all() and (c[EDGE + Q:] == 7).all(), "wrote outside an output"
        assert ranges or (r == 7).all()
        assert counts or (c == 7).all()
        return (r[EDGE:EDGE + 2 * Q].view(np.uint64).reshape(Q, 2) if ranges else None), (c[EDGE:EDGE + Q].view(np.uint32) if counts else None)

    def hit_list(self, g):
        """search_hits_compact + sort_hits -> (k-mer numbers, ranges) of the k-mers with hits"""
        torch, Q = self.torch, self.batch.Q
        d_kmers = torch.zeros(Q, dtype=torch.int32, device="cuda")
        d_ranges = torch.zeros(2 * Q, dtype=torch.int64, device="cuda")
        d_num = torch.zeros(1, dtype=torch.int32, device="cuda")
        g.search_hits_compact(self.address, 0 if self.offsets is None else self.offsets.data_ptr(), self.batch.fixed, Q, d_kmers.data_ptr(),
                              d_ranges.data_ptr(), Q, d_num.data_ptr())
        torch.cuda.synchronize()
        listed = int(d_num.item())
        assert listed <= Q
        g.sort_hits(d_kmers.data_ptr(), d_ranges.data_ptr(), listed)
        torch.cuda.synchronize()
        return d_kmers[:listed].cpu().numpy().view(np.uint32), d_ranges[:2 * listed].cpu().numpy().view(np.uint64).reshape(listed, 2)


def assert_exact(batch, ranges, counts, what):
    """awfmGpuSearch: every k-mer's final range, the first empty range of an absent k-mer included"""
    bad = np.flatnonzero((ranges[:, 0] != batch.sp) | (ranges[:, 1] != batch.ep))
    assert not len(bad), (what, "ranges", len(bad), [(int(j), batch.strings[j], ranges[j].tolist(), int(batch.sp[j]), int(batch.ep[j]), bool(batch.over[j])) for j in bad[:4]])
    assert np.array_equal(counts, batch.counts), (what, "counts")
    bv.assert_alias_property(batch.aliases, batch.first_alias, ranges[:, 0], ranges[:, 1], what)


def assert_hits(batch, ranges, counts, what):
    """awfmGpuSearchHits: exact range and count of a k-mer with hits, count 0 and some empty range otherwise"""
    bad = np.flatnonzero(counts != batch.counts)
    assert not len(bad), (what, "counts", len(bad), [(int(j), batch.strings[j], int(counts[j]), int(batch.counts[j]), bool(batch.over[j])) for j in bad[:4]])
    if ranges is not None:
        _check_hits_contract(ranges, counts, batch.sp, batch.ep, batch.counts)
        bv.assert_alias_property(batch.aliases, batch.first_alias, ranges[:, 0], ranges[:, 1], what)


def assert_list(batch, listed, what):
    ids, ranges = listed
    hit = batch.counts > 0
    assert np.array_equal(ids, np.flatnonzero(hit)), (what, "the k-mers of the sparse list")
    assert np.array_equal(ranges[:, 0], batch.sp[hit]) and np.array_equal(ranges[:, 1], batch.ep[hit]), (what, "the ranges of the sparse list")


def image_of(awfm, batch, wide, deep=True, ordered=None):
    g = awfm.GpuIndex(batch.ix)
    assert bool(g.is_wide) == bool(wide)  # the `wide` fixture really took effect
    if ordered is not None:
        g.set_ordered(ordered)
    if deep:
        g.set_deep_seed(batch.deep_k)
        assert g.deep_seed_k == batch.deep_k and f"deeper table depth {batch.deep_k}" in g.describe()
    else:
        assert "deeper table no" in g.describe()
    return g


# ---- the search family --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [1, 2, 3, 4])  # AWFM_GPU_KERNEL_GROUP8 / 4 / 2 / 1 lanes per query
@ALPHABETS
def test_search_kernel_in_every_variant(oracle, awfm, require_gpu, wide, monkeypatch, kernel, alphabet):
    """searchKernel: mixed lengths 1 .. 40, with a deeper table (the bytes of index 20 fall inside seed_k, inside deep_k only, ahead
    of both) and without"""
    import torch
    monkeypatch.setenv("AWFM_GPU_EXACT_LOOKUP", "0")
    batch = batch_of(awfm, oracle, alphabet, (1, 40))
    devices = [Device(torch, batch, skew) for skew in range(4)]
    for deep in (True, False):
        g = image_of(awfm, batch, wide, deep)
        g.set_kernel(kernel)
        for d in devices:
            ranges, counts = d.call(g.search)
            assert not g.last_search_was_exact_lookup()
            assert_exact(batch, ranges, counts, f"kernel {kernel} deep {deep} skew {d.skew}")
        g.destroy()


@pytest.mark.parametrize("K", [21, 13, 12, 28, 32])
def test_seed_order_kernels_of_fixed_length_nucleotide_batches(oracle, awfm, require_gpu, wide, monkeypatch, K):
    """orderedSearchKernel behind encodeCodes4Kernel ($AWFM_GPU_LOOKUP_FIRST=0) and lookupSearchKernel<K> (=1), forced as in
    test_lookup_first_keeps_hits_bit_identical: dense results, counts only, ranges only, the sparse list; then the exact lookup
    kernel under awfmGpuSearch.  Both front ends work on 8-byte records: 2 K bits of codes less the 11 of the bucket, and the
    k-mer's number.  A 32-mer's record does not fit them in a batch of more than 2^11 k-mers: it is ordered in 16-byte records
    (decodeWord), whatever $AWFM_GPU_LOOKUP_FIRST says -- 28 is the multiple of 4 that lookupSearchKernel sees"""
    import torch
    monkeypatch.setenv("AWFM_GPU_PAIR", "1")
    batch = batch_of(awfm, oracle, bv.DNA, K)
    g = image_of(awfm, batch, wide, ordered=1)
    assert "pair image yes" in g.describe() and g.search_hits_is_ordered(False, K, batch.Q)
    devices = [Device(torch, batch, skew) for skew in range(4)]
    fits = 2 * K - min(2 * batch.deep_k, 11) + (batch.Q - 1).bit_length() <= 64  # (bucketFits, csrc/awfm_ordered_kernel.h)
    assert fits == (K != 32)
    for mode in ("1", "0"):
        monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", mode)
        for d in devices:
            ranges, counts = d.call(g.search_hits)
            assert g.last_ordered_kernel_is_lookup() == (mode == "1" and fits)
            assert_hits(batch, ranges, counts, f"lookup first {mode} skew {d.skew}")
        d = devices[3]
        assert_hits(batch, None, d.call(g.search_hits, ranges=False)[1], f"lookup first {mode}, counts only")
        only = d.call(g.search_hits, counts=False)[0]
        _check_hits_contract(only, batch.counts, batch.sp, batch.ep, batch.counts)
        assert_list(batch, devices[1].hit_list(g), f"lookup first {mode}")
    for knob in ("1", "0"):
        monkeypatch.setenv("AWFM_GPU_EXACT_LOOKUP", knob)
        for d in devices:
            ranges, counts = d.call(g.search)
            assert g.last_search_was_exact_lookup() == (knob == "1")
            assert_exact(batch, ranges, counts, f"exact lookup {knob} skew {d.skew}")
    g.destroy()


def test_mixed_length_lookup_kernel(oracle, awfm, require_gpu, wide, monkeypatch):
    """the mixed-length lookup kernel ($AWFM_GPU_MIXED_LOOKUP=1) and the ordered kernels it replaces (=0), forced as in
    test_mixed_length_lookup_first_keeps_hits_bit_identical; then the exact lookup kernel on the same batch"""
    import torch
    batch = batch_of(awfm, oracle, bv.DNA, (1, 40))
    g = image_of(awfm, batch, wide, ordered=1)
    assert g.search_hits_is_ordered(True, 0, batch.Q)
    devices = [Device(torch, batch, skew) for skew in range(4)]
    for mode in ("1", "0"):
        monkeypatch.setenv("AWFM_GPU_MIXED_LOOKUP", mode)
        for d in devices:
            ranges, counts = d.call(g.search_hits)
            assert g.last_ordered_kernel_is_lookup() == (mode == "1")
            assert_hits(batch, ranges, counts, f"mixed lookup {mode} skew {d.skew}")
        assert_hits(batch, None, devices[3].call(g.search_hits, ranges=False)[1], f"mixed lookup {mode}, counts only")
        assert_list(batch, devices[2].hit_list(g), f"mixed lookup {mode}")
    monkeypatch.setenv("AWFM_GPU_EXACT_LOOKUP", "1")
    for d in devices:
        ranges, counts = d.call(g.search)
        assert g.last_search_was_exact_lookup()
        assert_exact(batch, ranges, counts, f"exact lookup, mixed lengths, skew {d.skew}")
    g.destroy()


@pytest.mark.parametrize("K", [13, 12])
def test_amino_lookup_kernel(oracle, awfm, require_gpu, wide, monkeypatch, K):
    """aminoLookupSearchKernel<K> forced as in test_amino_lookup_first_keeps_hits_bit_identical: a byte of index 20 among the deeper
    table's characters sends the k-mer back to the index's own table -- where the reference's carry, or the letter-by-letter
    search, decides"""
    import torch
    monkeypatch.setenv("AWFM_GPU_AMINO_LOOKUP", "1")
    batch = batch_of(awfm, oracle, bv.AMINO, K)
    g = image_of(awfm, batch, wide)
    devices = [Device(torch, batch, skew) for skew in range(4)]
    for d in devices:
        ranges, counts = d.call(g.search_hits)
        assert g.last_ordered_kernel_is_lookup()
        assert_hits(batch, ranges, counts, f"amino lookup skew {d.skew}")
    assert_hits(batch, None, devices[3].call(g.search_hits, ranges=False)[1], "amino lookup, counts only")
    assert_list(batch, devices[1].hit_list(g), "amino lookup")
    g.destroy()


@ALPHABETS
def test_longest_suffix_match_and_one_substitution_search(oracle, awfm, require_gpu, wide, alphabet):
    """against their host twins (which go letter by letter through awfm_letters.c), with and without the tables"""
    batch = batch_of(awfm, oracle, alphabet, (1, 40))
    few = batch.first_alias + len(batch.aliases)  # the base strings, the variants and the alias pairs
    strings = batch.strings[:few]
    chars, offsets = bv.csr(strings)
    starts, ends = offsets[:-1].copy(), offsets[1:].copy()
    want = twin(("longest match", alphabet), lambda: awfm.longest_suffix_matches_host(batch.ix, chars, starts, ends, threads=16))
    assert (want[0] < (ends - starts)).any() and (want[0] >= 20).any()
    for j, v in enumerate(batch.aliases):  # the alias property on the twin's own answers
        assert all(np.array_equal(w[batch.first_alias + j], w[v.source]) for w in want), v.value
    one = [s for s in strings[::7] if len(s) >= 2]
    assert {c for s in one for c in s} == set(bv.query_bytes(alphabet))
    one_chars, one_offsets = bv.csr(one)
    want_one = twin(("one substitution", alphabet), lambda: awfm.one_substitution_search_host(batch.ix, one_chars, one_offsets, threads=16))
    assert want_one[3] > 500
    g = awfm.GpuIndex(batch.ix)
    assert bool(g.is_wide) == bool(wide)
    for what in glm._configurations(g, alphabet == bv.AMINO, batch.deep_k):
        for skew in range(4):
            glm._same(glm._device(g, chars, starts, ends, skew=skew), want, (what, skew))
            gos._same(gos._device(g, one_chars, one_offsets, capacity=want_one[3] + 64, skew=skew), want_one, (what, skew))
    g.destroy()


@ALPHABETS
def test_pack_unpack_and_the_packed_search(oracle, awfm, require_gpu, alphabet):
    """awfmGpuPackKmers: the all-ones word and the bad count fall exactly on the k-mers awfmPackKmers refuses (here the sentinel class
    is sent too: packing walks no index); unpacking gives the canonical lower-case letters (u -> t); the packed search of the
    k-mers that can be packed equals the oracle"""
    import torch
    K = 12
    batch = batch_of(awfm, oracle, alphabet, K)
    rows = [s for s in batch.strings]
    for c in bv.sentinel_class(alphabet):  # every position mod 4, each of the four k-mers decoded together
        rows += [v.string for v in bv.byte_rich(batch.base, [c])]
    kmers = np.frombuffer(b"".join(rows), np.uint8).reshape(-1, K)
    index = bv.INDEX[alphabet][kmers]
    refused = (index >= bv.CARDINALITY[alphabet]).any(axis=1)
    assert refused.sum() > 1000 and (~refused).sum() > 1000
    bits = 2 if alphabet == bv.DNA else 5
    want = np.zeros(len(kmers), np.uint64)
    for column in range(K):
        want = (want << np.uint64(bits)) | (index[:, column].astype(np.uint64) & np.uint64((1 << bits) - 1))
    want[refused] = np.uint64(0xFFFFFFFFFFFFFFFF)
    with pytest.raises(ValueError) as e:  # the host's packing refuses the same k-mers: the first of them
        awfm.pack_kmers(kmers, alphabet)
    assert f"k-mer {np.flatnonzero(refused)[0]} " in str(e.value)
    assert np.array_equal(awfm.pack_kmers(kmers[~refused], alphabet), want[~refused])
    g = awfm.GpuIndex(batch.ix)
    canonical = np.frombuffer(b"acgt" if alphabet == bv.DNA else bv.AMINO_LETTERS.encode(), np.uint8)
    for skew in range(4):
        d_chars = torch.from_numpy(np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), kmers.reshape(-1), np.full(GUARD, PATTERN, np.uint8)))).to("cuda")
        d_packed = torch.full((len(kmers) + 2 * EDGE,), 7, dtype=torch.int64, device="cuda")
        assert g.pack_device(d_chars.data_ptr() + GUARD + skew, K, len(kmers), d_packed.data_ptr() + 8 * EDGE) == int(refused.sum())
        torch.cuda.synchronize()
        packed = d_packed.cpu().numpy()
        assert (packed[:EDGE] == 7).all() and (packed[EDGE + len(kmers):] == 7).all()
        bad = np.flatnonzero(packed[EDGE:EDGE + len(kmers)].view(np.uint64) != want)
        assert not len(bad), (skew, bytes(kmers[bad[0]]), hex(int(packed[EDGE + bad[0]])), hex(int(want[bad[0]])))
    good = np.flatnonzero(~refused)
    d_good = torch.from_numpy(want[good].view(np.int64)).to("cuda")
    d_back = torch.full((len(good) * K + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    g.unpack_device(d_good.data_ptr(), K, len(good), d_back.data_ptr() + GUARD)
    torch.cuda.synchronize()
    back = d_back.cpu().numpy()
    assert (back[:GUARD] == PATTERN).all() and (back[GUARD + len(good) * K:] == PATTERN).all()
    assert np.array_equal(back[GUARD:GUARD + len(good) * K].reshape(-1, K), canonical[index[good]])
    # the packed search of the k-mers of the batch that can be packed (they hold proper letters only: the oracle's all the way)
    mine = good[good < batch.Q]
    d_mine = torch.from_numpy(want[mine].view(np.int64)).to("cuda")
    d_ranges = torch.full((2 * len(mine),), 7, dtype=torch.int64, device="cuda")
    d_counts = torch.full((len(mine),), 7, dtype=torch.int32, device="cuda")
    d_scratch = torch.zeros(len(mine) * K + 64, dtype=torch.uint8, device="cuda")
    g.search_hits_packed(d_mine.data_ptr(), K, len(mine), d_ranges.data_ptr(), d_counts.data_ptr(), d_scratch.data_ptr())
    torch.cuda.synchronize()
    assert (batch.counts[mine] > 0).sum() > 500
    _check_hits_contract(d_ranges.cpu().numpy().view(np.uint64).reshape(-1, 2), d_counts.cpu().numpy().view(np.uint32), batch.sp[mine], batch.ep[mine], batch.counts[mine])
    g.destroy()


# ---- the read path ------------------------------------------------------------------------------------------------------------
BANDS = ((3, 4), (8, 15), (20, 23))  # 11, 32 and 64 diagonals: groups of 16, 32 and 64 lanes
assert [gr.natural_group(w, x) for w, x in BANDS] == [16, 32, 64]
SCORINGS = (af.DEFAULT, (2, 4, 4, 2), (1, 1, 0, 1))
_CASES, _TWINS = {}, {}


class Image:
    """an image whose index is built from a well-formed text of the case's length, with the case's byte-rich text and its record
    table installed: the calls of the read path take the image for its text, record table and alphabet only"""

    def __init__(self, awfm, case):
        well_formed = bv.well_formed_text(7, len(case.text), case.alphabet, ambiguity_runs=2)
        self.ix = awfm.create_index(well_formed, case.alphabet, 2, 2)
        self.g = awfm.GpuIndex(self.ix)
        self.g.set_text(case.text)
        assert self.g.text_length == len(case.text)
        if case.ends is not None:
            self.g.set_record_table(case.ends)

    def close(self):
        self.g.destroy()
        self.ix.dealloc()


def read_case(kind, alphabet):
    """the byte-rich batch of one call: 600 reads in a text of 2^14 positions, a third of all bytes replaced; every byte value
    stands at every position mod 4 of the read buffer and of the text"""
    key = (kind, alphabet)
    if key not in _CASES:
        shape = dict(text_length=1 << 14, num_records=19, max_length=90)
        if kind == "verify":
            case = vc.random_case(61 + alphabet, 600, 4, alphabet, **shape)
        elif kind == "align":
            case = ac.random_case(62 + alphabet, 600, 4, alphabet, hanging=0.2, **shape)
        elif kind == "affine":
            case = af.random_case(63 + alphabet, 600, 4, alphabet, hanging=0.2, **shape)
        elif kind == "score":
            case = sc.random_case(64 + alphabet, 600, 4, alphabet, hanging=0.2, **shape)
        else:
            case = ws.random_case(65 + alphabet, 600, alphabet, text_length=1 << 14, num_records=19, max_length=90, max_window=300)
        case = bv.enrich_case(case, 70 + alphabet)
        bv.assert_every_value(case.read_chars, "reads", by_residue=True)
        bv.assert_every_value(case.text, "text", by_residue=True)
        for c in bv.sentinel_class(alphabet):
            assert c in case.read_chars and c in case.text
        _CASES[key] = case
    return _CASES[key]


def twin(key, call):
    """a host twin's outputs, computed once for the skews they are compared at"""
    if key not in _TWINS:
        _TWINS[key] = call()
    return _TWINS[key]


@ALPHABETS
def test_verification_of_byte_rich_reads(awfm, require_gpu, alphabet):
    import torch
    case = read_case("verify", alphabet)
    b = vc.Builder(bv.PAIR_RECORDS[alphabet], alphabet=alphabet)
    b.add("equal up to alias", bv.ALIAS_READ[alphabet], 0, 24, 0, 0, 24, 0)
    b.add("equal non-letters do not match", bv.NON_LETTERS[alphabet], 0, 24, 1, 0, 24, 24)
    b.add("non-letters against letters", bv.NON_LETTERS[alphabet], 0, 24, 0, 0, 24, 24)
    image = Image(awfm, case)
    try:
        # the slots' text intervals begin at every position mod 4 of the text
        begins = case.slots["chainReadBegins"].astype(np.int64) + case.slots["chainBeginDiagonals"]
        assert {int(v) % 4 for v in begins[case.slots["sequences"] != vc.NONE]} == {0, 1, 2, 3}
        for w, x in BANDS:
            want = twin(("verify", alphabet, w), lambda: case.host(awfm, w, x, threads=16, unverified_before=5))
            assert ((want["editDistances"] > 0) & (want["editDistances"] < 90)).sum() > 500
            for skew in range(4):
                vc.assert_equal(gvc.DeviceCall(awfm, torch, case, skew=skew)(image.g, w, x, unverified_before=5), want, what=f"w={w} x={x} skew {skew}")
    finally:
        image.close()
    image = Image(awfm, b.case())
    try:
        for skew in range(4):
            got = gvc.DeviceCall(awfm, torch, b.case(), skew=skew)(image.g, 2, 3)
            assert np.array_equal(got["editDistances"], b.want()), (skew, got["editDistances"].tolist())
    finally:
        image.close()


@ALPHABETS
def test_alignment_of_byte_rich_reads(awfm, require_gpu, alphabet):
    import torch
    case = read_case("align", alphabet)
    image = Image(awfm, case)
    try:
        scratch = gac.Scratch(torch, image.g, 256)
        for w, x in BANDS:
            want = twin(("align", alphabet, w), lambda: case.host(awfm, w, x, 64, threads=16, unaligned_before=5, truncated_before=3))
            assert (want["editDistances"] < 90).sum() > 300
            for skew in range(4):
                got = gac.DeviceCall(awfm, torch, case, skew=skew)(image.g, w, x, scratch, max_ops=64, unaligned_before=5, truncated_before=3)
                ac.assert_equal(got, want, what=f"w={w} x={x} skew {skew}", fill=PATTERN)
    finally:
        image.close()
    b = ac.Builder(bv.PAIR_RECORDS[alphabet], alphabet=alphabet)
    b.add("equal up to alias", bv.ALIAS_READ[alphabet], 0, 0, 0, (0, 0, 24, "24="))
    b.add("equal non-letters do not match", bv.NON_LETTERS[alphabet], 1, 0, 0, None)
    image = Image(awfm, b.case())
    try:
        want = b.case().host(awfm, 2, 3, 64)
        assert int(want["editDistances"][0]) == 0 and int(want["editDistances"][1]) == 24
        for skew in range(4):
            got = gac.DeviceCall(awfm, torch, b.case(), skew=skew)(image.g, 2, 3, gac.Scratch(torch, image.g, 64), max_ops=64)
            ac.assert_equal(got, want, what=f"pairs, skew {skew}", fill=PATTERN)
            assert ac.cigar(ac.runs_of(got["ops"][0], int(got["numOps"][0]))) == "24=" and "=" not in ac.cigar(ac.runs_of(got["ops"][1], int(got["numOps"][1])))
    finally:
        image.close()


@ALPHABETS
def test_affine_alignment_of_byte_rich_reads(awfm, require_gpu, alphabet):
    import torch
    case = read_case("affine", alphabet)
    image = Image(awfm, case)
    try:
        scratch = gaa.Scratch(torch, image.g, 256)
        calls = [gaa.DeviceCall(awfm, torch, case, skew=skew) for skew in range(4)]
        for (w, x), scoring in zip(BANDS, SCORINGS):
            want = twin(("affine", alphabet, w), lambda: case.host(awfm, w, x, scoring, 64, threads=16, unaligned_before=5, truncated_before=3))
            assert ((want["scores"] > 0) & (want["scores"] < af.TOO_LONG)).sum() > 300
            for skew, call in enumerate(calls):
                got = call(image.g, w, x, scratch, scoring=scoring, max_ops=64, unaligned_before=5, truncated_before=3)
                af.assert_equal(got, want, what=f"w={w} x={x} {scoring} skew {skew}", fill=PATTERN)
    finally:
        image.close()
    b = af.Builder(bv.PAIR_RECORDS[alphabet], alphabet=alphabet)
    b.add("equal up to alias", bv.ALIAS_READ[alphabet], 0, 0, 0, (24, 0, 24, 0, 24, "24="))
    b.add("equal non-letters do not match", bv.NON_LETTERS[alphabet], 1, 0, 0, 0)
    image = Image(awfm, b.case())
    try:
        for skew in range(4):
            got = gaa.DeviceCall(awfm, torch, b.case(), skew=skew)(image.g, 2, 3, gaa.Scratch(torch, image.g, 64), max_ops=64)
            b.check(got, 64)
    finally:
        image.close()


@ALPHABETS
def test_slot_scores_of_byte_rich_reads(awfm, require_gpu, alphabet):
    import torch
    case = read_case("score", alphabet)
    image = Image(awfm, case)
    try:
        calls = [gsc.DeviceCall(awfm, torch, case, skew=skew) for skew in range(4)]
        for (w, x), scoring in zip(BANDS, SCORINGS):
            want = twin(("score", alphabet, w), lambda: case.score(awfm, w, x, scoring, min_score=2, threads=16, unscored_before=5, mapped_before=3))
            assert want["numMapped"] > 3 + 300
            for call in calls:
                sc.assert_equal(call(image.g, w, x, scoring=scoring, min_score=2, unscored_before=5, mapped_before=3), want, what=f"w={w} x={x} {scoring}")
    finally:
        image.close()
    b = sc.Builder(bv.PAIR_RECORDS[alphabet], 2, alphabet)
    b.add("equal up to alias", bv.ALIAS_READ[alphabet], [(0, 0, 0), (1, 0, 0)], (0, 24, sc.NO_SLOT, 0, 60), [24, 0])
    b.add("equal non-letters do not match", bv.NON_LETTERS[alphabet], [(1, 0, 0), (0, 0, 0)], (sc.NO_SLOT, 0, sc.NO_SLOT, 0, 0), [0, 0])
    image = Image(awfm, b.case())
    try:
        for skew in range(4):
            b.check(gsc.DeviceCall(awfm, torch, b.case(), skew=skew)(image.g, 2, 3))
    finally:
        image.close()


@ALPHABETS
@pytest.mark.parametrize("q", gws.TIERS, ids=["natural", "4", "8", "12"])
def test_window_scores_of_byte_rich_reads(awfm, require_gpu, diag, alphabet, q):
    """the window kernel's packed text letters and its 6-bit row letter, at the natural number of columns per lane and with 4, 8
    and 12 forced"""
    import torch
    diag(window_q=q)
    case = read_case("window", alphabet)
    image = Image(awfm, case)
    try:
        assert {int(v) % 4 for v in case.begins[case.sequences != ws.UNUSED]} == {0, 1, 2, 3}
        calls = [gws.DeviceCall(awfm, torch, case, skew=skew) for skew in range(4)]
        for scoring in SCORINGS:
            want = twin(("window", alphabet, scoring), lambda: gws.twin(awfm, case, scoring=scoring, min_score=3, unscored_before=5, found_before=3))
            assert want["numFound"] > 3 + 200
            for call in calls:
                ws.assert_equal(call(image.g, scoring=scoring, min_score=3, unscored_before=5, found_before=3), want, what=str(scoring))
    finally:
        image.close()
    b = ws.Builder(bv.PAIR_RECORDS[alphabet], alphabet)
    b.add("equal up to alias", bv.ALIAS_READ[alphabet], (0, 0, 24), (24, 0, 24, 0, 24))
    b.add("equal non-letters do not match", bv.NON_LETTERS[alphabet], (1, 0, 24), ws.NOTHING)
    b.add("non-letters against letters", bv.NON_LETTERS[alphabet], (0, 0, 24), ws.NOTHING)
    image = Image(awfm, b.case())
    try:
        for skew in range(4):
            b.check(gws.DeviceCall(awfm, torch, b.case(), skew=skew)(image.g))
    finally:
        image.close()


def test_reverse_complement_of_all_byte_values_at_every_alignment(awfm, require_gpu):
    """complementOfFour: every value at every position mod 4 of a read, counted from its front and from its back; input and output
    0 to 3 bytes into their allocations, independently"""
    import torch
    lengths = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 100, 255, 257] * 4
    offsets = np.concatenate(([3], 3 + np.cumsum(lengths))).astype(np.uint64)
    chars = np.random.default_rng(3).permutation(256).astype(np.uint8)[np.arange(int(offsets[-1])) % 257 % 256]  # (a period that is odd)
    bv.assert_every_value(chars[3:], "reads", by_residue=True)
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3}
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtaacc", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    g = awfm.GpuIndex(ix)  # the call takes the image for its device only
    d_offsets = _upload(torch, offsets)
    for which in (pm.ALL, pm.ODD):
        want, _ = awfm.reverse_complement_reads_host(chars, offsets, which, threads=16, fill=PATTERN)
        assert np.array_equal(want, pm.reverse_complement(chars, offsets, which, fill=PATTERN)[0])
        for skew_in in range(4):
            for skew_out in range(4):
                d_chars = torch.from_numpy(np.concatenate((np.full(GUARD + skew_in, PATTERN, np.uint8), chars, np.full(GUARD, PATTERN, np.uint8)))).to("cuda")
                d_out = torch.full((chars.size + 2 * GUARD + skew_out,), PATTERN, dtype=torch.uint8, device="cuda")
                g.reverse_complement_reads(d_chars.data_ptr() + GUARD + skew_in, chars.size, d_offsets.data_ptr(), len(lengths),
                                           d_out.data_ptr() + GUARD + skew_out, which)
                torch.cuda.synchronize()
                raw = d_out.cpu().numpy()
                assert (raw[:GUARD + skew_out] == PATTERN).all() and (raw[GUARD + skew_out + chars.size:] == PATTERN).all(), (skew_in, skew_out)
                assert np.array_equal(raw[GUARD + skew_out:GUARD + skew_out + chars.size], want), (which, skew_in, skew_out)
    g.destroy()
    ix.dealloc()


# ---- the GPU builder ----------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[False, True], ids=["pos32", "pos64"])
def build_wide(request, diag):
    diag(build_wide="1" if request.param else None)
    return request.param


@pytest.mark.parametrize("n", [4096, 100_003])
def test_builder_on_a_nucleotide_text_of_every_byte_value(oracle, awfm, require_gpu, build_wide, n):
    """sanitizeKernel, packKmersKernel and bwtBlockKernel on a text a third of whose bytes are anything but the sentinel class: the
    arrays are the host builder's byte for byte, and the byte-rich search on that index equals the oracle"""
    import torch
    rng = np.random.default_rng(n)
    text = bv.well_formed_text(n, n, bv.DNA)
    allowed = np.array(bv.query_bytes(bv.DNA), np.uint8)
    odd = np.flatnonzero(rng.random(n) < 1 / 3)
    for r in range(4):  # every value at every position mod 4
        mine = odd[odd % 4 == r]
        text[mine] = allowed[np.arange(mine.size) % allowed.size]
    assert bv.values_by_residue(text) >= {(int(c), r) for c in allowed for r in range(4)}
    assert not np.isin(text, bv.sentinel_class(bv.DNA)).any()
    for ratio, k in ((8, 6), (3, 3)):
        host = _host_build(awfm, text, awfm.AwFmAlphabetDna, ratio, k)
        dev = awfm.gpu_create_index(text, awfm.AwFmAlphabetDna, ratio, k)
        _same_arrays(host, dev)
        host.dealloc()
        if (ratio, k) != (8, 6):
            dev.dealloc()
            continue
        oi = oracle.Index.wrap(oracle.DNA, ratio, k, dev.bwt_length, dev.blocks(), dev.prefix_sums(), dev.seed_table(), dev.packed_sa())
        clean = bv.NUC_SANITIZED[text]  # queries are cut from what the index stores: x wherever the text has no letter
        strings, base, variants, aliases, first_variant, first_alias = bv.search_batch(n, clean, bv.DNA, (1, 40), fill=2000)
        bv.check_coverage(variants, bv.query_bytes(bv.DNA), first=first_variant)
        chars, offsets = bv.csr(strings)
        sp, ep, counts, _ = oi.batch_search(chars, offsets, threads=4)
        assert bv.classes_with_hits(bv.DNA, strings, counts) == bv.all_query_classes(bv.DNA)
        g = awfm.GpuIndex(dev)
        ranges, got_counts = g.count_host(chars, offsets)
        assert np.array_equal(ranges[:, 0], sp) and np.array_equal(ranges[:, 1], ep) and np.array_equal(got_counts, counts)
        bv.assert_alias_property(aliases, first_alias, ranges[:, 0], ranges[:, 1], "GPU-built index")
        g.destroy()
        dev.dealloc()


@pytest.mark.parametrize("n", [4096, 100_003])
def test_builder_on_a_well_formed_amino_text_the_sanitiser_changes(awfm, require_gpu, build_wide, n):
    """one case of letters, with b x B X and NUL among them, which the sanitiser turns into z (an ill-formed amino text is not given
    to the GPU builder: its accelerator builders walk the index)"""
    rng = np.random.default_rng(n + 1)
    text = rng.choice(np.frombuffer(bv.AMINO_LETTERS.encode(), np.uint8), n).astype(np.uint8)
    odd = np.flatnonzero(rng.random(n) < 0.02)
    text[odd] = np.frombuffer(b"bxBX\x00", np.uint8)[np.arange(odd.size) % 5]
    assert all(c in text for c in b"bxBX\x00") and set(bv.AMINO_SANITIZED[text].tolist()) == set(bv.AMINO_LETTERS.encode()) | {ord("z")}
    for ratio, k in ((8, 3), (5, 2)):
        host = _host_build(awfm, text, awfm.AwFmAlphabetAmino, ratio, k)
        dev = awfm.gpu_create_index(text, awfm.AwFmAlphabetAmino, ratio, k)
        _same_arrays(host, dev)
        host.dealloc()
        dev.dealloc()
