"""The list of hits (awfmGpuSearchHitsCompact) of the four kernels that collect it per wave -- lookupSearchKernel,
orderedSearchKernel<..., LIST>, mixedLookupSearchKernel, aminoLookupSearchKernel: one table of cases for all of them, against the
CPU oracle and against the dense results of the same batch.  What the cases are after is the code the kernels share
(awfm_search_parts_kernel.h: HitList): the appends into a wave's 32-entry buffer, the flushes when it fills, the one
reservation the last wave of a workgroup makes for all leftovers, and the clipping at the list's capacity.

Routes (how a batch reaches its kernel; the text is 200 000 letters, seed table 8 and deeper table 12 for nucleotides, 3 and 5
for amino acids, as the amino list tests of test_gpu_parity.py have them):
  lookup   fixed-length 21-mers, $AWFM_GPU_LOOKUP_FIRST=1: lookupSearchKernel.  A wave has 64 slots for the survivors of a
           round of 256 k-mers; the others go through the ordering passes to orderedSearchKernel<LIST>, so a batch of planted
           k-mers -- all 256 of a round alive -- has both kernels append to the one list (awfmGpuLastOrderedKept: every k-mer kept).
  ordered  the same batches with $AWFM_GPU_LOOKUP_FIRST=0: every k-mer through orderedSearchKernel<LIST>.
  mixed    lengths 8..30 through offsets, $AWFM_GPU_MIXED_LOOKUP=1: mixedLookupSearchKernel (k-mers of up to 12 characters are
           settled by their table entry and listed a round at a time; the longer ones go through the wave's buffer).
  amino    10-mers, $AWFM_GPU_AMINO_LOOKUP=1: aminoLookupSearchKernel.
Every route runs with 32-bit and with 64-bit positions in the kernels, and every case at buffer misalignments 0 and 3."""
import os

import numpy as np
import pytest

from avxwindowfmindex_amd import synth

pytestmark = pytest.mark.gpu

N = 200_000
FILL_KMER = 0xFFFFFFFF  # what the search fills the list's capacity with before anything is appended: {0xFFFFFFFF, {1, 0}}
GUARD = 64              # entries behind the capacity, which nothing may write
GUARD_KMER, GUARD_WORD = 0x5A5A5A5A, 7

ROUTES = {
    #          alphabet, what forces the kernel,           k-mer lengths
    "lookup": ("dna", ("AWFM_GPU_LOOKUP_FIRST", "1"), (21, 21)),
    "ordered": ("dna", ("AWFM_GPU_LOOKUP_FIRST", "0"), (21, 21)),
    "mixed": ("dna", ("AWFM_GPU_MIXED_LOOKUP", "1"), (8, 30)),
    "amino": ("amino", ("AWFM_GPU_AMINO_LOOKUP", "1"), (10, 10)),
}
#        Q, k-mers drawn from the text (None: all), capacity = hits // 2 instead of Q
CASES = {
    "all_planted": (3 * 256 + 31, None, False),   # (a) every wave flushes its buffer several times; the last round is short
    "five_planted": (1024, 5, False),             # (b) no flush: only the last wave's reservation
    "no_hit": (1024, 0, False),                   # (c) nothing is appended: the count is 0 and the fill stays
    "half_capacity": (3 * 256 + 31, None, True),  # (d) the batch of (a) into a list half as long as its hits
}


class _Image:
    """an index of the 200 000-letter text, its oracle twin and its device image; the batches of the cases, made once"""

    def __init__(self, oracle, awfm, alphabet, wide):
        amino = alphabet == "amino"
        letters = synth.AMINO_ALPHABET if amino else synth.DNA_ALPHABET
        self.letters = letters
        self.txt = synth.text(4100 + amino, N, letters).copy()
        seed_k, deep_k = (3, 5) if amino else (8, 12)
        self.ix = awfm.create_index(self.txt, awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 8, seed_k)
        self.oi = oracle.Index.wrap(oracle.AMINO if amino else oracle.DNA, 8, seed_k, self.ix.bwt_length, self.ix.blocks(),
                                    self.ix.prefix_sums(), self.ix.seed_table(), self.ix.packed_sa())
        before = os.environ.get("AWFM_GPU_FORCE_WIDE")
        os.environ["AWFM_GPU_FORCE_WIDE"] = "1" if wide else "0"  # read when the image is created
        try:
            self.g = awfm.GpuIndex(self.ix)
        finally:
            if before is None:
                del os.environ["AWFM_GPU_FORCE_WIDE"]
            else:
                os.environ["AWFM_GPU_FORCE_WIDE"] = before
        assert self.g.is_wide == wide
        if not amino:
            self.g.set_ordered(1)
        self.g.set_deep_seed(deep_k)
        self.batches = {}

    def batch(self, lengths, case):
        """(chars, offsets, sp, ep, cnt) of a case for k-mers of lengths[0]..lengths[1] characters: `planted` k-mers drawn from
        the text at seeded places among seeded random k-mers that the oracle does not find in it"""
        Q, planted, _ = CASES[case]
        planted = Q if planted is None else planted
        key = (lengths, Q, planted)  # (d) is the batch of (a)
        if key in self.batches:
            return self.batches[key]
        lo, hi = lengths
        rng = np.random.default_rng(1000 * lo + hi + planted)
        lut = np.frombuffer(self.letters, np.uint8)
        # absent k-mers: random candidates (a random 8-mer is in a 200 000-letter text 19 times in 20), kept when the oracle says so
        kmers = []
        while len(kmers) < Q - planted:
            lens = rng.integers(lo, hi + 1, 4096)
            cand = [lut[rng.integers(0, len(lut), l)] for l in lens]
            off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
            _, _, cnt, _ = self.oi.batch_search(np.concatenate(cand), off)
            kmers += [c for c, n in zip(cand, cnt) if n == 0]
        kmers = kmers[:Q - planted]
        for _ in range(planted):
            l = int(rng.integers(lo, hi + 1))
            at = int(rng.integers(0, N - l + 1))
            kmers.append(self.txt[at:at + l])
        kmers = [kmers[i] for i in rng.permutation(Q)]
        chars = np.ascontiguousarray(np.concatenate(kmers), dtype=np.uint8)
        offsets = np.concatenate([[0], np.cumsum([len(k) for k in kmers])]).astype(np.uint64)
        sp, ep, cnt, _ = self.oi.batch_search(chars, offsets)
        assert int((cnt > 0).sum()) == planted
        self.batches[key] = (chars, offsets, sp, ep, cnt)
        return self.batches[key]

    def close(self):
        self.g.destroy()
        self.ix.dealloc()


@pytest.fixture(scope="module", params=["narrow", "wide"])
def images(request, oracle, awfm, require_gpu):
    made = {}

    def get(alphabet):
        if alphabet not in made:
            made[alphabet] = _Image(oracle, awfm, alphabet, request.param == "wide")
        return made[alphabet]

    yield get
    for image in made.values():
        image.close()


@pytest.mark.parametrize("mis", [0, 3])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("route", list(ROUTES))
def test_hit_list_of_every_kernel_that_collects_it(images, monkeypatch, route, case, mis):
    import torch
    alphabet, (name, value), lengths = ROUTES[route]
    image = images(alphabet)
    g = image.g
    monkeypatch.setenv(name, value)
    Q, _, halved = CASES[case]
    chars, offsets, sp, ep, cnt = image.batch(lengths, case)
    has = np.flatnonzero(cnt > 0)
    capacity = len(has) // 2 if halved else Q
    assert 0 < capacity and (not halved or capacity < len(has))
    dev = torch.device("cuda")
    buf = torch.zeros(chars.size + 64, dtype=torch.uint8, device=dev)
    buf[mis:mis + chars.size] = torch.from_numpy(chars).to(dev)
    fixed = lengths[0] if lengths[0] == lengths[1] else 0
    d_off = None if fixed else torch.from_numpy(offsets.view(np.int64)).to(dev)
    off_ptr = 0 if fixed else d_off.data_ptr()
    d_kmers = torch.full((capacity + GUARD,), GUARD_KMER, dtype=torch.int32, device=dev)
    d_list = torch.full(((capacity + GUARD) * 2,), GUARD_WORD, dtype=torch.int64, device=dev)
    d_num = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    g.search_hits_compact(buf.data_ptr() + mis, off_ptr, fixed, Q, d_kmers.data_ptr(), d_list.data_ptr(), capacity, d_num.data_ptr())
    torch.cuda.synchronize()
    # the kernel the route names took the batch
    assert g.last_ordered_kernel_is_lookup() == (route != "ordered")
    if route == "lookup" and case in ("all_planted", "half_capacity"):
        # every k-mer is alive behind its table entry: 64 of a wave's round of 256 in its slots, 192 on to orderedSearchKernel<LIST>
        assert g.last_ordered_kept() == Q
    listed = int(d_num.cpu().numpy().view(np.uint32)[0])
    ids = d_kmers.cpu().numpy().view(np.uint32)
    ranges = d_list.cpu().numpy().view(np.uint64).reshape(-1, 2)
    print(f"{route} {case} mis={mis}: {listed} listed, {len(has)} k-mers with hits, capacity {capacity}")
    # the true number of k-mers with hits, whatever the capacity
    assert listed == len(has)
    # nothing behind the capacity is touched
    assert np.all(ids[capacity:] == GUARD_KMER) and np.all(ranges[capacity:] == GUARD_WORD)
    stored = min(listed, capacity)
    # the entries behind the hits keep the fill
    assert np.all(ids[stored:capacity] == FILL_KMER)
    assert np.all(ranges[stored:capacity, 0] == 1) and np.all(ranges[stored:capacity, 1] == 0)
    order = np.argsort(ids[:stored], kind="stable")
    ids, ranges = ids[:stored][order], ranges[:stored][order]
    if halved:
        # distinct k-mers that have hits, each with its oracle range
        assert stored == capacity and len(np.unique(ids)) == capacity and np.all(np.isin(ids, has))
        assert np.array_equal(ranges[:, 0], sp[ids]) and np.array_equal(ranges[:, 1], ep[ids])
        return
    # the sorted list is the oracle's (number, sp, ep) of every k-mer with hits ...
    assert np.array_equal(ids, has)
    assert np.array_equal(ranges[:, 0], sp[has]) and np.array_equal(ranges[:, 1], ep[has])
    # ... and what the dense results of the same buffer say
    d_ranges = torch.full((Q * 2,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((Q,), 7, dtype=torch.int32, device=dev)
    g.search_hits(buf.data_ptr() + mis, off_ptr, fixed, Q, d_ranges.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    dense_counts = d_counts.cpu().numpy().view(np.uint32)
    dense_ranges = d_ranges.cpu().numpy().view(np.uint64).reshape(Q, 2)
    dense_has = np.flatnonzero(dense_counts > 0)
    assert np.array_equal(ids, dense_has) and np.array_equal(ranges, dense_ranges[dense_has])
    assert np.array_equal(dense_counts, cnt)
