"""The kernels on the texts of index_geometry_common.py: BWT lengths that end on, one past and well past a device block
(128 positions) and a host block (256), and a sentinel row at every slice edge of a device block from both sides, in the
first, an interior and the last block -- with batches of queries whose sp - 1 and ep are asserted to meet these rows.

Every answer is compared bit for bit, on every query, with what tests/test_index_geometry.py pins to a brute force, the
step walks and the compiled reference at exactly these inputs: the oracle's ranges, hit offsets and positions, the host
twins' longest suffix matches and one-substitution records, and the suffix array of a plain sort for a locate of every BWT
row.  One test per flavour and width loops over the flavour's texts; the first HIP error ends it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_geometry_common as igc  # noqa: E402
import test_gpu_longest_match as longest  # noqa: E402  (its _device, _same and _configurations)
import test_gpu_one_substitution as subst  # noqa: E402  (its _device and _same)
from test_gpu_reference_parity import device_locate_all  # noqa: E402

pytestmark = pytest.mark.gpu


class Batch:
    """the text's queries on the device, and pattern-filled outputs for the search calls"""

    def __init__(self, x):
        import torch
        dev = torch.device("cuda")
        self.n = len(x.queries)
        self.chars = torch.from_numpy(x.chars.copy()).to(dev)
        self.offsets = torch.from_numpy(x.offsets.view(np.int64).copy()).to(dev)
        self.ranges = torch.empty(2 * self.n + 2, dtype=torch.int64, device=dev)
        self.counts = torch.empty(self.n + 1, dtype=torch.int32, device=dev)

    def search(self, g, hits_only=False):
        import torch
        self.ranges.fill_(7)
        self.counts.fill_(7)
        (g.search_hits if hits_only else g.search)(self.chars.data_ptr(), self.offsets.data_ptr(), 0, self.n, self.ranges.data_ptr(),
                                                   self.counts.data_ptr())
        torch.cuda.synchronize()
        ranges, counts = self.ranges.cpu().numpy().view(np.uint64), self.counts.cpu().numpy().view(np.uint32)
        assert ranges[2 * self.n:].tolist() == [7, 7] and int(counts[self.n]) == 7  # nothing behind the last query is written
        return ranges[:2 * self.n].reshape(self.n, 2), counts[:self.n]


def check_search(b, g, x, what):
    """exact {sp, ep} of every query, the first empty range included"""
    ranges, counts = b.search(g)
    bad = np.flatnonzero((ranges[:, 0] != x.sp) | (ranges[:, 1] != x.ep) | (counts != x.count))
    assert bad.size == 0, (x.entry, what, [(x.queries[i], ranges[i].tolist(), int(x.sp[i]), int(x.ep[i])) for i in bad[:5]])


def check_search_hits_and_locate(awfm, b, g, x, what):
    """search_hits (in seed order where the caller has asked for it), the hit offsets from its ranges, locate"""
    import torch
    ranges, counts = b.search(g, hits_only=True)
    has_hits = x.count > 0
    assert np.array_equal(counts, x.count), (x.entry, what, "counts")
    bad = np.flatnonzero(has_hits & ((ranges[:, 0] != x.sp) | (ranges[:, 1] != x.ep)))
    assert bad.size == 0, (x.entry, what, [(x.queries[i], ranges[i].tolist(), int(x.sp[i]), int(x.ep[i])) for i in bad[:5]])
    assert (ranges[~has_hits, 0] > ranges[~has_hits, 1]).all(), (x.entry, what, "a query without hits has an empty range")
    d_hit_off = torch.full((b.n + 2,), 7, dtype=torch.int64, device="cuda")
    d_scratch = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(b.n), dtype=torch.uint8, device="cuda")
    total = g.hit_offsets(b.ranges.data_ptr(), b.n, d_hit_off.data_ptr(), d_scratch.data_ptr())
    assert total == int(x.hit_offsets[-1]), (x.entry, what, "total")
    d_pos = torch.full((total + 1,), 7, dtype=torch.int64, device="cuda")
    g.locate(b.ranges.data_ptr(), d_hit_off.data_ptr(), b.n, total, d_pos.data_ptr())
    torch.cuda.synchronize()
    hit_off, pos = d_hit_off.cpu().numpy().view(np.uint64), d_pos.cpu().numpy().view(np.uint64)
    assert int(hit_off[b.n + 1]) == 7 and int(pos[total]) == 7
    assert np.array_equal(hit_off[:b.n + 1], x.hit_offsets), (x.entry, what, "hit offsets")
    bad = np.flatnonzero(pos[:total] != x.positions)
    assert bad.size == 0, (x.entry, what, "positions", bad[:5].tolist(), pos[bad[:5]].tolist(), x.positions[bad[:5]].tolist())


def check_locate_of_every_row(awfm, x, wide):
    e = x.entry
    assert 0 < e.r < e.L  # rows 0 .. L - 1 are asked for: the sentinel's and the one after it (where r + 1 < L) are among them
    ending = {ratio: igc.walks_that_end_on_the_sentinel(x, ratio) for ratio in igc.RATIOS}
    assert not ending[1] and any(ending.values()), (e, "no walk ends on the sentinel's row")
    for ratio in igc.RATIOS:
        ix = x.index if ratio == x.ratio else awfm.create_index(e.text, x.alphabet, ratio, x.seed_k)
        g = awfm.GpuIndex(ix)
        assert bool(g.is_wide) == bool(wide)
        for pair in ((True, False) if not e.amino else (None,)):
            if pair is not None:
                g.set_pair_image(pair)
                assert bool(g.has_pair_image) == pair
            got = device_locate_all(g, e.L)
            bad = np.flatnonzero(got != x.suffix_array)
            assert bad.size == 0, (e, "locate of every row", ratio, pair, bad[:5].tolist(), got[bad[:5]].tolist(),
                                   x.suffix_array[bad[:5]].tolist())
        g.set_dense_sa(True)
        assert g.has_dense_sa
        got = device_locate_all(g, e.L)
        bad = np.flatnonzero(got != x.suffix_array)
        assert bad.size == 0, (e, "locate of every row, full suffix array", ratio, bad[:5].tolist(), got[bad[:5]].tolist())
        g.destroy()
        if ix is not x.index:
            ix.dealloc()


@pytest.mark.parametrize("flavour", igc.FLAVOURS)
def test_every_text_of_the_table(awfm, oracle, require_gpu, wide, flavour):
    import time
    seconds = []
    for e in igc.entries(flavour):
        x = igc.expected(awfm, oracle, e)  # (computed once, shared by the three widths)
        t0 = time.perf_counter()
        deep_k = x.seed_k + 2
        g = awfm.GpuIndex(x.index)
        assert bool(g.is_wide) == bool(wide)
        b = Batch(x)
        want_longest = x.longest
        want_subst = x.one_substitution
        cap = want_subst[True][3] + 100
        for what in longest._configurations(g, e.amino, deep_k):
            for kernel in (awfm.AWFM_GPU_KERNEL_AUTO, awfm.AWFM_GPU_KERNEL_GROUP4):  # the two that use the tables and the pair image
                g.set_kernel(kernel)
                check_search(b, g, x, (what, "kernel", kernel))
            g.set_kernel(awfm.AWFM_GPU_KERNEL_AUTO)
            for min_length in (0, 3):
                got = longest._device(g, x.chars, x.starts, x.ends, min_length=min_length)
                longest._same(got, want_longest[min_length], (e, what, "longest suffix match", min_length))
            for include_exact in (True, False):
                got = subst._device(g, x.chars, x.offsets, capacity=cap, include_exact=include_exact)
                subst._same(got, want_subst[include_exact], (e, what, "one substitution", include_exact))
        # the image with its tables again; the kernels that never use them (the reference's letter-by-letter algorithm)
        if not e.amino:
            g.set_pair_image(True)
        g.set_deep_seed(deep_k)
        for kernel in (awfm.AWFM_GPU_KERNEL_GROUP8, awfm.AWFM_GPU_KERNEL_GROUP2, awfm.AWFM_GPU_KERNEL_GROUP1):
            g.set_kernel(kernel)
            check_search(b, g, x, ("kernel", kernel))
        g.set_kernel(awfm.AWFM_GPU_KERNEL_GROUP2)  # the plain path of the one-substitution search
        for include_exact in (True, False):
            got = subst._device(g, x.chars, x.offsets, capacity=cap, include_exact=include_exact)
            subst._same(got, want_subst[include_exact], (e, "plain path", "one substitution", include_exact))
        g.set_kernel(awfm.AWFM_GPU_KERNEL_AUTO)
        if not e.amino:
            g.set_ordered(1)
            assert g.search_hits_is_ordered(True, 0, b.n)
        check_search_hits_and_locate(awfm, b, g, x, "search_hits, ordered")
        g.set_ordered(-1)
        g.destroy()
        check_locate_of_every_row(awfm, x, wide)
        seconds.append(time.perf_counter() - t0)
    print(f"\n{flavour}, wide={wide}: {len(seconds)} texts, device part {sum(seconds):.2f} s, slowest text {max(seconds):.2f} s")
