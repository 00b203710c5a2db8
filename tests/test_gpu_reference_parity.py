"""The kernels against what the reference itself answered: tests/golden/ref_*.npz, recorded from the compiled reference by
scripts/make_reference_golden.py and kept current by tests/test_reference_parity.py.  Each fixture carries the bytes of the
.awfmi file the reference wrote, so the device image is built from an index this library did not write.  Nothing here
reads the reference or the library compiled from it; nothing skips.

The fixtures' queries are of mixed length (shorter than the seed, ambiguity letters, either case); the nucleotide ones also
go through the seed-order search (set_ordered(1)), which takes such batches through its bucketed path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_common as rc  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in rc.FIXTURE_CASES]


def load(name):
    f = np.load(os.path.join(rc.GOLDEN_DIR, name + ".npz"))
    return {k: f[k] for k in f.files}


def queries_of(fx):
    chars, off = fx["chars"], fx["offsets"]
    return [bytes(chars[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def device_search(g, fx, hits_only=False):
    import torch
    dev = torch.device("cuda")
    n = len(fx["offsets"]) - 1
    d_chars = torch.from_numpy(fx["chars"].copy()).to(dev)
    d_off = torch.from_numpy(fx["offsets"].view(np.int64).copy()).to(dev)
    d_ranges = torch.full((2 * n,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((n,), 7, dtype=torch.int32, device=dev)
    (g.search_hits if hits_only else g.search)(d_chars.data_ptr(), d_off.data_ptr(), 0, n, d_ranges.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    return d_ranges.cpu().numpy().view(np.uint64).reshape(n, 2), d_counts.cpu().numpy().view(np.uint32)


def device_search_hits_and_locate(awfm, g, fx):
    """awfmGpuSearchHits, the hit offsets from its ranges, awfmGpuLocate -> (ranges, counts, hit offsets, positions)"""
    import torch
    dev = torch.device("cuda")
    n = len(fx["offsets"]) - 1
    d_chars = torch.from_numpy(fx["chars"].copy()).to(dev)
    d_off = torch.from_numpy(fx["offsets"].view(np.int64).copy()).to(dev)
    d_ranges = torch.full((2 * n,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((n,), 7, dtype=torch.int32, device=dev)
    g.search_hits(d_chars.data_ptr(), d_off.data_ptr(), 0, n, d_ranges.data_ptr(), d_counts.data_ptr())
    d_hit_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_scratch = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(n), dtype=torch.uint8, device=dev)
    total = g.hit_offsets(d_ranges.data_ptr(), n, d_hit_off.data_ptr(), d_scratch.data_ptr())
    d_pos = torch.full((max(total, 1),), -1, dtype=torch.int64, device=dev)
    g.locate(d_ranges.data_ptr(), d_hit_off.data_ptr(), n, total, d_pos.data_ptr())
    torch.cuda.synchronize()
    return (d_ranges.cpu().numpy().view(np.uint64).reshape(n, 2), d_counts.cpu().numpy().view(np.uint32),
            d_hit_off.cpu().numpy().view(np.uint64), d_pos[:total].cpu().numpy().view(np.uint64))


def check_ordered(awfm, g, fx, what):
    """search_hits in seed order (the caller has set_ordered(1)): ranges of the queries with hits, counts, hit offsets, positions"""
    n = len(fx["offsets"]) - 1
    assert g.search_hits_is_ordered(True, 0, n), what
    want_ranges = np.stack([fx["sp"], fx["ep"]], axis=1)
    has_hits = fx["count"] > 0
    ranges, counts, hit_off, pos = device_search_hits_and_locate(awfm, g, fx)
    assert np.array_equal(counts, fx["count"]), (what, "counts")
    assert np.array_equal(ranges[has_hits], want_ranges[has_hits]), (what, "ranges")
    assert (ranges[~has_hits, 0] > ranges[~has_hits, 1]).all(), (what, "a query without hits has an empty range")
    assert np.array_equal(hit_off, fx["hit_offsets"]) and np.array_equal(pos, fx["positions"]), (what, "positions")


def device_locate_all(g, bwt_length):
    """text position of every BWT position 0 .. bwt_length-1: one single-row range per position through awfmGpuLocate"""
    import torch
    dev = torch.device("cuda")
    rows = np.arange(bwt_length, dtype=np.uint64)
    d_ranges = torch.from_numpy(np.stack([rows, rows], axis=1).view(np.int64).copy()).to(dev)
    d_off = torch.from_numpy(np.arange(bwt_length + 1, dtype=np.int64)).to(dev)
    d_pos = torch.full((bwt_length,), -1, dtype=torch.int64, device=dev)
    g.locate(d_ranges.data_ptr(), d_off.data_ptr(), bwt_length, bwt_length, d_pos.data_ptr())
    torch.cuda.synchronize()
    return d_pos.cpu().numpy().view(np.uint64)


def device_longest(g, fx, min_length):
    import torch
    dev = torch.device("cuda")
    n = len(fx["offsets"]) - 1
    d_chars = torch.from_numpy(fx["chars"].copy()).to(dev)
    d_starts = torch.from_numpy(fx["offsets"][:-1].view(np.int64).copy()).to(dev)
    d_ends = torch.from_numpy(fx["offsets"][1:].view(np.int64).copy()).to(dev)
    d_len = torch.full((n,), 7, dtype=torch.int32, device=dev)
    d_ranges = torch.full((2 * n,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((n,), 7, dtype=torch.int32, device=dev)
    g.longest_suffix_matches(d_chars.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, n, min_length, d_len.data_ptr(),
                             d_ranges.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    return (d_len.cpu().numpy().view(np.uint32), d_ranges.cpu().numpy().view(np.uint64).reshape(n, 2),
            d_counts.cpu().numpy().view(np.uint32))


def check_searches(g, fx, what):
    want_ranges = np.stack([fx["sp"], fx["ep"]], axis=1)
    has_hits = fx["count"] > 0
    ranges, counts = g.count_host(fx["chars"], fx["offsets"])
    assert np.array_equal(ranges, want_ranges) and np.array_equal(counts, fx["count"]), (what, "count_host")
    ranges, hit_off, pos = g.locate_host(fx["chars"], fx["offsets"])
    assert np.array_equal(ranges, want_ranges), (what, "locate_host ranges")
    assert np.array_equal(hit_off, fx["hit_offsets"]) and np.array_equal(pos, fx["positions"]), (what, "locate_host")
    ranges, counts = device_search(g, fx)
    assert np.array_equal(ranges, want_ranges) and np.array_equal(counts, fx["count"]), (what, "search")
    ranges, counts = device_search(g, fx, hits_only=True)
    assert np.array_equal(counts, fx["count"]), (what, "search_hits counts")
    assert np.array_equal(ranges[has_hits], want_ranges[has_hits]), (what, "search_hits ranges")
    assert (ranges[~has_hits, 0] > ranges[~has_hits, 1]).all(), (what, "search_hits: a query without hits has an empty range")


@pytest.mark.parametrize("keep_sa", [True, False], ids=["sa-in-memory", "sa-on-disk"])
@pytest.mark.parametrize("name", NAMES)
def test_image_of_a_reference_written_file(awfm, require_gpu, wide, tmp_path, name, keep_sa):
    fx = load(name)
    amino = int(fx["config"][0]) == awfm.AwFmAlphabetAmino
    bwt_length = int(fx["config"][3])
    path = str(tmp_path / (name + ".awfmi"))
    fx["awfmi"].tofile(path)
    ix = awfm.read_index_from_file(path, keep_sa_in_memory=keep_sa)
    assert ix.bwt_length == bwt_length and (ix.packed_sa() is None) == (not keep_sa)
    g = awfm.GpuIndex(ix)
    assert bool(g.is_wide) == bool(wide)
    check_searches(g, fx, (name, "auto"))
    for kernel in (awfm.AWFM_GPU_KERNEL_GROUP8, awfm.AWFM_GPU_KERNEL_GROUP4, awfm.AWFM_GPU_KERNEL_GROUP2,
                   awfm.AWFM_GPU_KERNEL_GROUP1):
        g.set_kernel(kernel)
        check_searches(g, fx, (name, "kernel", kernel))
    g.set_kernel(awfm.AWFM_GPU_KERNEL_AUTO)
    if not amino:
        g.set_pair_image(False)
        assert not g.has_pair_image
        check_searches(g, fx, (name, "no pair image"))
        g.set_pair_image(True)
        # the seed-order search: ordered kernels on an image of a reference-written file, pair image on and off
        g.set_ordered(1)
        for pair in (True, False):
            g.set_pair_image(pair)
            assert bool(g.has_pair_image) == pair
            check_ordered(awfm, g, fx, (name, "seed order", "pair image", pair))
        g.set_pair_image(True)
        g.set_ordered(-1)
    assert np.array_equal(device_locate_all(g, bwt_length), fx["all_positions"]), (name, "every BWT position")
    g.set_dense_sa(True)
    assert g.has_dense_sa
    check_searches(g, fx, (name, "dense suffix array"))
    assert np.array_equal(device_locate_all(g, bwt_length), fx["all_positions"]), (name, "every BWT position, dense")
    g.set_dense_sa(False)
    # longest suffix match: the recorded walk over the reference's step functions
    walk = list(zip(fx["walk_length"].tolist(), [tuple(r) for r in fx["walk_range"].tolist()]))
    for min_length in (0, 5):
        want = rc.longest_match_expected(walk, min_length)
        got = device_longest(g, fx, min_length)
        for k, what in enumerate(("lengths", "ranges", "counts")):
            assert np.array_equal(got[k], want[k]), (name, "longest suffix match", min_length, what)
    g.destroy()
    # the array-of-structs calls of AwFmIndex.h
    queries = queries_of(fx)
    lst = awfm.KmerSearchList(len(queries))
    lst.fill(queries)
    awfm.parallel_search_count(ix, lst, 4)
    assert np.array_equal(lst.counts(), fx["count"]), (name, "awFmParallelSearchCount")
    assert awfm.parallel_search_locate(ix, lst, 4) == awfm.AwFmSuccess
    assert np.array_equal(lst.counts(), fx["count"]), (name, "awFmParallelSearchLocate counts")
    off = fx["hit_offsets"]
    for i in range(len(queries)):
        assert np.array_equal(lst.positions(i), fx["positions"][int(off[i]):int(off[i + 1])]), (name, "awFmParallelSearchLocate", i)
    lst.dealloc()
    ix.dealloc()


@pytest.mark.parametrize("keep_sa", [True, False], ids=["sa-in-memory", "sa-on-disk"])
@pytest.mark.parametrize("name", NAMES)
def test_bytes_behind_the_last_sample_do_not_reach_a_position(awfm, require_gpu, wide, tmp_path, name, keep_sa):
    """the reference leaves leftovers of its full suffix array in the 8 padding bytes behind the samples; the format gives them
    no meaning, so 0xFF there is as legal.  The kernels read the last sample with a load wider than the sample."""
    fx = load(name)
    bwt_length = int(fx["config"][3])
    path = str(tmp_path / (name + "_ff.awfmi"))
    with open(path, "wb") as f:
        f.write(rc.with_padding(fx["awfmi"].tobytes(), 0xFF))
    ix = awfm.read_index_from_file(path, keep_sa_in_memory=keep_sa)
    g = awfm.GpuIndex(ix)
    assert np.array_equal(device_locate_all(g, bwt_length), fx["all_positions"])
    _, hit_off, pos = g.locate_host(fx["chars"], fx["offsets"])
    assert np.array_equal(hit_off, fx["hit_offsets"]) and np.array_equal(pos, fx["positions"])
    g.set_dense_sa(True)  # expands the same packed samples, the last one included
    assert g.has_dense_sa
    assert np.array_equal(device_locate_all(g, bwt_length), fx["all_positions"]), "dense suffix array"
    g.destroy()
    ix.dealloc()


@pytest.mark.parametrize("name", NAMES)
def test_gpu_built_index_equals_the_reference_built_one(awfm, oracle, require_gpu, wide, name):
    fx = load(name)
    alphabet, ratio, seed_k, bwt_length, width = (int(v) for v in fx["config"])
    ix = awfm.gpu_create_index(fx["text"], alphabet, ratio, seed_k)
    assert ix.bwt_length == bwt_length and ix.sa_width == width
    digests = [oracle.fnv1a(np.ascontiguousarray(a)) for a in (ix.blocks(), ix.prefix_sums(), ix.seed_table())]
    assert digests == [int(d) for d in fx["digests"]]
    assert np.array_equal(rc.sa_samples(ix.packed_sa(), bwt_length, ratio), fx["samples"])
    ix.dealloc()
