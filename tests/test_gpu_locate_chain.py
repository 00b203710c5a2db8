"""The stage from ranges to positions on hand-made ranges at its kernels' thresholds (csrc/awfm_gpu_locate.hip and the end of
csrc/awfm_gpu_ordered.hip): awfmGpuHitOffsets / FromCounts / OnDevice, awfmGpuLocate / Window / OnDevice, awfmGpuListLocateOnDevice,
awfmGpuSortHitsOnDevice / awfmGpuSortHits against tests/locate_chain_common.py, the plain model of those calls, whose case lists
are generated from the thresholds and name the branch each case is there for.  Every result is compared for equality.

The ranges are rows of the suffix array of a random text of 2^17 letters with a few n (a range need not be a k-mer's: a locate
reads nothing else of it), on images with suffix-array ratios 1, 3 and 8, with 32- and 64-bit positions (`wide`) and with and
without the full suffix array.  Inputs, outputs and the scan's scratch (exactly awfmGpuScanScratchBytes) lie between guard
words; outputs hold a pattern before the call (position buffers: a row of the index, see ROW)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import locate_chain_common as lc  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5
# What a position buffer holds before a call.  Without the full suffix array the LF walk reads every word of the window back as a
# row of the index, so a defect that left a word unwritten must find a row there (and then fails the comparison), not the guard
# pattern, which as a row lies far outside every image
ROW = 1
IMAGES = [pytest.param(ratio, dense, id=f"sa{ratio}-{'full' if dense else 'sampled'}") for ratio in (1, 3, 8) for dense in (True, False)]


def _guarded(torch, array, skew=0):
    """the array's bytes on the device between guard words, `skew` bytes further in -> (buffer, address)"""
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    host = np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), raw, np.full(GUARD, PATTERN, np.uint8)))
    buffer = torch.from_numpy(host).to("cuda")
    assert (buffer.data_ptr() + GUARD) % 16 == 0
    return buffer, buffer.data_ptr() + GUARD + skew


def _untouched(torch, pairs):
    """the inputs and what lies around them are as they were uploaded"""
    for (buffer, address), array in pairs:
        raw = buffer.cpu().numpy()
        begin = address - buffer.data_ptr()
        body = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert (raw[:begin] == PATTERN).all() and (raw[begin + body.size:] == PATTERN).all(), "wrote beside an input"
        assert np.array_equal(raw[begin:begin + body.size], body), "wrote into an input"


class Arena:
    """the outputs of several calls in one device buffer that holds the pattern: every output between guard words"""

    def __init__(self):
        self.items, self.words, self.size, self.buffer = [], [], GUARD, None

    def add(self, nbytes, skew=0, word=None):
        """word: the 64-bit value the output's words hold before the call instead of the pattern"""
        at = self.size + skew
        self.items.append((at, nbytes))
        if word is not None:
            assert at % 8 == 0 and nbytes % 8 == 0
            self.words.append((at, nbytes, word))
        self.size = (at + nbytes + GUARD + 15) // 16 * 16
        return len(self.items) - 1

    def allocate(self, torch):
        self.buffer = torch.full((self.size,), PATTERN, dtype=torch.uint8, device="cuda")
        assert self.buffer.data_ptr() % 16 == 0
        for at, nbytes, word in self.words:
            self.buffer[at:at + nbytes].view(torch.int64).fill_(word)

    def address(self, item):
        return self.buffer.data_ptr() + self.items[item][0]

    def collect(self):
        """the outputs as byte arrays, after checking that nothing was written between them"""
        host = self.buffer.cpu().numpy()
        between = np.ones(self.size, bool)
        for at, nbytes in self.items:
            between[at:at + nbytes] = False
        assert (host[between] == PATTERN).all(), "wrote outside an output"
        return [host[at:at + nbytes] for at, nbytes in self.items]


class Scratch:
    """exactly awfmGpuScanScratchBytes bytes between guard words"""

    def __init__(self, torch, awfm, n):
        self.size = awfm.GpuIndex.scan_scratch_bytes(n)
        self.buffer = torch.full((self.size + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.address = self.buffer.data_ptr() + GUARD
        assert self.address % 16 == 0

    def check(self):
        assert bool((self.buffer[:GUARD] == PATTERN).all()) and bool((self.buffer[GUARD + self.size:] == PATTERN).all()), "wrote outside the scratch"


class World:
    """the text, its suffix array, and one image per parameter set, built when first asked for"""

    def __init__(self, oracle, awfm):
        self.awfm, self.text = awfm, lc.text()
        self.sa = oracle.Index.from_text(self.text.tobytes(), oracle.DNA, 8, 8).full_sa()
        assert self.sa.size == lc.TEXT_ROWS
        self.indexes, self.images = {}, {}

    def image(self, ratio, dense, wide):
        """`wide`: the parameter of the fixture of that name, which is in force while the image is created"""
        if ratio not in self.indexes:
            self.indexes[ratio] = self.awfm.create_index(self.text, self.awfm.AwFmAlphabetDna, ratio, 8)
        key = (ratio, dense, wide)
        if key not in self.images:
            g = self.awfm.GpuIndex(self.indexes[ratio])
            g.set_dense_sa(dense)
            assert g.has_dense_sa == dense
            self.images[key] = g
        return self.images[key]

    def close(self):
        for g in self.images.values():
            g.destroy()
        for ix in self.indexes.values():
            ix.dealloc()


@pytest.fixture(scope="module")
def world(oracle, awfm, require_gpu):
    w = World(oracle, awfm)
    yield w
    w.close()


@pytest.fixture
def image(world, wide, request):
    """image(ratio, dense): the module's image of that kind under this test's `wide`"""
    name = request.node.callspec.params["wide"]
    return lambda ratio, dense: world.image(ratio, dense, name)


def _u64(raw):
    return raw.view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- scans
def _scan_inputs(n, values):
    lens = lc.scan_lengths(n, values)
    if values == "random":
        ranges = lc.scan_ranges(lens)
    else:  # (cheap: these batches are large)
        sp = np.arange(5, 5 + n, dtype=np.uint64)
        ranges = np.stack((sp, sp + lens - np.uint64(1)), axis=1)
        assert np.array_equal(lc.lengths(ranges), lens)
    return lens, np.ascontiguousarray(ranges), lens.astype(np.uint32)


SCANS = [(n, v) for n in lc.SCAN_SIZES for v in lc.SCAN_VALUES] + [(lc.SCAN_CROSSING_N, v) for v in ("cross-in-tile", "cross-between-tiles")]


@pytest.mark.parametrize("n,values", SCANS, ids=[f"{n}-{v}" for n, v in SCANS])
def test_hit_offsets(world, n, values):
    """the four ways into the scans (awfmGpuHitOffsets, FromCounts, OnDevice with counts and with ranges) give the model's
    exclusive prefix sums and total at every size at which the scan takes another path -- one tile, scanSmallKernel, tile sums
    through one tile / through scanSmallKernel / through a level of their own (beyond 2^24) --, each from both sides, and with a
    total that passes 2^32 inside a tile and between two"""
    import torch
    awfm, g = world.awfm, world.image(8, True, "module")
    lens, ranges, counts = _scan_inputs(n, values)
    want = lc.offsets(lens)
    if values.startswith("cross"):
        assert int(want[-1]) > 1 << 32 and lc.scan_path(n) == "two-level-tile"
    d_want = torch.from_numpy(want.view(np.int64)).to("cuda")
    d_ranges, d_counts = _guarded(torch, ranges), _guarded(torch, counts)
    scratch = Scratch(torch, awfm, n)
    calls = {
        "awfmGpuHitOffsets": lambda out: g.hit_offsets(d_ranges[1], n, out, scratch.address),
        "awfmGpuHitOffsetsFromCounts": lambda out: g.hit_offsets_from_counts(d_counts[1], n, out, scratch.address),
        "awfmGpuHitOffsetsOnDevice, counts": lambda out: g.hit_offsets_on_device(d_counts[1], 0, n, out, scratch.address),
        "awfmGpuHitOffsetsOnDevice, ranges": lambda out: g.hit_offsets_on_device(0, d_ranges[1], n, out, scratch.address),
    }
    for name, call in calls.items():
        out = torch.full((8 * (n + 1) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        total = call(out.data_ptr() + GUARD)
        torch.cuda.synchronize()
        assert total is None or total == int(want[-1]), (name, total)
        assert bool((out[:GUARD] == PATTERN).all()) and bool((out[GUARD + 8 * (n + 1):] == PATTERN).all()), (name, "wrote outside the offsets")
        got = out[GUARD:GUARD + 8 * (n + 1)].view(torch.int64)
        if not torch.equal(got, d_want):
            bad = torch.nonzero(got != d_want).flatten()
            raise AssertionError((name, lc.scan_path(n), "first wrong offset", int(bad[0]), "of", int(bad.numel()), int(got[bad[0]]), int(d_want[bad[0]])))
        scratch.check()
        del out
    for raw in (d_ranges[0], d_counts[0]):
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[-GUARD:] == PATTERN).all()), "wrote beside an input"
    assert np.array_equal(d_counts[0].cpu().numpy()[GUARD:-GUARD].view(np.uint32), counts)


def test_hit_offsets_of_an_empty_batch(world):
    """n = 0: the host-counted calls give a total of 0 and offsets[0] = 0; the call that leaves the total on the device refuses"""
    import torch
    awfm, g = world.awfm, world.image(8, True, "module")
    some = _guarded(torch, np.zeros(4, np.uint64))
    scratch = Scratch(torch, awfm, 0)
    arena = Arena()
    items = [arena.add(8) for _ in range(4)]
    arena.allocate(torch)
    assert g.hit_offsets(some[1], 0, arena.address(items[0]), scratch.address) == 0
    assert g.hit_offsets_from_counts(some[1], 0, arena.address(items[1]), scratch.address) == 0
    for counts, ranges, item in ((some[1], 0, items[2]), (0, some[1], items[3])):
        with pytest.raises(awfm.AwFmError):
            g.hit_offsets_on_device(counts, ranges, 0, arena.address(item), scratch.address)
    torch.cuda.synchronize()
    got = arena.collect()
    assert _u64(got[0]).tolist() == [0] and _u64(got[1]).tolist() == [0]
    assert _u64(got[2]).tolist() == [lc.PATTERN64] and _u64(got[3]).tolist() == [lc.PATTERN64]
    scratch.check()


# ---------------------------------------------------------------------------------------------------------------- windows
class Batch:
    """hand-made ranges on the device with their hit offsets, which the scan computes there (and the model confirms)"""

    def __init__(self, torch, world, g, lens, seed, ranges=None):
        self.torch, self.g, self.sa, self.n = torch, g, world.sa, len(lens)
        self.ranges = lc.make_ranges(lens, seed) if ranges is None else ranges
        self.off = lc.offsets(lc.lengths(self.ranges))
        self.total = int(self.off[-1])
        self.d_ranges = _guarded(torch, self.ranges)
        self.scratch = Scratch(torch, world.awfm, self.n)
        self.d_off = _guarded(torch, np.full(self.n + 1, lc.PATTERN64, np.uint64))
        assert g.hit_offsets(self.d_ranges[1], self.n, self.d_off[1], self.scratch.address) == self.total
        self.scratch.check()
        self.arena, self.pending = Arena(), []

    def want(self, qb, qe, hb, he):
        return lc.window(self.sa, self.ranges, self.off, qb, qe, hb, he, fill=ROW)

    def expect(self, name, words, want, call):
        """call(address of `words` output words) is to leave `want` there"""
        self.pending.append((name, self.arena.add(8 * words, word=ROW), want, call))

    def window(self, name, qb, qe, hb, he):
        assert lc.covered(self.off, qb, qe, hb, he), name
        self.expect(f"awfmGpuLocateWindow, {name}", he - hb, self.want(qb, qe, hb, he),
                    lambda out: self.g.locate_window(self.d_ranges[1], self.d_off[1], qb, qe, hb, he, out))

    def capacity(self, name, capacity_hits, room=None):
        """awfmGpuLocateOnDevice: the first capacity_hits hits, the number of hits read on the device"""
        room = max(capacity_hits, 1) if room is None else room
        want = np.full(room, ROW, np.uint64)
        m = min(capacity_hits, self.total)
        want[:m] = self.want(0, self.n, 0, m)
        self.expect(f"awfmGpuLocateOnDevice, {name}", room, want,
                    lambda out: self.g.locate_on_device(self.d_ranges[1], self.d_off[1], self.n, capacity_hits, out))

    def run(self):
        torch = self.torch
        self.arena.allocate(torch)
        for name, item, want, call in self.pending:
            call(self.arena.address(item))
        torch.cuda.synchronize()
        got = self.arena.collect()
        for name, item, want, call in self.pending:
            have = _u64(got[item])
            if not np.array_equal(have, want):
                bad = np.flatnonzero(have != want)
                raise AssertionError((name, "first wrong position", int(bad[0]), "of", bad.size, hex(int(have[bad[0]])), hex(int(want[bad[0]]))))
        raw = self.d_off[0].cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all() and np.array_equal(_u64(raw[GUARD:-GUARD]), self.off), "the hit offsets"
        _untouched(torch, [(self.d_ranges, self.ranges)])


@pytest.mark.parametrize("ratio,dense", IMAGES)
def test_windows_of_lists_at_every_threshold(world, image, ratio, dense):
    """lists of 0, 1, 31 .. 33 (lane or wave), 63 .. 65, 4095 .. 4097, 16383 .. 16385 and 4 * 16384 hits in a shuffled order: the
    whole hit list, windows of one hit, windows that begin or end at, one before and one after a list's first hit, a window
    inside one list -- each over all k-mers and over just its own (queryBegin > 0) --, and awfmGpuLocateOnDevice cut at the same
    places"""
    import torch
    b = Batch(torch, world, image(ratio, dense), lc.window_batch(), seed=21)
    assert set(lc.lengths(b.ranges).tolist()) == set(lc.ENTRY_HITS) | {5}
    b.expect("awfmGpuLocate, whole", b.total, b.want(0, b.n, 0, b.total), lambda out: b.g.locate(b.d_ranges[1], b.d_off[1], b.n, b.total, out))
    cuts = {b.total, b.total + 50}
    for name, qb, qe, hb, he in lc.window_cases(b.off):
        b.window(name, qb, qe, hb, he)
        cuts.add(he)
    for he in sorted(cuts):
        b.capacity(f"capacity {he}", he)
    b.run()


LONG_BEGIN = 5000  # a window that begins here lies inside the list over five chunks


@pytest.mark.parametrize("ratio,dense", IMAGES)
def test_windows_of_long_lists(world, image, ratio, dense):
    """a window with LONG_RULE hits a k-mer and more goes to expandLongKernel where the image has the full suffix array: a list
    over five chunks of 16384 hits, a chunk that begins exactly at a list's start, 200 single-hit k-mers inside one chunk (the
    stage of 64 is refilled), 130 empty lists mid-chunk and in front of the k-mer a chunk begins with, parts of a chunk of
    767 .. 769 and 1023 .. 1025 hits (the unrolled loop).  The same batch with one k-mer more falls below the rule and goes to
    expandHitsKernel; a window cut out of the middle; all equal to the model"""
    import torch
    lens, notes = lc.long_batch()
    n, total = lens.size, lc.exact_total(lens)
    assert lc.expand_kernel(total, n, dense) == ("long" if dense else "hits") and lc.expand_kernel(total, n + 1, dense) == "hits"
    more = np.concatenate((lens, np.zeros(1, np.uint64)))
    b = Batch(torch, world, image(ratio, dense), more, seed=22)
    assert b.total == total and b.n == n + 1
    for name, queries in (("the rule's side", n), ("one k-mer more", n + 1)):
        b.expect(f"awfmGpuLocate, {name}", total, b.want(0, queries, 0, total),
                 lambda out, queries=queries: b.g.locate(b.d_ranges[1], b.d_off[1], queries, total, out))
    # from inside the single-hit k-mers to the end, over the k-mers in front of the filler: chunks that begin nowhere special
    qb, hb = notes["singles"][0] + 7, notes["singles"][1] + 7
    qe = notes["filler"][0]
    assert lc.expand_kernel(total - hb, qe - qb, dense) == ("long" if dense else "hits")
    b.window("from inside the single-hit k-mers on", qb, qe, hb, total)
    b.window("the same over all k-mers", 0, n + 1, hb, total)
    b.window("three chunks and a bit of the long list", 0, 1, LONG_BEGIN, LONG_BEGIN + 3 * lc.LONG_CHUNK + 777)
    b.capacity("half the hits", total // 2)
    b.run()


@pytest.mark.parametrize("ratio,dense", IMAGES)
def test_windows_beyond_2_32_hits(world, image, ratio, dense):
    """33 000 ranges of 2^17 hits: the offsets pass 2^32 (only they are computed); the windows [2^32 - 5000, 2^32 + 5000) and
    [total - 100, total), over all k-mers (expandHitsKernel) and over their own (expandLongKernel with the full suffix array)"""
    import torch
    lens = np.full(lc.BEYOND_N, lc.BEYOND_LENGTH, np.uint64)
    b = Batch(torch, world, image(ratio, dense), lens, seed=23)
    assert b.total == lc.BEYOND_N * lc.BEYOND_LENGTH > 1 << 32
    for hb, he in lc.beyond_windows(b.total):
        qb = int(np.searchsorted(b.off, hb, side="right")) - 1
        qe = int(np.searchsorted(b.off, he, side="left"))
        assert lc.expand_kernel(he - hb, b.n, dense) == "hits" and lc.expand_kernel(he - hb, qe - qb, dense) == ("long" if dense else "hits")
        b.window(f"[{hb}, {he}) over all k-mers", 0, b.n, hb, he)
        b.window(f"[{hb}, {he}) over its k-mers", qb, qe, hb, he)
    b.run()


@pytest.mark.parametrize("ratio", [1, 3, 8])
def test_walk_of_short_and_long_hit_lists(world, image, ratio):
    """without the full suffix array the positions come from the LF walk, whose launch has a rule for short hit lists: batches
    of 4 instead of 16 hits a lane group while th <= grid * (512 / 4) * 4, grid = min(ceil(th / 128), CUs * blocks per CU) with
    at most 8 blocks per CU (AWFM_LOCP in awfmGpuLaunchLocate, gridFor in awfm_device.h).  So a total of 1000 hits is on the
    short side on every device (8 blocks of the grid's at least `CUs`) and CUs * 8 * 512 + 4097 is on the long side whatever
    the occupancy; both give the model's positions, as does a capacity below the total that is still on the device"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    short, long_ = 1000, cus * 8 * 512 + 4097
    assert -(-short // 128) < cus and long_ > cus * 8 * 128 * 4
    g = image(ratio, False)
    rng = np.random.default_rng(31)
    for total in (short, long_):
        lens = rng.integers(0, max(total // 60, 3), 400).astype(np.uint64)
        lens = lens[np.cumsum(lens) < total]
        lens = np.concatenate((lens, [total - lc.exact_total(lens)])).astype(np.uint64)
        assert int(lens.max()) <= lc.TEXT_ROWS
        b = Batch(torch, world, g, lens, seed=total)
        assert b.total == total
        b.expect(f"awfmGpuLocate, {total} hits", total, b.want(0, b.n, 0, total), lambda out, b=b: b.g.locate(b.d_ranges[1], b.d_off[1], b.n, b.total, out))
        b.capacity("a capacity below the total", total - total // 3)
        b.capacity("a capacity above the total", total + 77)
        b.run()


# ---------------------------------------------------------------------------------------------------------------- list tail
LIST_CASES = lc.list_cases()
_list_models = {}


def _list_model(world, case):
    """the case's arrays and what the call is to leave, computed once"""
    if case.name not in _list_models:
        kmers, ranges = case.arrays()
        capacity_hits = case.capacity_hits()
        _list_models[case.name] = (kmers, ranges, capacity_hits, lc.list_tail(world.sa, kmers, ranges, case.count, case.cap, capacity_hits, fill=ROW))
    return _list_models[case.name]


class ListCall:
    """one awfmGpuListLocateOnDevice on a case's arrays: guarded inputs, outputs that hold the pattern"""

    def __init__(self, torch, world, case):
        self.torch, self.case = torch, case
        self.kmers, self.ranges, self.capacity_hits, self.want = _list_model(world, case)
        self.d_kmers = _guarded(torch, self.kmers, skew=case.skew)
        self.d_ranges = _guarded(torch, self.ranges)
        self.d_count = _guarded(torch, np.array([case.count], np.uint32))
        self.arena = Arena()
        cap = case.cap
        self.items = [self.arena.add(4 * cap), self.arena.add(16 * cap), self.arena.add(8 * (cap + 1)), self.arena.add(8 * max(self.capacity_hits, 1), word=ROW)]
        self.arena.allocate(torch)

    def enqueue(self, g, stream=0):
        a, c = self.arena, self.case
        g.list_locate_on_device(self.d_kmers[1], self.d_ranges[1], c.cap, self.d_count[1], c.num_queries, a.address(self.items[0]), a.address(self.items[1]),
                                a.address(self.items[2]), self.capacity_hits, 0 if c.cut == "null" else a.address(self.items[3]), stream=stream)

    def check(self, what=""):
        kmers, ranges, off, pos = self.arena.collect()
        want_kmers, want_ranges, want_off, want_pos = self.want
        name = (self.case.name, what)
        assert np.array_equal(kmers.view(np.uint32), want_kmers), (name, "the sorted k-mers")
        assert np.array_equal(_u64(ranges).reshape(-1, 2), want_ranges), (name, "the sorted ranges")
        assert np.array_equal(_u64(off), want_off), (name, "the hit offsets", np.flatnonzero(_u64(off) != want_off)[:5])
        have = _u64(pos)
        want = want_pos if self.capacity_hits else np.full(1, ROW, np.uint64)
        if not np.array_equal(have, want):
            bad = np.flatnonzero(have != want)
            raise AssertionError((name, "first wrong position", int(bad[0]), "of", bad.size, hex(int(have[bad[0]])), hex(int(want[bad[0]]))))
        _untouched(self.torch, [(self.d_kmers, self.kmers), (self.d_ranges, self.ranges), (self.d_count, np.array([self.case.count], np.uint32))])


@pytest.mark.parametrize("dense", [True, False], ids=["full", "sampled"])
@pytest.mark.parametrize("case", LIST_CASES, ids=[c.name.replace(" ", "-") for c in LIST_CASES])
def test_list_tail(world, image, case, dense):
    """awfmGpuListLocateOnDevice on hand-made lists in the shape awfmGpuSearchHitsCompact leaves (distinct k-mer numbers below
    numQueries in the order the waves came, the length word, {0xFFFFFFFF, empty} behind the entries): the list in k-mer order,
    {0xFFFFFFFF, {1, 0}} behind it, the hit offsets with the total from the list's length on, the positions cut at capacityHits,
    and the appended list untouched -- at the capacities, range fillings, entry sizes and cuts at which listTailKernel chooses,
    and beyond 2^18 entries, where the call falls back to copy, bitmap sort, scan and locate.  The branches a case is there for
    are the ones the thresholds give it on this device"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    took = lc.list_tail_branches(case, cus)
    assert set(case.branches) <= took, (case.name, "is there for", case.branches, "and takes", sorted(took))
    for ratio in (1, 3, 8):
        call = ListCall(torch, world, case)
        call.enqueue(image(ratio, dense))
        torch.cuda.synchronize()
        call.check(f"ratio {ratio}")


@pytest.mark.parametrize("dense", [True, False], ids=["full", "sampled"])
def test_list_tails_from_two_streams(world, image, dense):
    """two streams on one image at once, nothing waited for in between: the one-launch tail, and the fall-back, whose bitmap
    sort shares the image's temporaries behind their gate and whose scan allocates in stream order"""
    import torch
    g = image(3, dense)
    by_name = {c.name: c for c in LIST_CASES}
    pairs = [(by_name["5000 consecutive k-mers across two ranges"], by_name[f"{lc.HUGE_SLOTS + 1} neighbours above {lc.HUGE} hits"]),
             (by_name["capacity 2^18 + 1"], by_name["capacity 2^18 + 1, a position buffer too small"])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for pair in pairs:
        calls = [[ListCall(torch, world, c) for _ in range(3)] for c in pair]
        torch.cuda.synchronize()
        for k in range(3):
            for mine, s in zip(calls, streams):
                mine[k].enqueue(g, stream=s.cuda_stream)
        torch.cuda.synchronize()
        for mine in calls:
            for k, call in enumerate(mine):
                call.check(f"call {k} of its stream")
    for s in streams:
        g.stream_retire(s.cuda_stream)


# ---------------------------------------------------------------------------------------------------------------- sorts
@pytest.mark.parametrize("num_queries", lc.SORT_QUERIES)
def test_sorts_of_a_list(world, num_queries):
    """awfmGpuSortHitsOnDevice (a bitmap of the batch, a count per 4096 k-mers, their scan by one workgroup in trips of 1024
    blocks with a carry, a rank per entry) and awfmGpuSortHits (a radix sort) on a few thousand entries that hold the first and
    last k-mer of every block edge and the batch's last: one block, two, 1024 (one trip of the scan), 1025 (the carry) and 2049
    (two carries); a length word above the capacity"""
    import torch
    g = world.image(8, True, "module")
    took = lc.sort_branches(num_queries)
    kmers = lc.sort_entries(num_queries)
    assert kmers.size >= 2000 and int(kmers.max()) == num_queries - 1 and 0 in kmers
    if num_queries > lc.RANK_BLOCK * lc.RANK_SCAN_THREADS:
        assert "rank-scan-carry" in took and {lc.RANK_BLOCK * lc.RANK_SCAN_THREADS - 1, lc.RANK_BLOCK * lc.RANK_SCAN_THREADS} <= set(kmers.tolist())
    ranges = lc.make_ranges(np.random.default_rng(3).integers(1, 9, kmers.size), seed=num_queries)
    for count, cap in ((kmers.size, kmers.size + 100), (kmers.size + 500, kmers.size)):
        n = min(count, cap)
        k = np.full(cap, lc.NO_KMER, np.uint32)
        r = np.tile(np.array([1, 0], np.uint64), (cap, 1))
        k[:n], r[:n] = kmers[:n], ranges[:n]
        want_k, want_r = lc.sort_on_device(k, r, count, cap)
        assert np.array_equal(want_k[:n], np.sort(kmers[:n])) and (want_k[n:] == lc.NO_KMER).all()
        d_count = _guarded(torch, np.array([count], np.uint32))
        on_device = (_guarded(torch, k), _guarded(torch, r))
        on_host = (_guarded(torch, k), _guarded(torch, r))
        g.sort_hits_on_device(on_device[0][1], on_device[1][1], cap, d_count[1], num_queries)
        g.sort_hits(on_host[0][1], on_host[1][1], cap)
        torch.cuda.synchronize()
        host_k, host_r = lc.sort_on_host(k, r, cap)
        assert np.array_equal(host_k, want_k) and np.array_equal(host_r, want_r)  # (the entries behind the list sort last)
        _untouched(torch, [(on_device[0], want_k), (on_device[1], want_r), (on_host[0], want_k), (on_host[1], want_r), (d_count, np.array([count], np.uint32))])
