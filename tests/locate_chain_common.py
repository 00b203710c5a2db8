"""A host model of the stage from ranges to positions (include/awfm_gpu.h: awfmGpuHitOffsets*, awfmGpuLocate*, awfmGpuSortHits*,
awfmGpuListLocateOnDevice), in plain numpy and Python integers and written from the words of that header, not from the kernels:

  the length of a range {sp, ep} is ep - sp + 1 where sp <= ep and 0 otherwise (the reference's awFmSearchRangeLength; {1, 0},
  {sp, sp - 1} and {0, 2^64 - 1}, whose length wraps to 0, are empty);
  the hit offsets are the exclusive prefix sums of the lengths, the total at [n];
  hit h of the flat hit list belongs to the k-mer i with off_i <= h < off_(i+1) and is SA[sp_i + (h - off_i)];
  a window writes positions[h - hitBegin] for hitBegin <= h < hitEnd over the k-mers [queryBegin, queryEnd) and nothing else;
  the tail of a list is its first min(count, cap) entries in k-mer order, {0xFFFFFFFF, {1, 0}} behind them, every offset from
  the list's length on the total, and the first capacityHits positions.

Beside the model: the thresholds of the kernels behind those calls as named values (tests/test_locate_chain.py reads them out of
the sources again and fails when they differ), functions that say which branch a case takes at those thresholds, and the case
lists, generated from the thresholds so that each appears as t - 1, t and t + 1.  Every case names the branches it is there
for; check_coverage() derives the branches again and asserts that each named branch is reached."""
import numpy as np

# ---------------------------------------------------------------- the thresholds (csrc/awfm_gpu_locate.hip, awfm_gpu_ordered.hip)
SCAN_THREADS, SCAN_ITEMS = 256, 4  # kScanThreads, kScanItems
SCAN_TILE = SCAN_THREADS * SCAN_ITEMS
SCAN_SMALL_THREADS, SCAN_SMALL_ITEMS = 1024, 16  # kScanSmallThreads, kScanSmallItems
SCAN_SMALL = SCAN_SMALL_THREADS * SCAN_SMALL_ITEMS
LANE_MAX = 32  # a list of up to 32 hits is its lane's, a longer one its wave's (expandHitsKernel, listTailKernel)
WAVE = 64
LONG_CHUNK, LONG_STAGE = 16384, 64  # kLongChunk, kLongStage
LONG_RULE = 64  # window hits >= 64 * window k-mers: expandLongKernel (awfmGpuLocateWindow)
LONG_THREADS = 256
LONG_UNROLL = 3 * LONG_THREADS  # the loop `h + 768 < hi` of expandLongKernel: four gathers of a thread at once
LIST_TAIL_THREADS, LIST_TAIL_SLOTS = 1024, 2048  # kListTailThreads, kListTailSlots
LIST_TAIL_MAX_ENTRIES = 1 << 18  # kListTailMaxEntries: a longer list takes copy + sort + scan + locate
LIST_TAIL_ALL_RANGES = 16384  # `allRanges`: up to this capacity every range is requested beside its key
LIST_TAIL_PER_TRIP = LIST_TAIL_THREADS * 8 * 2  # entries of one trip of the pass over the list (kPer * kGroups a thread)
LIST_TAIL_GRID_DIVISOR = 16  # capacity / 16 workgroups
HUGE, HUGE_SLOTS = 4096, 64  # kHuge, kHugeSlots
RANK_BLOCK_WORDS = 64  # kRankBlockWords
RANK_BLOCK = 64 * RANK_BLOCK_WORDS  # k-mers of one counted block of the bitmap
RANK_SCAN_THREADS = 1024  # blocks of one trip of rankBlockScanKernel
MI355X_CUS = 256

NO_KMER = 0xFFFFFFFF
PATTERN64 = 0xA5A5A5A5A5A5A5A5  # what every output word holds before a call
MASK64 = (1 << 64) - 1

TEXT_LETTERS = 1 << 17
TEXT_ROWS = TEXT_LETTERS + 1  # the suffix array's rows: the text and its sentinel


def text():
    """the tests' text: random a, c, g, t with a few n, 2^17 letters"""
    rng = np.random.default_rng(20241)
    t = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, TEXT_LETTERS)].copy()
    t[[0, 777, 65535, 65536, TEXT_LETTERS - 1]] = ord("n")
    return t


# ---------------------------------------------------------------- the model
def lengths(ranges):
    """uint64[n, 2] -> uint64[n]"""
    r = np.asarray(ranges, np.uint64).reshape(-1, 2)
    with np.errstate(over="ignore"):
        return np.where(r[:, 0] <= r[:, 1], r[:, 1] - r[:, 0] + np.uint64(1), np.uint64(0)).astype(np.uint64)


def exact_total(lens):
    """the sum of uint64 lengths as a Python integer (the halves are summed apart: no wrap below 2^32 elements)"""
    lens = np.asarray(lens, np.uint64)
    return (int((lens >> np.uint64(32)).sum(dtype=np.uint64)) << 32) + int((lens & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64))


def offsets(lens):
    """exclusive prefix sums uint64[n + 1], the total at [n]; exact: the total is below 2^63"""
    lens = np.asarray(lens, np.uint64)
    total = exact_total(lens)
    assert total < (1 << 63), "the model keeps totals below 2^63"
    off = np.zeros(lens.size + 1, np.uint64)
    np.cumsum(lens, out=off[1:])
    assert int(off[-1]) == total
    return off


def window(sa, ranges, off, query_begin, query_end, hit_begin, hit_end, fill=PATTERN64):
    """what a locate of the window leaves in positions[0 .. hit_end - hit_begin): untouched words hold `fill`"""
    out = np.full(max(hit_end - hit_begin, 0), fill, np.uint64)
    if query_end <= query_begin or hit_end <= hit_begin:
        return out
    r = np.asarray(ranges, np.uint64).reshape(-1, 2)
    first = max(query_begin, int(np.searchsorted(off, hit_begin, side="right")) - 1)
    for i in range(first, query_end):
        begin, end = int(off[i]), int(off[i + 1])
        if begin >= hit_end:
            break
        lo, hi = max(begin, hit_begin), min(end, hit_end)
        if lo < hi:
            sp = int(r[i, 0])
            out[lo - hit_begin:hi - hit_begin] = sa[sp + lo - begin:sp + hi - begin]
    return out


def covered(off, query_begin, query_end, hit_begin, hit_end):
    """every hit of the window belongs to a k-mer of [query_begin, query_end): the window then comes out without a gap (a
    locate without the full suffix array walks every word of the window, so its callers pass such windows only)"""
    return query_begin < query_end and int(off[query_begin]) <= hit_begin < hit_end <= int(off[query_end])


def empty_range(form, sp=7):
    return {0: (1, 0), 1: (sp, sp - 1), 2: (0, MASK64)}[form % 3]


def make_ranges(lens, seed, rows=TEXT_ROWS):
    """hand-made ranges of these lengths on an index of `rows` rows; the empty ones in every empty form in turn"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.uint64)
    assert int(lens.max(initial=0)) <= rows
    sp = (rng.random(lens.size) * (rows - lens.astype(np.float64) + 1)).astype(np.uint64)
    sp = np.minimum(sp, np.uint64(rows) - lens)
    r = np.stack((sp, sp + lens - np.uint64(1)), axis=1)
    empties = np.flatnonzero(lens == 0)
    for k, i in enumerate(empties[:3000]):
        r[i] = empty_range(k, sp=int(sp[i]) + 1)
    r[empties[3000:]] = (1, 0)
    assert np.array_equal(lengths(r), lens)
    return np.ascontiguousarray(r)


def sort_on_device(kmers, ranges, count, cap):
    """awfmGpuSortHitsOnDevice: the first min(count, cap) entries in k-mer order, the others as they were"""
    n = min(count, cap)
    k, r = np.array(kmers, np.uint32), np.array(ranges, np.uint64).reshape(-1, 2)
    order = np.argsort(k[:n], kind="stable")
    k[:n], r[:n] = k[:n][order], r[:n][order]
    return k, r


def sort_on_host(kmers, ranges, num_entries):
    """awfmGpuSortHits: the first num_entries entries in k-mer order ({0xFFFFFFFF, empty} sorts last)"""
    return sort_on_device(kmers, ranges, num_entries, num_entries)


def list_tail(sa, kmers, ranges, count, cap, capacity_hits, fill=PATTERN64):
    """awfmGpuListLocateOnDevice -> (sorted k-mers uint32[cap], sorted ranges uint64[cap, 2], offsets uint64[cap + 1],
    positions uint64[capacity_hits])"""
    n = min(count, cap)
    k = np.full(cap, NO_KMER, np.uint32)
    r = np.tile(np.array([1, 0], np.uint64), (cap, 1))
    order = np.argsort(np.asarray(kmers, np.uint32)[:n], kind="stable")
    k[:n] = np.asarray(kmers, np.uint32)[:n][order]
    r[:n] = np.asarray(ranges, np.uint64).reshape(-1, 2)[:n][order]
    off = offsets(lengths(r))
    assert np.all(off[n:] == off[n])
    return k, r, off, window(sa, r, off, 0, n, 0, capacity_hits, fill) if capacity_hits else np.zeros(0, np.uint64)


# ---------------------------------------------------------------- which branch a case takes
def entry_branch(hits_here, huge_slot_free=True):
    """who expands the `hits_here` hits an entry has inside the window or below capacityHits"""
    if hits_here == 0:
        return "none"
    if hits_here <= LANE_MAX:
        return "lane"
    if hits_here <= HUGE or not huge_slot_free:
        return "wave"
    return "workgroup"  # (listTailKernel only: expandHitsKernel has lane and wave)


def scan_path(n):
    """the launches of the scan of n elements"""
    tiles = -(-n // SCAN_TILE)
    if tiles > 1 and n <= SCAN_SMALL:
        return "small"
    if tiles <= 1:
        return "one-tile"
    inner = scan_path(tiles)
    return {"one-tile": "two-level-tile", "small": "two-level-small"}.get(inner, "three-level")


def expand_kernel(window_hits, window_kmers, dense):
    return "long" if dense and window_hits >= LONG_RULE * window_kmers else "hits"


def sort_path(num_queries):
    blocks = -(-num_queries // RANK_BLOCK)
    return "rank-scan-one-trip" if blocks <= RANK_SCAN_THREADS else "rank-scan-carry"


class ListCase:
    """a hand-made list in the shape awfmGpuSearchHitsCompact leaves: `kmers` / `lens` are the min(count, cap) entries stored, in
    the order they were appended; cut: "all" (capacityHits beyond the total), "zero", "null" (no position buffer), or
    ("inside", branch): capacityHits in the middle of the first entry in k-mer order that `branch` expands"""

    def __init__(self, name, branches, num_queries, cap, count, kmers, lens, cut="all", skew=0):
        self.name, self.branches, self.num_queries, self.cap, self.count = name, tuple(branches), num_queries, cap, count
        self.kmers, self.lens, self.cut, self.skew = np.asarray(kmers, np.uint32), np.asarray(lens, np.uint64), cut, skew
        n = min(count, cap)
        assert self.kmers.size == n == self.lens.size and np.unique(self.kmers).size == n, name
        assert n == 0 or int(self.kmers.max()) < num_queries, name
        assert 1 <= num_queries < NO_KMER and cap >= 1 and int(self.lens.min(initial=1)) >= 1, name

    def __repr__(self):
        return self.name

    def arrays(self, seed=5):
        """(kmers uint32[cap], ranges uint64[cap, 2]) as the search leaves them: {0xFFFFFFFF, {1, 0}} behind the entries"""
        k = np.full(self.cap, NO_KMER, np.uint32)
        r = np.tile(np.array([1, 0], np.uint64), (self.cap, 1))
        k[:self.kmers.size] = self.kmers
        r[:self.kmers.size] = make_ranges(self.lens, seed)
        return k, r

    def sorted_lens(self):
        return self.lens[np.argsort(self.kmers, kind="stable")]

    def capacity_hits(self):
        lens = self.sorted_lens()
        total = exact_total(lens)
        if self.cut == "all":
            return total + 9
        if self.cut in ("zero", "null"):
            return 0
        off = offsets(lens)
        want = self.cut[1]
        for j, length in enumerate(lens.tolist()):
            if length >= 2 and entry_branch(length // 2) == want:
                return int(off[j]) + length // 2
        raise AssertionError((self.name, "no entry for the cut", want))


def list_tail_branches(case, num_cus=MI355X_CUS):
    """the branches of awfmGpuListLocateOnDevice this case takes, derived from the thresholds"""
    out = set()
    n, cap, nq = min(case.count, case.cap), case.cap, case.num_queries
    out.add("count=0" if case.count == 0 else "count=cap" if case.count == cap else "count>cap" if case.count > cap else "count<cap")
    out.add({"all": "cut-none", "zero": "cut-zero", "null": "cut-null"}.get(case.cut) or "cut-" + {"lane": "short", "wave": "long", "workgroup": "huge"}[case.cut[1]])
    if n and int(case.kmers.max()) == nq - 1:
        out.add("last-kmer")
    if cap > LIST_TAIL_MAX_ENTRIES:
        out.add("fall-back")
        return out
    out.add("one-launch")
    grid = max(cap // LIST_TAIL_GRID_DIVISOR, 1)
    name = "grid=1" if cap // LIST_TAIL_GRID_DIVISOR < 1 else "grid=capacity/16"
    if grid > num_cus:
        grid, name = num_cus, "grid=CUs"
    if grid > nq:
        grid, name = nq, "grid=numQueries"
    out.add(name)
    out.add("keys-scalar" if case.skew % 16 else "keys-vector" if cap % 8 == 0 else "keys-vector-and-scalar" if cap > 8 else "keys-scalar")
    out.add("all-ranges" if cap <= LIST_TAIL_ALL_RANGES else "ranges-behind-keys")
    out.add("pass-one-trip" if cap <= LIST_TAIL_PER_TRIP else "pass-more-trips")
    width = -(-nq // grid)
    order = np.argsort(case.kmers, kind="stable")
    keys, lens = case.kmers[order].astype(np.int64), case.lens[order]
    off = offsets(lens)
    capacity_hits = case.capacity_hits()
    here = np.clip(capacity_hits - off[:-1].astype(np.int64), 0, lens.astype(np.int64))
    group = np.minimum(keys // width, grid - 1)

    def trips(idx):
        """the entries idx (positions in k-mer order) of one emit()"""
        out.add("emit-second-trip" if idx.size > LIST_TAIL_THREADS else "emit-full-trip" if idx.size == LIST_TAIL_THREADS else "emit-one-trip")
        for base in range(0, idx.size, LIST_TAIL_THREADS):
            part = here[idx[base:base + LIST_TAIL_THREADS]]
            huge = int((part > HUGE).sum())
            if huge == HUGE_SLOTS:
                out.add("huge-slots-full")
            if huge > HUGE_SLOTS:
                out.add("huge-overflow")
            for h in part.tolist():
                for edge, label in ((LANE_MAX, "lane-32"), (LANE_MAX + 1, "wave-33"), (HUGE, "wave-4096"), (HUGE + 1, "workgroup-4097")):
                    if h == edge:
                        out.add(label)
                if h > 4 * LIST_TAIL_THREADS:
                    out.add("workgroup-unrolled")

    for g in np.unique(group).tolist():
        idx = np.flatnonzero(group == g)
        if idx.size <= LIST_TAIL_SLOTS:
            out.add("slots-full" if idx.size == LIST_TAIL_SLOTS else "slots")
            trips(idx)
        else:
            out.add("sub-ranges")
            sub = (keys[idx] - width * g) // LIST_TAIL_SLOTS
            for s in np.unique(sub).tolist():
                trips(idx[sub == s])
    return out


# ---------------------------------------------------------------- the case lists
def around(*thresholds):
    return sorted({t + d for t in thresholds for d in (-1, 0, 1)})


# scans: (n, branch).  n = 0 is each entry point's own case (accepted with a total of 0, or refused)
SCAN_SIZES = [n for n in {1} | set(around(SCAN_ITEMS, SCAN_THREADS, SCAN_TILE, SCAN_SMALL, SCAN_TILE * SCAN_TILE, SCAN_TILE * SCAN_SMALL)) if n > 0]
SCAN_SIZES.sort()
SCAN_CROSSING_N = 40 * SCAN_TILE + 7  # the two batches whose total crosses 2^32 (ranges of 2^17 hits, repeated)
SCAN_VALUES = ("zeros", "ones", "random")
SCAN_MAX_LENGTH = 1 << 17


def scan_lengths(n, values):
    if values == "zeros":
        return np.zeros(n, np.uint64)
    if values == "ones":
        return np.ones(n, np.uint64)
    if values == "random":  # a third of the ranges empty
        rng = np.random.default_rng(n)
        lens = rng.integers(1, SCAN_MAX_LENGTH + 1, n).astype(np.uint64)
        lens[rng.integers(0, 3, n) == 0] = 0
        return lens
    lens = np.full(n, SCAN_MAX_LENGTH, np.uint64)  # 2^15 of them make 2^32: the offset of element 32 * SCAN_TILE, a tile's first
    if values == "cross-in-tile":
        lens[:SCAN_TILE // 2] = 0  # ... and half a tile later
    else:
        assert values == "cross-between-tiles"
    return lens


def scan_ranges(lens, seed=3):
    """ranges of these lengths without a text behind them: the scans read nothing else"""
    return make_ranges(lens, seed, rows=1 << 40)


def crossing_element(lens):
    """the first element whose offset is 2^32 or more"""
    return int(np.searchsorted(offsets(lens), 1 << 32, side="left"))


SCAN_BRANCHES = ("one-tile", "small", "two-level-tile", "two-level-small", "three-level", "cross-2^32-in-tile", "cross-2^32-between-tiles")

# windows: the lists of the batch every window is cut out of, in a fixed shuffled order
ENTRY_HITS = sorted({0, 1, 4 * LONG_CHUNK} | set(around(LANE_MAX, WAVE, HUGE, LONG_CHUNK)))


def window_batch():
    lens = np.array(ENTRY_HITS + [0, 0, 5], np.uint64)
    return lens[np.random.default_rng(11).permutation(lens.size)]


def window_cases(off):
    """[(name, query_begin, query_end, hit_begin, hit_end)]: every window with all k-mers and with just the k-mers it touches"""
    n, total = off.size - 1, int(off[-1])
    cuts = [("whole", 0, total)]
    for i in range(n):
        first, length = int(off[i]), int(off[i + 1]) - int(off[i])
        if length == 0:
            continue
        cuts.append((f"list {i} ({length}): its first hit", first, first + 1))
        for d in (-1, 0, 1):
            if 0 <= first + d < total:
                cuts.append((f"list {i} ({length}): begins at first{d:+d}", first + d, min(first + d + 100, total)))
            if 0 < first + d <= total:
                cuts.append((f"list {i} ({length}): ends at first{d:+d}", max(first + d - 100, 0), first + d))
        if length >= 3:
            cuts.append((f"list {i} ({length}): inside", first + length // 3, first + 2 * length // 3))
    out = []
    for name, hb, he in cuts:
        qb = int(np.searchsorted(off, hb, side="right")) - 1
        qe = int(np.searchsorted(off, he, side="left"))
        assert covered(off, qb, qe, hb, he) and covered(off, 0, n, hb, he), name
        out.append((name + ", all k-mers", 0, n, hb, he))
        if (qb, qe) != (0, n):
            out.append((name + ", its k-mers", qb, qe, hb, he))
    return out


def long_batch():
    """the batch for expandLongKernel -> (lens, notes): as many k-mers as the rule allows for its hits, so that one k-mer more (an
    empty one) puts the whole window below the rule"""
    lens, notes = [], {}

    def add(name, items):
        notes[name] = (len(lens), sum(lens))  # (first k-mer, first hit)
        lens.extend(items)

    add("five-chunks", [5 * LONG_CHUNK])  # one list over five chunks; the next chunk begins exactly at the next list's start
    add("singles", [1] * 200)  # more than LONG_STAGE k-mers inside one chunk: the stage is refilled mid-chunk
    add("unroll-edges", around(LONG_UNROLL, 4 * LONG_THREADS))  # parts of a chunk of 767 .. 1025 hits
    add("empties-mid-chunk", [0] * 130 + [300])  # stages that hold empty lists only
    add("pad-to-chunk", [LONG_CHUNK - sum(lens) % LONG_CHUNK])
    add("empties-at-chunk-start", [0] * 130 + [LONG_CHUNK + 5])  # ... in front of the k-mer a chunk begins with
    add("tail", [LONG_CHUNK // 2, 3, 70])
    add("filler", [0] * (sum(lens) // LONG_RULE - len(lens)))  # k-mers without hits, until one more tips the rule
    assert LONG_RULE * len(lens) <= sum(lens) < LONG_RULE * (len(lens) + 1)
    return np.array(lens, np.uint64), notes


def long_batch_branches(lens, notes):
    out = set()
    off = offsets(lens)
    total, n = int(off[-1]), lens.size
    out.add("expand-" + expand_kernel(total, n, True))
    out.add("expand-" + expand_kernel(total, n + 1, True) + "-with-one-k-mer-more")
    starts = set(off[:-1][lens > 0].tolist())
    for chunk in range(0, total, LONG_CHUNK):
        first = int(np.searchsorted(off, chunk, side="right")) - 1  # the last k-mer whose list begins at or before the chunk
        last = int(np.searchsorted(off, min(chunk + LONG_CHUNK, total), side="left"))
        if chunk in starts and chunk:
            out.add("chunk-begins-at-a-list")
            if first >= 130 and not lens[first - 130:first].any():
                out.add("empties-in-front-of-a-chunk's-k-mer")
        if last - first > LONG_STAGE:
            out.add("stage-refilled-mid-chunk")
            inside = lens[first:last]
            run = 0
            for v in inside.tolist():
                run = run + 1 if v == 0 else 0
                if run > LONG_STAGE:
                    out.add("stage-of-empties")
        for i in range(first, last):
            part = min(int(off[i + 1]), chunk + LONG_CHUNK) - max(int(off[i]), chunk)
            for edge in around(LONG_UNROLL, 4 * LONG_THREADS):
                if part == edge:
                    out.add(f"part-of-{edge}")
    if int(lens.max()) >= 5 * LONG_CHUNK:
        out.add("list-over-five-chunks")
    return out


LONG_BRANCHES = ("expand-long", "expand-hits-with-one-k-mer-more", "chunk-begins-at-a-list", "empties-in-front-of-a-chunk's-k-mer",
                 "stage-refilled-mid-chunk", "stage-of-empties", "list-over-five-chunks") + tuple(
                     f"part-of-{e}" for e in around(LONG_UNROLL, 4 * LONG_THREADS))

# offsets beyond 2^32
BEYOND_N, BEYOND_LENGTH = 33000, 1 << 17


def beyond_windows(total):
    return [((1 << 32) - 5000, (1 << 32) + 5000), (total - 100, total)]


# list tails
LIST_WIDE_QUERIES = MI355X_CUS * 4 * LIST_TAIL_SLOTS  # 256 workgroups own 8192 k-mer numbers each


def _spread(rng, n, low, high):
    return rng.choice(np.arange(low, high, dtype=np.int64), n, replace=False)


def list_cases():
    rng = np.random.default_rng(77)
    cases = []

    def case(name, branches, nq, cap, count, kmers, lens=None, **more):
        kmers = np.asarray(kmers, np.int64)
        lens = rng.integers(1, 4, kmers.size) if lens is None else np.asarray(lens)
        order = rng.permutation(kmers.size)  # the order the waves came in
        kmers, lens = kmers[order], lens[order]
        cases.append(ListCase(name, branches, nq, cap, count, kmers, lens, **more))

    width = LIST_WIDE_QUERIES // MI355X_CUS
    # capacities
    case("capacity 1", ("grid=1", "keys-scalar", "count=cap", "last-kmer"), 10, 1, 1, [9])
    case("capacity 15", ("grid=1", "keys-vector-and-scalar", "count<cap", "slots", "emit-one-trip", "cut-none", "one-launch"), 1000, 15, 11, _spread(rng, 11, 0, 1000))
    case("capacity 16", ("grid=capacity/16", "keys-vector", "count=cap"), 1000, 16, 16, _spread(rng, 16, 0, 1000))
    case("capacity 17, more hits than it holds", ("count>cap", "keys-vector-and-scalar"), 1000, 17, 40, _spread(rng, 17, 0, 1000))
    for t in around(LIST_TAIL_ALL_RANGES):
        case(f"capacity {t}", ("grid=CUs", "all-ranges" if t <= LIST_TAIL_ALL_RANGES else "ranges-behind-keys",
                                "pass-one-trip" if t <= LIST_TAIL_PER_TRIP else "pass-more-trips"),
             LIST_WIDE_QUERIES, t, 9000, _spread(rng, 9000, 0, LIST_WIDE_QUERIES))
    case(f"capacity {LIST_TAIL_ALL_RANGES + 1}, full", ("count=cap", "pass-more-trips"), LIST_WIDE_QUERIES, LIST_TAIL_ALL_RANGES + 1,
         LIST_TAIL_ALL_RANGES + 1, _spread(rng, LIST_TAIL_ALL_RANGES + 1, 0, LIST_WIDE_QUERIES))
    case("capacity 2^18", ("one-launch", "ranges-behind-keys"), 1 << 22, LIST_TAIL_MAX_ENTRIES, 3000, _spread(rng, 3000, 0, 1 << 22))
    case("capacity 2^18 + 1", ("fall-back", "cut-none"), 1 << 22, LIST_TAIL_MAX_ENTRIES + 1, 3000, _spread(rng, 3000, 0, 1 << 22))
    case("capacity 2^18 + 1, more hits than it holds", ("fall-back", "count>cap"), 1 << 22, LIST_TAIL_MAX_ENTRIES + 1, LIST_TAIL_MAX_ENTRIES + 50,
         _spread(rng, LIST_TAIL_MAX_ENTRIES + 1, 0, 1 << 22))
    case("capacity 2^18 + 1, offsets only", ("fall-back", "cut-null"), 1 << 22, LIST_TAIL_MAX_ENTRIES + 1, 3000, _spread(rng, 3000, 0, 1 << 22), cut="null")
    case("capacity 2^18 + 1, a position buffer too small", ("fall-back", "cut-long"), 1 << 22, LIST_TAIL_MAX_ENTRIES + 1, 3000,
         _spread(rng, 3000, 0, 1 << 22), lens=rng.integers(60, 90, 3000), cut=("inside", "wave"))
    case("fewer k-mers than capacity / 16", ("grid=numQueries", "last-kmer"), 5, 1024, 3, [4, 0, 2])
    case("no hits", ("count=0",), 1000, 100, 0, [])
    for skew in (4, 8, 12):
        case(f"the list {skew} bytes off a 16-byte boundary", ("keys-scalar",), 5000, 200, 150, _spread(rng, 150, 0, 5000), skew=skew)
    # entries of one workgroup's range
    for t in (LIST_TAIL_SLOTS, LIST_TAIL_SLOTS + 1):
        case(f"{t} consecutive k-mers in one workgroup's range", ("slots-full" if t == LIST_TAIL_SLOTS else "sub-ranges", "emit-second-trip"),
             LIST_WIDE_QUERIES, LIST_TAIL_ALL_RANGES, t + 40, np.concatenate((3 * width + 100 + np.arange(t), _spread(rng, 40, 4 * width, LIST_WIDE_QUERIES))))
    case("5000 consecutive k-mers across two ranges", ("sub-ranges",), LIST_WIDE_QUERIES, LIST_TAIL_ALL_RANGES, 5000, 4 * width - 2500 + np.arange(5000))
    case("the batch's last 3000 k-mers", ("sub-ranges", "last-kmer"), LIST_WIDE_QUERIES, LIST_TAIL_ALL_RANGES, 3000, LIST_WIDE_QUERIES - 3000 + np.arange(3000))
    for t in (LIST_TAIL_THREADS, LIST_TAIL_THREADS + 1):
        case(f"{t} entries in a range", ("emit-full-trip" if t == LIST_TAIL_THREADS else "emit-second-trip", "slots"),
             LIST_WIDE_QUERIES, LIST_TAIL_ALL_RANGES, t, _spread(rng, t, 7 * width, 8 * width))
    # entries by their number of hits
    sizes = around(LANE_MAX, HUGE) + [70000]
    case("entries of 31 .. 70 000 hits", ("lane-32", "wave-33", "wave-4096", "workgroup-4097", "workgroup-unrolled"), 100000, 64, len(sizes),
         _spread(rng, len(sizes), 0, 100000), lens=sizes)
    for t in (HUGE_SLOTS, HUGE_SLOTS + 1):
        case(f"{t} neighbours above {HUGE} hits", ("huge-slots-full" if t == HUGE_SLOTS else "huge-overflow",), 100000, 256, t + 20,
             np.concatenate((50000 + np.arange(t), _spread(rng, 20, 0, 40000))), lens=[HUGE + 1 + 3 * i for i in range(t)] + [2] * 20)
    # the position buffer
    mixed = [3, 20, 700, 9, 12000, 31, 5000, 2]
    case("no room for positions", ("cut-zero",), 5000, 64, len(mixed), _spread(rng, len(mixed), 0, 5000), lens=mixed, cut="zero")
    case("no position buffer", ("cut-null",), 5000, 64, len(mixed), _spread(rng, len(mixed), 0, 5000), lens=mixed, cut="null")
    for who, label in (("lane", "short"), ("wave", "long"), ("workgroup", "huge")):
        case(f"the position buffer ends inside a {label} entry", (f"cut-{label}",), 5000, 64, len(mixed), _spread(rng, len(mixed), 0, 5000),
             lens=mixed, cut=("inside", who))
    return cases


LIST_BRANCHES = ("one-launch", "fall-back", "grid=1", "grid=capacity/16", "grid=CUs", "grid=numQueries", "keys-vector", "keys-scalar",
                 "keys-vector-and-scalar", "all-ranges", "ranges-behind-keys", "pass-one-trip", "pass-more-trips", "slots", "slots-full",
                 "sub-ranges", "emit-one-trip", "emit-full-trip", "emit-second-trip", "lane-32", "wave-33", "wave-4096", "workgroup-4097",
                 "workgroup-unrolled", "huge-slots-full", "huge-overflow", "cut-none", "cut-zero", "cut-null", "cut-short", "cut-long",
                 "cut-huge", "count=0", "count<cap", "count=cap", "count>cap", "last-kmer")

# sorts: (numQueries, branch)
SORT_QUERIES = [RANK_BLOCK, RANK_BLOCK + 1, RANK_BLOCK * RANK_SCAN_THREADS, RANK_BLOCK * RANK_SCAN_THREADS + 1, 2 * RANK_BLOCK * RANK_SCAN_THREADS + 1]
SORT_BRANCHES = ("rank-scan-one-trip", "rank-scan-carry", "one-block", "second-block", "third-trip")


def sort_branches(num_queries):
    blocks = -(-num_queries // RANK_BLOCK)
    out = {sort_path(num_queries)}
    out.add("one-block" if blocks == 1 else "second-block" if blocks == 2 else "more-blocks")
    if blocks > 2 * RANK_SCAN_THREADS:
        out.add("third-trip")
    return out


def sort_entries(num_queries, seed=1):
    """a few thousand distinct k-mer numbers: the first and last of every block edge (of up to 3000 blocks), the batch's last, random"""
    rng = np.random.default_rng(seed + num_queries)
    edges = np.arange(0, num_queries, RANK_BLOCK, dtype=np.int64)
    if edges.size > 1500:
        edges = np.concatenate((edges[:20], edges[RANK_SCAN_THREADS - 10:RANK_SCAN_THREADS + 10], edges[rng.choice(edges.size, 700, replace=False)], edges[-20:]))
    k = np.concatenate((edges, edges[edges > 0] - 1, [num_queries - 1], rng.integers(0, num_queries, 3000)))
    k = np.unique(k[(k >= 0) & (k < num_queries)])
    return k[rng.permutation(k.size)].astype(np.uint32)


def check_coverage(num_cus=MI355X_CUS):
    """every branch a case names is the branch the thresholds give it, and every branch listed is reached"""
    reached = {scan_path(n) for n in SCAN_SIZES} | {scan_path(SCAN_CROSSING_N)}
    for t in (SCAN_TILE, SCAN_SMALL, SCAN_TILE * SCAN_TILE, SCAN_TILE * SCAN_SMALL):
        assert scan_path(t) != scan_path(t + 1) and {t - 1, t, t + 1} <= set(SCAN_SIZES), ("scan", t)
    for values in ("cross-in-tile", "cross-between-tiles"):
        at = crossing_element(scan_lengths(SCAN_CROSSING_N, values))
        assert 0 < at < SCAN_CROSSING_N and (at % SCAN_TILE == 0) == (values == "cross-between-tiles"), (values, at)
        reached.add("cross-2^32-" + values[6:])
    assert set(SCAN_BRANCHES) <= reached, sorted(set(SCAN_BRANCHES) - reached)
    for t in (LANE_MAX, WAVE, HUGE, LONG_CHUNK):
        assert {t - 1, t, t + 1} <= set(ENTRY_HITS), ("entry", t)
    assert {entry_branch(LANE_MAX), entry_branch(LANE_MAX + 1), entry_branch(HUGE), entry_branch(HUGE + 1)} == {"lane", "wave", "workgroup"}
    lens, notes = long_batch()
    got = long_batch_branches(lens, notes)
    assert set(LONG_BRANCHES) <= got, sorted(set(LONG_BRANCHES) - got)
    reached = set()
    for c in list_cases():
        got = list_tail_branches(c, num_cus)
        assert set(c.branches) <= got, (c.name, "names", sorted(set(c.branches) - got), "takes", sorted(got))
        reached |= set(c.branches)
    assert set(LIST_BRANCHES) <= reached, sorted(set(LIST_BRANCHES) - reached)
    reached = set()
    for nq in SORT_QUERIES:
        reached |= sort_branches(nq)
    assert set(SORT_BRANCHES) <= reached, sorted(set(SORT_BRANCHES) - reached)
    total = BEYOND_N * BEYOND_LENGTH
    assert total > (1 << 32) and all(0 <= a < b <= total for a, b in beyond_windows(total))


check_coverage()
