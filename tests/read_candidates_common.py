"""Shared by the tests of awfmReadCandidates / awfmGpuReadCandidates (include/awfm_gpu.h, "candidate loci"): a NumPy
restatement of the definition (lexsort and diff: no code shared with the C), the instances -- the edge list, random batches,
batches of given sizes -- and the end-to-end pipeline from a FASTA file to candidates on the host."""
import ctypes as C

import numpy as np

NONE = 0xFFFFFFFF
MAX_HITS = 4096
MALFORMED, SATURATED = 0xFFFFFFFF, 0xFFFFFFFE
SLOT_FIELDS = ("sequences", "diagonals", "votes", "diagonalSpans", "readBegins", "readEnds")
READ_FIELDS = ("numCandidates", "keptHits")
FIELDS = SLOT_FIELDS + READ_FIELDS + ("numOverflowed",)
DTYPES = {"sequences": np.uint32, "diagonals": np.int64, "votes": np.uint32, "diagonalSpans": np.uint32, "readBegins": np.uint32,
          "readEnds": np.uint32, "numCandidates": np.uint32, "keptHits": np.uint32}


class Instance:
    """the arrays of one call; num_seeds / num_hits are what the call is told (by default the arrays' sizes)"""

    def __init__(self, offsets, seed_ends, hit_offsets, positions, sequences=None, seed_lengths=None, fixed_length=0, num_seeds=None,
                 num_hits=None):
        self.offsets = np.asarray(offsets, np.uint64)
        self.seed_ends = np.asarray(seed_ends, np.uint32)
        self.hit_offsets = np.asarray(hit_offsets, np.uint64)
        self.positions = np.asarray(positions, np.uint64)
        self.sequences = None if sequences is None else np.asarray(sequences, np.uint32)
        self.seed_lengths = None if seed_lengths is None else np.asarray(seed_lengths, np.uint32)
        self.fixed_length = fixed_length
        self.num_seeds = len(self.seed_ends) if num_seeds is None else num_seeds
        self.num_hits = len(self.positions) if num_hits is None else num_hits
        self.num_reads = len(self.offsets) - 1

    def host(self, awfm, **params):
        return awfm.read_candidates_host(self.offsets, self.seed_ends, self.hit_offsets, self.positions, self.sequences, self.seed_lengths,
                                         self.fixed_length, num_seeds=self.num_seeds, num_hits=self.num_hits, **params)


def from_reads(reads, with_sequences=True, fixed_length=0):
    """reads: a list of reads, a read a list of seeds (seedEnd, length, [(sequence, position), ...])"""
    offsets, ends, lengths, hit_offsets, positions, sequences = [0], [], [], [0], [], []
    for read in reads:
        for end, length, hits in read:
            ends.append(end)
            lengths.append(length)
            for sequence, position in hits:
                sequences.append(sequence)
                positions.append(position)
            hit_offsets.append(len(positions))
        offsets.append(len(ends))
    return Instance(offsets, ends, hit_offsets, positions, sequences if with_sequences else None,
                    None if fixed_length else lengths, fixed_length)


# ---- the definition, restated ----
def _kept_hits(inst, r, max_hits_per_seed):
    """(sequence, diagonal int64, anchor, seedEnd) of read r's kept hits, or None for a malformed read"""
    first, last = int(inst.offsets[r]), int(inst.offsets[r + 1])
    if first > last or last > inst.num_seeds or last - first >= 1 << 32:
        return None
    begins, stops = inst.hit_offsets[first:last], inst.hit_offsets[first + 1:last + 1]
    if (begins > stops).any() or (stops > np.uint64(inst.num_hits)).any():
        return None
    seed_ends = inst.seed_ends[first:last].astype(np.int64)
    lengths = (inst.seed_lengths[first:last] if inst.seed_lengths is not None else np.full(last - first, inst.fixed_length)).astype(np.int64)
    counts = (stops - begins).astype(np.int64)
    usable = lengths <= seed_ends
    if max_hits_per_seed:
        usable &= counts <= max_hits_per_seed
    counts = np.where(usable, counts, 0)
    seed_of_hit = np.repeat(np.arange(last - first), counts)
    within = np.arange(counts.sum()) - np.repeat(np.cumsum(counts) - counts, counts)
    h = begins.astype(np.int64)[seed_of_hit] + within
    sequence = inst.sequences[h] if inst.sequences is not None else np.zeros(len(h), np.uint32)
    legal = sequence != NONE
    h, seed_of_hit, sequence = h[legal], seed_of_hit[legal], sequence[legal]
    anchor = (seed_ends - lengths)[seed_of_hit]
    with np.errstate(over="ignore"):
        diagonal = inst.positions[h].view(np.int64) - anchor
    return sequence, diagonal, anchor, seed_ends[seed_of_hit]


def expected(inst, max_hits_per_seed=0, band=0, min_votes=1, max_candidates=4, overflowed_before=0):
    """every output of the call by the definition, as awfm.read_candidates_host returns them"""
    n, slots = inst.num_reads, max_candidates
    out = {name: np.zeros((n, slots), DTYPES[name]) for name in SLOT_FIELDS}
    out.update({name: np.zeros(n, np.uint32) for name in READ_FIELDS})
    out["sequences"][...] = NONE
    overflowed = overflowed_before
    min_votes = max(min_votes, 1)
    for r in range(n):
        kept = _kept_hits(inst, r, max_hits_per_seed)
        if kept is None or len(kept[0]) > MAX_HITS:
            out["keptHits"][r] = MALFORMED if kept is None else min(len(kept[0]), SATURATED)
            overflowed += 1
            continue
        sequence, diagonal, anchor, seed_end = kept
        out["keptHits"][r] = len(sequence)
        if not len(sequence):
            continue
        order = np.lexsort((diagonal, sequence))
        sequence, diagonal, anchor, seed_end = sequence[order], diagonal[order], anchor[order], seed_end[order]
        gaps = np.diff(diagonal.view(np.uint64))  # (ascending: the differences do not wrap)
        heads = np.flatnonzero(np.concatenate([[True], (np.diff(sequence) != 0) | (gaps > np.uint64(band))]))
        votes = np.diff(np.concatenate([heads, [len(sequence)]]))
        lows, highs = diagonal[heads], np.maximum.reduceat(diagonal, heads)
        spans = np.minimum(highs.view(np.uint64) - lows.view(np.uint64), np.uint64(0xFFFFFFFF))
        begins, ends = np.minimum.reduceat(anchor, heads), np.maximum.reduceat(seed_end, heads)
        cand = np.flatnonzero(votes >= min_votes)
        cand = cand[np.lexsort((lows[cand], sequence[heads][cand], -votes[cand]))]
        out["numCandidates"][r] = len(cand)
        cand = cand[:slots]
        k = len(cand)
        out["sequences"][r, :k] = sequence[heads][cand]
        out["diagonals"][r, :k] = lows[cand]
        out["votes"][r, :k] = votes[cand]
        out["diagonalSpans"][r, :k] = spans[cand]
        out["readBegins"][r, :k] = begins[cand]
        out["readEnds"][r, :k] = ends[cand]
    out["numOverflowed"] = overflowed
    return out


def assert_equal(got, want, names=FIELDS, what=""):
    for name in names:
        g, w = got[name], want[name]
        if name == "numOverflowed":
            assert g == w, (what, name, g, w)
            continue
        bad = np.flatnonzero((np.asarray(g) != np.asarray(w)).reshape(len(w), -1).any(axis=1))
        assert not len(bad), (what, name, "reads", bad[:8].tolist(), np.asarray(g)[bad[:3]].tolist(), np.asarray(w)[bad[:3]].tolist())


# ---- instances ----
EDGE_BAND, EDGE_MAX_HITS = 5, 3
EDGE_READS = {}  # name -> read number in edge_instance()


def _many_hits(rng, count):
    """a read of `count` kept hits: seeds of EDGE_MAX_HITS hits each, in a few sequences, diagonals close and far"""
    seeds, left = [], count
    while left:
        take = min(EDGE_MAX_HITS, left)
        end = int(rng.integers(20, 150))
        hits = [(int(rng.integers(0, 3)), int(rng.integers(0, 3000)) + (end - 20)) for _ in range(take)]
        seeds.append((end, 20, hits))
        left -= take
    return seeds


def edge_instance():
    """one read per entry of the edge list, for EDGE_BAND and EDGE_MAX_HITS (the callers vary band, minVotes and C on top)"""
    rng = np.random.default_rng(4096)
    reads = [
        ("no seeds", []),
        ("seeds without hits", [(20, 20, []), (24, 20, [])]),
        ("one hit", [(20, 20, [(2, 777)])]),
        ("one diagonal", [(20 + 4 * i, 20, [(1, 1000 + 4 * i)]) for i in range(5)]),
        ("gaps of band", [(20, 20, [(0, 100)]), (24, 20, [(0, 109)]), (28, 20, [(0, 118)])]),  # diagonals 100, 105, 110
        ("gaps of band + 1", [(20, 20, [(0, 100)]), (24, 20, [(0, 110)])]),  # diagonals 100, 106
        ("neighbouring sequences", [(20, 20, [(3, 50), (4, 50)]), (22, 20, [(4, 52), (3, 52)])]),
        ("negative diagonals", [(15, 10, [(0, 0)]), (15, 10, [(0, 2)]), (30, 10, [(0, 21)])]),  # -5, -3, 1
        ("across 2^32", [(20, 20, [(0, (1 << 32) - 2)]), (30, 20, [(0, (1 << 32) + 12)]),  # 2^32 - 2 and 2^32 + 2: one cluster
                         (20, 20, [(9, 10), (9, 9 + (1 << 32)), (9, 8 + (1 << 33))])]),  # one cluster once band = 2^32 - 1, span saturated
        ("far ends of the keys", [(20, 20, [(0, (1 << 64) - 1), (0, 1 << 63), (0, (1 << 63) - 1)]), (25, 20, [(NONE - 1, 5), (0, 0)])]),
        ("ties", [(20, 20, [(2, 500), (1, 900), (1, 100)]), (24, 20, [(1, 904), (2, 504), (1, 104)])]),
        ("more than C", [(20 + i, 20, [(i % 3, 1000 * i + i)]) for i in range(20)]),
        ("at and above maxHitsPerSeed", [(20, 20, [(0, 10), (0, 1000), (0, 2000)]), (24, 20, [(0, 14), (0, 1004), (0, 2004), (0, 3004)])]),
        ("length beyond seedEnd", [(5, 10, [(0, 40), (0, 41)]), (20, 20, [(0, 60)]), (20, 21, [(0, 60)])]),
        ("illegal hits in between", [(20, 20, [(NONE, 7), (1, 300), (NONE, 9)]), (24, 20, [(1, 304), (NONE, 304)]), (28, 20, [(NONE, 1)])]),
        ("zero length", [(20, 0, [(0, 50)]), (20, 20, [(0, 30)])]),
        ("4096 kept hits", _many_hits(rng, MAX_HITS)),
        ("4097 kept hits", _many_hits(rng, MAX_HITS + 1)),
        ("after the overflow", [(20, 20, [(5, 123)])]),
    ]
    EDGE_READS.update({name: r for r, (name, _) in enumerate(reads)})
    return from_reads([read for _, read in reads])


MALFORMED_READS = (1, 3, 4, 5, 6, 7, 8)


def malformed_instance():
    """every malformed shape of the definition next to well-formed reads (0 and 2): a seed whose hit range is inverted (read 1),
    leaves numHits (3), both (4); a seed range that leaves numSeeds (5), is inverted (6, 7, 8)"""
    return Instance(offsets=[0, 2, 3, 4, 5, 6, 9, 6, 2, 0], seed_ends=[20, 24, 20, 20, 20, 20], hit_offsets=[0, 2, 4, 3, 5, 50, 6],
                    positions=[100, 200, 104, 300, 400, 500], sequences=[0, 0, 0, 1, 1, 1], fixed_length=20)


def dropped_seeds_instance():
    """reads whose kept seeds (up to 16 hits) stand between dropped ones of 17, 63, 64, 65, 70, 200 and 5000 hits, at every
    alignment to the 64 hits a wave reads per round; one read is a single dropped seed, one has them first and last"""
    rng = np.random.default_rng(64)

    def seed(hits):
        end = int(rng.integers(20, 150))
        return (end, 20, [(int(rng.integers(0, 2)), int(rng.integers(0, 400)) * 5 + end) for _ in range(hits)])

    reads = [[seed(3), seed(1000), seed(5), seed(70), seed(2)], [seed(5000)], [seed(64), seed(16), seed(64)], [seed(200), seed(1)],
             [seed(1), seed(63), seed(16), seed(65), seed(7), seed(17), seed(128), seed(16)]]
    reads += [[seed(int(rng.integers(0, 17))) for _ in range(k)] + [seed(64 + k)] + [seed(int(rng.integers(0, 17))) for _ in range(3)]
              for k in range(12)]
    return from_reads(reads)


def random_instance(seed, reads=120, with_sequences=True, fixed_length=0):
    """reads of 0..40 seeds of 0..6 hits: true loci (several seeds on one diagonal, some off by a little) among noise, seeds
    longer than their end, illegal hits"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(reads):
        read = []
        loci = [(int(rng.integers(0, 4)), int(rng.integers(0, 1 << 34))) for _ in range(int(rng.integers(0, 4)))]
        for _ in range(int(rng.integers(0, 41))):
            length = fixed_length or int(rng.integers(1, 65))
            end = int(rng.integers(max(length - 3, 0), 150))
            hits = []
            for _ in range(int(rng.integers(0, 7))):
                kind = rng.random()
                if loci and kind < 0.6:
                    sequence, diagonal = loci[int(rng.integers(0, len(loci)))]
                    hits.append((sequence, max(diagonal + (end - length) + int(rng.integers(-3, 4)), 0)))
                elif kind < 0.9:
                    hits.append((int(rng.integers(0, 4)), int(rng.integers(0, 1 << 34))))
                else:
                    hits.append((NONE, int(rng.integers(0, 1 << 34))))
            read.append((end, length, hits))
        out.append(read)
    return from_reads(out, with_sequences, fixed_length)


def sized_instance(sizes, seed=1):
    """one read per entry of sizes with that many kept hits (seeds of up to 8 hits, three sequences, diagonals from a range that
    grows with the read, so that clusters of many sizes form); built with arrays, not loops"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    seeds_per_read = (sizes + 7) // 8
    offsets = np.concatenate([[0], np.cumsum(seeds_per_read)])
    num_seeds = int(offsets[-1])
    read_of_seed = np.repeat(np.arange(len(sizes)), seeds_per_read)
    seed_in_read = np.arange(num_seeds) - offsets[read_of_seed]
    counts = np.minimum(sizes[read_of_seed] - 8 * seed_in_read, 8)
    hit_offsets = np.concatenate([[0], np.cumsum(counts)])
    seed_of_hit = np.repeat(np.arange(num_seeds), counts)
    seed_ends = rng.integers(24, 150, num_seeds)
    total = int(hit_offsets[-1])
    spread = 40 + 3 * sizes[read_of_seed[seed_of_hit]]
    positions = (rng.integers(0, 1 << 20, total) % spread) * 7 + (seed_ends[seed_of_hit] - 24) + 1000
    return Instance(offsets, seed_ends, hit_offsets, positions, rng.integers(0, 3, total), fixed_length=24)


def many_small_reads_instance(reads=6000, with_sequences=True):
    """more reads than the 4096 items below which the library's parallel loop stays on the calling thread, of 0..40 kept hits"""
    inst = sized_instance(np.random.default_rng(6000).integers(0, 41, reads), seed=12)
    if not with_sequences:
        inst.sequences = None
    return inst


# ---- end to end on the host: FASTA -> reads -> longest matches -> located -> mapped -> candidates ----
E2E_STEP, E2E_CAP, E2E_MIN_LENGTH, E2E_MAX_HITS, E2E_READ_LENGTH = 4, 64, 14, 16, 120


def planted_reads(records, seed=21, count=48):
    """-> (reads, planted): reads of 120 characters cut from records of at least 200 with a substitution at every 30th character
    (positions 15, 45, 75, 105: stretches of 29 matching characters remain); every third of them has the character at position
    60 deleted (and one more taken from the record, to stay 120 long); every sixth read is random.  planted[i] = (record,
    offset, deleted) or None."""
    import longest_match_common as lm
    rng = np.random.default_rng(seed)
    long_enough = [i for i, r in enumerate(records) if len(r) >= 200]
    other = {ord("a"): b"c", ord("c"): b"g", ord("g"): b"t", ord("t"): b"a"}
    reads, planted = [], []
    for i in range(count):
        if i % 6 == 5:
            reads.append(lm.random_text(rng, E2E_READ_LENGTH, lm.DNA))
            planted.append(None)
            continue
        record = long_enough[int(rng.integers(0, len(long_enough)))]
        deleted = i % 3 == 1
        at = int(rng.integers(0, len(records[record]) - E2E_READ_LENGTH - 1))
        piece = bytearray(records[record][at:at + E2E_READ_LENGTH + (1 if deleted else 0)])
        if deleted:
            del piece[60]
        for p in range(15, E2E_READ_LENGTH, 30):
            piece[p:p + 1] = other[piece[p]]
        reads.append(bytes(piece))
        planted.append((record, at, deleted))
    return reads, planted


def windows_of(reads):
    """the longest-match windows: ending at every 4th position of every read, at most 64 characters -> (chars, starts, ends,
    read seed offsets, seed ends)"""
    chars = np.frombuffer(b"".join(reads), np.uint8)
    read_at = np.concatenate([[0], np.cumsum([len(r) for r in reads])])
    starts, ends, seed_ends, offsets = [], [], [], [0]
    for r, read in enumerate(reads):
        for e in range(E2E_STEP, len(read) + 1, E2E_STEP):
            starts.append(read_at[r] + max(e - E2E_CAP, 0))
            ends.append(read_at[r] + e)
            seed_ends.append(e)
        offsets.append(len(ends))
    return chars, np.array(starts, np.uint64), np.array(ends, np.uint64), np.array(offsets, np.uint64), np.array(seed_ends, np.uint32)


def host_pipeline(awfm, ix, reads):
    """the inputs of the candidates call from the host's own calls: awfmLongestSuffixMatches, the host's locate of every row of
    every range, awfmLocalPositions"""
    from avxwindowfmindex_amd import _lib
    chars, starts, ends, offsets, seed_ends = windows_of(reads)
    lengths, ranges, counts = awfm.longest_suffix_matches_host(ix, chars, starts, ends, min_length=E2E_MIN_LENGTH)
    hit_offsets = np.concatenate([[0], np.cumsum(counts.astype(np.uint64))]).astype(np.uint64)
    L, ok = _lib.lib(), C.c_int(0)
    rows = np.array([L.awFmFindDatabaseHitPositionSingle(ix.ptr, int(p), C.byref(ok))
                     for (sp, ep), count in zip(ranges, counts) if count for p in range(int(sp), int(ep) + 1)], np.uint64)
    sequences, local, _ = awfm.local_positions_host(ix, rows)
    return Instance(offsets, seed_ends, hit_offsets, local, sequences, seed_lengths=lengths)


def assert_planted_reads_found(result, planted, band):
    """EVERY planted read: candidate 0 is its record, on a diagonal within band of the planted offset"""
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, _ = plant
        assert result["numCandidates"][r] >= 1 and result["sequences"][r, 0] == record, (r, plant, result["sequences"][r].tolist())
        assert abs(int(result["diagonals"][r, 0]) - at) <= band, (r, plant, result["diagonals"][r].tolist())
