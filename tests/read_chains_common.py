"""Shared by the tests of awfmReadChains / awfmGpuReadChains (include/awfm_gpu.h, "read chains"): a plain-Python restatement of
the definition (lists, loops and Python's exact integers: no code shared with the C, no NumPy arithmetic), a brute-force search
over all chains of a small slot as a second oracle, and the instances -- the edge list, hand-made slots, batches of given sizes.
The inputs are those of tests/read_candidates_common.py (rc.Instance); a case is an instance and its slot arrays."""
import itertools

import numpy as np

import read_candidates_common as rc

NONE = 0xFFFFFFFF
NO_SLOT = 0xFFFFFFFF
MAX_HITS = 4096
MAX_LOOKBACK = 64
MALFORMED, SATURATED = 0xFFFFFFFF, 0xFFFFFFFE
SLOT_FIELDS = ("chainScores", "chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
READ_FIELDS = ("bestSlots", "keptHits")
FIELDS = SLOT_FIELDS + READ_FIELDS + ("numOverflowed",)
DTYPES = {"chainScores": np.uint32, "chainAnchors": np.uint32, "chainReadBegins": np.uint32, "chainReadEnds": np.uint32,
          "chainBeginDiagonals": np.int64, "chainEndDiagonals": np.int64, "bestSlots": np.uint32, "keptHits": np.uint32}


class Case:
    """an instance (rc.Instance) and the slot arrays of its reads, shaped (reads, C)"""

    def __init__(self, inst, sequences, diagonals, spans):
        self.inst = inst
        self.sequences = np.ascontiguousarray(sequences, np.uint32).reshape(inst.num_reads, -1)
        self.diagonals = np.ascontiguousarray(diagonals, np.int64).reshape(self.sequences.shape)
        self.spans = np.ascontiguousarray(spans, np.uint32).reshape(self.sequences.shape)
        self.slots = self.sequences.shape[1]

    def host(self, awfm, **params):
        i = self.inst
        return awfm.read_chains_host(i.offsets, i.seed_ends, i.hit_offsets, i.positions, self.sequences, self.diagonals, self.spans,
                                     i.sequences, i.seed_lengths, i.fixed_length, num_seeds=i.num_seeds, num_hits=i.num_hits, **params)


def candidate_case(awfm, inst, band, slots, max_hits_per_seed=0, min_votes=1):
    """the case whose slots awfmReadCandidates writes for the instance (tests/test_read_candidates.py pins that call)"""
    got = inst.host(awfm, max_hits_per_seed=max_hits_per_seed, band=band, min_votes=min_votes, max_candidates=slots)
    return Case(inst, got["sequences"], got["diagonals"], got["diagonalSpans"])


# ---- the definition, restated in plain Python ----
def _signed(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def kept_hits(inst, r, max_hits_per_seed):
    """[(sequence, D, e, len)] of read r's kept hits in the order of the arrays, or None for a malformed read"""
    first, last = int(inst.offsets[r]), int(inst.offsets[r + 1])
    if first > last or last > inst.num_seeds or last - first >= 1 << 32:
        return None
    for s in range(first, last):
        if int(inst.hit_offsets[s]) > int(inst.hit_offsets[s + 1]) or int(inst.hit_offsets[s + 1]) > inst.num_hits:
            return None
    out = []
    for s in range(first, last):
        e = int(inst.seed_ends[s])
        length = int(inst.seed_lengths[s]) if inst.seed_lengths is not None else inst.fixed_length
        begin, stop = int(inst.hit_offsets[s]), int(inst.hit_offsets[s + 1])
        if length > e or (max_hits_per_seed and stop - begin > max_hits_per_seed):
            continue
        for h in range(begin, stop):
            sequence = int(inst.sequences[h]) if inst.sequences is not None else 0
            if sequence != NONE:
                out.append((sequence, _signed(int(inst.positions[h]) - (e - length)), e, length))
    return out


def compatible(x, y, band):
    """anchor y = (e, D, len) may directly precede anchor x"""
    dr, dd = x[0] - y[0], x[1] - y[1]
    return dr > 0 and dr + dd > 0 and abs(dd) <= band


def link(x, y, gap_penalty):
    """what anchor x adds to a chain that ends in y"""
    dr, dd = x[0] - y[0], x[1] - y[1]
    return min(x[2], dr, dr + dd) - abs(dd) * gap_penalty


def chain(anchors, band, lookback, gap_penalty):
    """the recurrence over a slot's anchors [(e, D, len)] in their order -> per anchor (f, first a, first D, anchors)"""
    state = []
    for i, x in enumerate(anchors):
        best, source = None, None
        for j in range(max(0, i - lookback), i):
            if compatible(x, anchors[j], band):
                value = state[j][0] + link(x, anchors[j], gap_penalty)
                if best is None or value >= best:  # ties: the largest j
                    best, source = value, j
        if best is not None and best > x[2]:
            state.append((best, state[source][1], state[source][2], state[source][3] + 1))
        else:
            state.append((x[2], x[0] - x[2], x[1], 1))
        assert state[-1][0] <= x[0]  # f(i) <= e_i
    return state


def slot_anchors(kept, sequence, diagonal, span):
    return sorted((e, D, length) for s, D, e, length in kept if s == sequence and 0 <= D - diagonal <= span)


def slots_intersect(sequences, diagonals, spans):
    for j, k in itertools.combinations(range(len(sequences)), 2):
        if sequences[j] != NONE and sequences[j] == sequences[k]:
            if diagonals[j] <= diagonals[k] + spans[k] and diagonals[k] <= diagonals[j] + spans[j]:
                return True
    return False


def expected(case, max_hits_per_seed=0, band=0, lookback=MAX_LOOKBACK, gap_penalty=0, overflowed_before=0, reads=None):
    """every output of the call by the definition, as awfm.read_chains_host returns them (reads: only these, the others zero)"""
    inst, n, slots = case.inst, case.inst.num_reads, case.slots
    out = {name: np.zeros((n, slots), DTYPES[name]) for name in SLOT_FIELDS}
    out.update({name: np.zeros(n, np.uint32) for name in READ_FIELDS})
    overflowed = overflowed_before
    for r in (range(n) if reads is None else reads):
        sequences = [int(x) for x in case.sequences[r]]
        diagonals = [int(x) for x in case.diagonals[r]]
        spans = [int(x) for x in case.spans[r]]
        kept = kept_hits(inst, r, max_hits_per_seed)
        if kept is not None and slots_intersect(sequences, diagonals, spans):
            kept = None
        out["bestSlots"][r] = NO_SLOT
        if kept is None or len(kept) > MAX_HITS:
            out["keptHits"][r] = MALFORMED if kept is None else min(len(kept), SATURATED)
            overflowed += 1
            continue
        out["keptHits"][r] = len(kept)
        best_slot, best_score = NO_SLOT, -1
        for j in range(slots):
            if sequences[j] == NONE:
                continue
            anchors = slot_anchors(kept, sequences[j], diagonals[j], spans[j])
            if not anchors:
                continue
            state = chain(anchors, band, lookback, gap_penalty)
            last = max(range(len(state)), key=lambda i: (state[i][0], -i))  # the largest f, ties to the smallest position
            f, first_a, first_d, count = state[last]
            out["chainScores"][r, j], out["chainAnchors"][r, j] = f, count
            out["chainReadBegins"][r, j], out["chainReadEnds"][r, j] = first_a, anchors[last][0]
            out["chainBeginDiagonals"][r, j], out["chainEndDiagonals"][r, j] = first_d, anchors[last][1]
            if f > best_score:
                best_slot, best_score = j, f
        out["bestSlots"][r] = best_slot
    out["numOverflowed"] = overflowed
    return out


def brute_force_score(anchors, band, gap_penalty):
    """the best score over ALL order-respecting subsequences of a slot's anchors whose consecutive pairs are compatible"""
    best = 0
    for size in range(1, len(anchors) + 1):
        for picked in itertools.combinations(range(len(anchors)), size):
            if all(compatible(anchors[b], anchors[a], band) for a, b in zip(picked, picked[1:])):
                score = anchors[picked[0]][2] + sum(link(anchors[b], anchors[a], gap_penalty) for a, b in zip(picked, picked[1:]))
                best = max(best, score)
    return best


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


def anchor(e, length, diagonal, sequence=0):
    """a seed with one hit that is the anchor (e, D, len) in `sequence`"""
    return (e, length, [(sequence, (diagonal + e - length) % (1 << 64))])


def edge_instance():
    """one read per entry of the edge list, for EDGE_BAND and EDGE_MAX_HITS; its slots come from awfmReadCandidates"""
    rng = np.random.default_rng(4096)
    reads = [
        ("empty read", []),
        ("seeds without hits", [(20, 20, []), (24, 20, [])]),
        ("one anchor", [anchor(20, 20, 100, 2)]),
        ("equal e", [anchor(20, 20, 100), anchor(20, 10, 102)]),
        ("dt = 0", [anchor(20, 10, 100), anchor(24, 10, 96)]),
        ("dt = 1", [anchor(20, 10, 100), anchor(24, 10, 97)]),
        ("g = band", [anchor(20, 10, 100), anchor(30, 10, 105)]),
        # 100 -> 106 would score 20 but is 6 apart; the anchor between shares e with the first, so only 103 -> 106 chains: 15
        ("g = band + 1", [anchor(20, 10, 100), anchor(20, 5, 103), anchor(30, 10, 106)]),
        ("one diagonal", [anchor(20 + 4 * i, 20, 1000, 1) for i in range(5)]),
        ("drift", [anchor(20 + 10 * i, 10, 500 + 2 * i) for i in range(6)]),
        ("zero length alone", [anchor(20, 0, 100)]),
        ("zero length in a chain", [anchor(20, 10, 100), anchor(25, 0, 100), anchor(40, 10, 100)]),
        ("negative diagonals", [(15, 10, [(0, 0)]), (30, 10, [(0, 17)]), (45, 10, [(0, 33)])]),  # -5, -3, -2
        ("across 2^32", [anchor(20, 20, (1 << 32) - 2), anchor(30, 20, (1 << 32) + 2),
                         anchor(20, 20, 10, 9), anchor(30, 20, 9 + (1 << 32), 9), anchor(40, 20, 8 + (1 << 33), 9)]),
        ("far ends of the keys", [(20, 20, [(0, (1 << 64) - 1), (0, 1 << 63), (0, (1 << 63) - 1)]), (25, 20, [(NONE - 1, 5), (0, 0)])]),
        # both predecessors give 20 without a penalty: the later one (D 101) wins; with a penalty the first
        ("tie between predecessors", [anchor(10, 10, 100), anchor(10, 10, 101), anchor(30, 10, 100)]),
        # two chains of 30 that cannot join (equal e pairwise): the one that ends first in the order wins
        ("tie between chain ends", [anchor(20, 20, 100), anchor(20, 20, 104), anchor(30, 20, 100), anchor(30, 20, 104)]),
        ("two sequences", [anchor(20, 20, 50, 3), anchor(20, 20, 50, 4), anchor(32, 20, 52, 4), anchor(30, 20, 52, 3)]),
        ("more loci than C", [anchor(20 + i, 20, 1000 * i + i, i % 3) for i in range(20)]),
        ("at and above maxHitsPerSeed", [(20, 20, [(0, 10), (0, 1000), (0, 2000)]), (24, 20, [(0, 14), (0, 1004), (0, 2004), (0, 3004)]),
                                         (30, 20, [(0, 20)])]),
        ("length beyond seedEnd", [(5, 10, [(0, 40), (0, 41)]), (20, 20, [(0, 60)]), (20, 21, [(0, 60)]), (30, 20, [(0, 70)])]),
        ("illegal hits in between", [(20, 20, [(NONE, 7), (1, 300), (NONE, 9)]), (24, 20, [(1, 304), (NONE, 304)]), (28, 20, [(NONE, 1)])]),
        ("a repeat seed", [anchor(20, 20, 100), (30, 20, [(0, 110), (0, 112)]), anchor(40, 20, 100)]),  # D 100, 100 and 102, 100
        ("4096 kept hits", rc._many_hits(rng, MAX_HITS)),
        ("4097 kept hits", rc._many_hits(rng, MAX_HITS + 1)),
        ("after the overflow", [anchor(20, 20, 123, 5)]),
    ]
    EDGE_READS.update({name: r for r, (name, _) in enumerate(reads)})
    return rc.from_reads([read for _, read in reads])


def lookback_case():
    """hand-made slots.  Read 0: a slot of 66 anchors whose last (e 100, len 20) has one good predecessor at distance 64 (len 5:
    25) and a better one at distance 65 (len 12: 32), out of reach of lookback 64; the 63 anchors between share e and lie more
    than the band from all three.  Read 1: slots that hold none of the read's hits, an unused slot between used ones.
    Read 2: one slot that holds hits of two clusters (the call does not depend on how the slots were made)."""
    far = [(50, 10, [(0, 1010 + k + 40)]) for k in range(63)]  # D = 1010 + k
    reads = [[anchor(30, 12, 1000), anchor(30, 5, 1001)] + far + [anchor(100, 20, 1000)],
             [anchor(20, 20, 100, 1), anchor(30, 20, 100, 1)],
             [anchor(20, 10, 100), anchor(40, 10, 100), anchor(60, 10, 140), anchor(80, 10, 140)]]
    inst = rc.from_reads(reads)
    sequences = [[0, NONE, NONE], [1, NONE, 1], [NONE, 0, 7]]
    diagonals = [[1000, 0, 0], [0, 0, 100], [5, 100, 100]]
    spans = [[10000, 0, 0], [99, 0xFFFFFFFF, 0], [0xFFFFFFFF, 40, 40]]
    return Case(inst, sequences, diagonals, spans)


INTERSECTING_READS = (1, 2, 4)


def intersecting_case():
    """reads 1, 2 and 4 are malformed by their slots alone: intervals of one sequence that share a diagonal, that nest, that meet
    at the top of the keys; reads 0 and 3 have slots that touch nothing (neighbours one apart, other sequences, unused twins)"""
    reads = [[anchor(20, 20, 100), anchor(30, 20, 111)]] * 4 + [[anchor(20, 20, (1 << 63) - 1)]]
    inst = rc.from_reads(reads)
    sequences = [[0, 0, NONE, NONE], [0, 0, 1, 1], [0, 5, 0, 6], [0, 1, NONE, NONE], [0, 0, 2, 3]]
    diagonals = [[100, 111, 100, 100], [100, 110, 0, 50], [0, 0, 100, 0], [100, 100, 0, 0], [(1 << 63) - 1, (1 << 63) - 5, 0, 0]]
    spans = [[10, 5, 50, 50], [10, 5, 10, 10], [0xFFFFFFFF, 0, 0, 0], [11, 11, 0, 0], [0xFFFFFFFF, 4, 0, 0]]
    return Case(inst, sequences, diagonals, spans)


def sized_case(sizes, loci=4, slots=None, seed=1, span=3):
    """one read per entry of sizes with that many kept hits, ALL of them anchors: read r's hits lie in min(loci, slots) loci
    (sequence k % 3, diagonals of a few around a base of the locus' own), seeds of up to 8 hits with lengths of their own, seed
    ends from a range that grows with the read so that long chains form; the slots are the loci, hand-made.  Built with arrays."""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    slots = loci if slots is None else slots
    seeds_per_read = (sizes + 7) // 8
    offsets = np.concatenate([[0], np.cumsum(seeds_per_read)])
    num_seeds = int(offsets[-1])
    read_of_seed = np.repeat(np.arange(len(sizes)), seeds_per_read)
    seed_in_read = np.arange(num_seeds) - offsets[read_of_seed]
    counts = np.minimum(sizes[read_of_seed] - 8 * seed_in_read, 8)
    hit_offsets = np.concatenate([[0], np.cumsum(counts)])
    seed_of_hit = np.repeat(np.arange(num_seeds), counts)
    lengths = rng.integers(1, 25, num_seeds)
    seed_ends = 24 + rng.integers(0, 1 << 30, num_seeds) % (40 + sizes[read_of_seed])
    total = int(hit_offsets[-1])
    locus = rng.integers(0, min(loci, slots), total)
    base = 1000 + 100000 * locus
    positions = base + rng.integers(0, span + 1, total) + (seed_ends - lengths)[seed_of_hit]
    inst = rc.Instance(offsets, seed_ends, hit_offsets, positions, locus % 3, seed_lengths=lengths)
    n = len(sizes)
    k = np.arange(slots)
    used = k < loci
    sequences = np.where(used, k % 3, NONE)[None, :].repeat(n, axis=0)
    diagonals = np.where(used, 1000 + 100000 * k, 0)[None, :].repeat(n, axis=0)
    spans = np.where(used, span, 0)[None, :].repeat(n, axis=0)
    return Case(inst, sequences, diagonals, spans)


def assert_planted_reads_chained(result, case, planted, seed_length):
    """EVERY planted read: the best slot is its record, and the chain's text interval holds the planted one shrunk by a seed
    length at each end"""
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        j = int(result["bestSlots"][r])
        assert j != NO_SLOT and case.sequences[r, j] == record, (r, plant)
        begin = int(result["chainReadBegins"][r, j]) + int(result["chainBeginDiagonals"][r, j])
        end = int(result["chainReadEnds"][r, j]) + int(result["chainEndDiagonals"][r, j])
        planted_end = at + rc.E2E_READ_LENGTH + (1 if deleted else 0)
        assert begin <= at + seed_length and end >= planted_end - seed_length, (r, plant, begin, end)
        assert at <= begin and end <= planted_end, (r, plant, begin, end)
