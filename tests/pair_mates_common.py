"""Pair mates (include/awfm_gpu.h "pair mates", csrc/awfm_pair_mates.c) restated in plain Python loops for the tests of the host
twins and the device calls: every candidate (a, b) of a pair in turn, the header's rules in the header's order, Python integers
wrapped to 64-bit two's complement where the header says so; the reverse complement byte by byte; and cases: random slot tables
and the EDGE LIST, one pair an edge with hand-computed expectations (literals: the restatement is held to them as well)."""
import os

import numpy as np

NONE, MALFORMED, TOO_WIDE, TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NO_SLOT = 0xFFFFFFFF     # AWFM_CHAINS_NO_SLOT
NO_WINDOW = 0xFFFFFFFF   # AWFM_CANDIDATES_NONE
SLOT_INPUTS = dict(sequences=np.uint32, slotScores=np.uint32, slotReadEnds=np.uint32, slotTextEnds=np.uint64)
PAIR_OUTPUTS = dict(properPairs=np.uint8, pairScores=np.uint32, pairSecondScores=np.uint32, templateLengths=np.int64, pairQualities=np.uint8)
READ_OUTPUTS = dict(pairSlots=np.uint32, mappingQualities=np.uint8, windowSequences=np.uint32, windowBegins=np.uint64, windowEnds=np.uint64)
COUNTERS = ("numProper", "numWindows")
NAMES = list(PAIR_OUTPUTS) + list(READ_OUTPUTS) + list(COUNTERS)
ALL, ODD, EVEN = 0, 1, 2  # AWFM_COMPLEMENT_*
PARAMS = dict(min_insert=200, max_insert=500, min_score=0, unpaired_penalty=17, window_pad=50, mapq_cap=60)


def wrap(x):
    """x as a 64-bit two's complement number"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


class Case:
    """offsets uint64[2 pairs + 1], slots: the four arrays shaped (reads, C), qualities uint8[reads] or None, params: the keyword
    arguments of pair_mates_host"""

    def __init__(self, offsets, slots, qualities, params):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.slots = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in SLOT_INPUTS.items()}
        self.qualities = None if qualities is None else np.ascontiguousarray(qualities, dtype=np.uint8)
        self.params = dict(PARAMS, **params)
        self.num_reads = self.offsets.size - 1
        self.num_pairs = self.num_reads // 2
        self.C = self.slots["sequences"].shape[1]

    def host(self, awfm, **kw):
        return awfm.pair_mates_host(self.offsets, self.slots, mapping_qualities=self.qualities, **dict(self.params, **kw))

    def expected(self, proper_before=0, windows_before=0):
        return expected(self, proper_before, windows_before)


def expected(case, proper_before=0, windows_before=0):
    """the header's rules 1 to 8, pair by pair"""
    q, C = case.params, case.C
    floor = max(q["min_score"], 1)
    out = {name: np.zeros(case.num_pairs, dtype) for name, dtype in PAIR_OUTPUTS.items()}
    out.update({name: np.zeros(case.num_reads, dtype) for name, dtype in READ_OUTPUTS.items()})
    proper_pairs, windows = proper_before, windows_before
    for p in range(case.num_pairs):
        reads = (2 * p, 2 * p + 1)
        n, slots, best = [], [], []
        for r in reads:
            begin, end = int(case.offsets[r]), int(case.offsets[r + 1])
            n.append(wrap(end - begin))
            mine = []
            for j in range(C):
                score, sequence = int(case.slots["slotScores"][r, j]), int(case.slots["sequences"][r, j])
                read_end, text_end = int(case.slots["slotReadEnds"][r, j]), int(case.slots["slotTextEnds"][r, j])
                counts = begin <= end and score < TOO_LONG and score >= floor
                mine.append(dict(counts=counts, score=score, sequence=sequence, end=(read_end, text_end), start=wrap(text_end - read_end)))
            slots.append(mine)
            top = None
            for j in range(C):
                if mine[j]["counts"] and (top is None or mine[j]["score"] > mine[top]["score"]):
                    top = j
            best.append(top)
        candidates = []  # (value, concordant, a, b, T)
        for a in range(C):
            for b in range(C):
                x, y = slots[0][a], slots[1][b]
                if not (x["counts"] and y["counts"]):
                    continue
                T = wrap(y["start"] + n[1] - x["start"])
                if x["sequence"] == y["sequence"] and q["min_insert"] <= T <= q["max_insert"]:
                    candidates.append((x["score"] + y["score"], True, a, b, T))
                elif a == best[0] and b == best[1]:
                    candidates.append((max(0, x["score"] + y["score"] - q["unpaired_penalty"]), False, a, b, T))
        winner = None
        for k in candidates:  # the largest value, then the concordant one, then the lowest a, then the lowest b
            if winner is None or (k[0], k[1], -k[2], -k[3]) > (winner[0], winner[1], -winner[2], -winner[3]):
                winner = k

        def same(m, j, k):
            x, y = slots[m][j], slots[m][k]
            return j == k or (x["counts"] and y["counts"] and x["sequence"] == y["sequence"] and x["end"] == y["end"])

        second = 0
        for k in candidates:
            if winner is not None and same(0, k[2], winner[2]) and same(1, k[3], winner[3]):
                continue
            second = max(second, k[0])
        is_proper = winner is not None and winner[1]
        chosen = list(best)
        value = 0
        if winner is not None:
            chosen, value = [winner[2], winner[3]], winner[0]
        elif best[0] is not None:
            value = slots[0][best[0]]["score"]
        elif best[1] is not None:
            value = slots[1][best[1]]["score"]
        quality = q["mapq_cap"] * (winner[0] - second) // winner[0] if is_proper else 0
        proper_pairs += int(is_proper)
        out["properPairs"][p] = int(is_proper)
        out["pairScores"][p] = value & 0xFFFFFFFF
        out["pairSecondScores"][p] = second & 0xFFFFFFFF
        out["templateLengths"][p] = winner[4] if is_proper else 0
        out["pairQualities"][p] = quality
        for m, r in enumerate(reads):
            given = 0 if case.qualities is None else int(case.qualities[r])
            mine = 0 if best[m] is None else given
            if is_proper:
                mine = max(quality, given if chosen[m] == best[m] else 0)
            other = 1 - m
            window = (NO_WINDOW, 0, 0)
            if not is_proper and best[other] is not None:
                s = slots[other][best[other]]
                pad, S = q["window_pad"], s["start"]
                if m == 1:
                    lo, hi = wrap(S + q["min_insert"] - n[1] - pad), wrap(S + q["max_insert"] + pad)
                else:
                    E = wrap(S + n[1])
                    lo, hi = wrap(E - q["max_insert"] - pad), wrap(E - q["min_insert"] + n[0] + pad)
                window = (s["sequence"], max(lo, 0), max(hi, 0))
                windows += 1
            out["pairSlots"][r] = NO_SLOT if chosen[m] is None else chosen[m]
            out["mappingQualities"][r] = mine
            out["windowSequences"][r], out["windowBegins"][r], out["windowEnds"][r] = window
    out["numProper"], out["numWindows"] = proper_pairs, windows
    return out


def assert_equal(got, want, names=None, what=""):
    for name in NAMES if names is None else names:
        if name in COUNTERS:
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            g, w = np.asarray(got[name]), np.asarray(want[name])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            if not np.array_equal(g, w):
                at = int(np.argwhere(g != w)[0][0])
                raise AssertionError(f"{what}: {name}[{at}] is {g[at]}, expected {w[at]} ({(g != w).sum()} differ)")


def random_case(seed, pairs, C, params=None, qualities=True, big=False):
    """slot tables as slot scores might write them, made to collide: a few sequences, starts on a coarse grid around a fragment
    per pair, scores from a small range (ties), a fifth of the slots a status, some duplicates, some reads with inverted offsets;
    big: scores just below 2^24"""
    rng = np.random.default_rng(seed)
    n = 2 * pairs
    lengths = rng.integers(0, 200, n).astype(np.int64)
    inverted = rng.random(n) < 0.03
    offsets = np.zeros(n + 1, np.int64)
    offsets[0] = 1000
    for r in range(n):
        offsets[r + 1] = offsets[r] + (-int(rng.integers(1, 50)) if inverted[r] else lengths[r])
    slots = {name: np.zeros((n, C), dtype) for name, dtype in SLOT_INPUTS.items()}
    for p in range(pairs):
        fragment = int(rng.integers(0, 3000))
        for m in range(2):
            r = 2 * p + m
            for j in range(C):
                kind = rng.random()
                if kind < 0.2:
                    slots["slotScores"][r, j] = int(rng.choice([NONE, MALFORMED, TOO_WIDE, TOO_LONG]))
                    slots["sequences"][r, j] = NO_WINDOW if rng.random() < 0.5 else int(rng.integers(0, 3))
                    continue
                if kind < 0.3 and j > 0:  # the slot before once more: a duplicate when that one counts
                    for name in slots:
                        slots[name][r, j] = slots[name][r, j - 1]
                    if rng.random() < 0.3:
                        slots["slotScores"][r, j] = int(rng.integers(0, 12))
                    continue
                score = int(rng.integers(0, 12)) + ((1 << 24) - 12 if big and rng.random() < 0.7 else 0)
                read_end = int(rng.integers(0, 200))
                start = fragment + (0 if m == 0 else 190) + 10 * int(rng.integers(-3, 4)) - (0 if rng.random() < 0.9 else 3000)
                slots["slotScores"][r, j] = score
                slots["sequences"][r, j] = int(rng.integers(0, 2))
                slots["slotReadEnds"][r, j] = read_end
                slots["slotTextEnds"][r, j] = max(start + read_end, 0)
    given = rng.integers(0, 61, n).astype(np.uint8) if qualities else None
    return Case(offsets.astype(np.uint64), slots, given, params or {})


# ---- the edge list ----------------------------------------------------------------------------------------------------------
def slot(score, sequence, start, read_end=100):
    """(score, sequence, readEnd, textEnd) of a slot whose START is `start`"""
    return (score, sequence, read_end, start + read_end)


STATUS = (NONE, NO_WINDOW, 0, 0)
NO_W = (NO_WINDOW, 0, 0)
BIG = (1 << 24) - 1


class Edge:
    """one pair: the slots of mate A and of mate B, the lengths of the two reads (a negative length: inverted offsets), the input
    qualities (None: the array is NULL), params, and want: the hand-computed outputs -- per pair a value, per read a pair"""

    def __init__(self, name, a, b, want, lengths=(100, 100), qualities=(30, 25), **params):
        self.name, self.a, self.b, self.want, self.lengths, self.qualities, self.params = name, a, b, want, lengths, qualities, params


def improper(slots, score, second, qualities, windows):
    return dict(properPairs=0, pairSlots=slots, pairScores=score, pairSecondScores=second, templateLengths=0, pairQualities=0,
                mappingQualities=qualities, windows=windows)


def proper(slots, score, second, T, quality, qualities):
    return dict(properPairs=1, pairSlots=slots, pairScores=score, pairSecondScores=second, templateLengths=T, pairQualities=quality,
                mappingQualities=qualities, windows=(NO_W, NO_W))


NOTHING = improper((NO_SLOT, NO_SLOT), 0, 0, (0, 0), (NO_W, NO_W))
EDGES = [
    # four candidates of value 90: the lowest a, then the lowest b; the three others are no duplicates, so the second is 90
    Edge("tie between concordant candidates", [slot(50, 0, 1000), slot(50, 0, 1010)], [slot(40, 0, 1200), slot(40, 0, 1210)],
         proper((0, 0), 90, 90, 300, 0, (30, 25))),
    # (1, 0) is concordant with 43 + 60, (best, best) = (0, 0) discordant with 60 + 60 - 17: the concordant one goes first; read A
    # is not placed at its best slot, so its own quality does not count
    Edge("a concordant and a discordant candidate of equal value", [slot(60, 0, 1000), slot(43, 1, 5000)], [slot(60, 1, 5200)],
         proper((1, 0), 103, 103, 300, 0, (0, 25))),
    Edge("unpairedPenalty larger than the sum", [slot(60, 0, 1000)], [slot(60, 1, 5000)],
         improper((0, 0), 0, 0, (30, 25), ((1, 4550, 5050), (0, 1050, 1550))), unpaired_penalty=1000),
    Edge("T at minInsert", [slot(50, 0, 1000)], [slot(50, 0, 1100)], proper((0, 0), 100, 0, 200, 60, (60, 60))),
    Edge("T at maxInsert", [slot(50, 0, 1000)], [slot(50, 0, 1400)], proper((0, 0), 100, 0, 500, 60, (60, 60))),
    Edge("T one below minInsert", [slot(50, 0, 1000)], [slot(50, 0, 1099)],
         improper((0, 0), 83, 0, (30, 25), ((0, 649, 1149), (0, 1050, 1550)))),
    Edge("T one above maxInsert", [slot(50, 0, 1000)], [slot(50, 0, 1401)],
         improper((0, 0), 83, 0, (30, 25), ((0, 951, 1451), (0, 1050, 1550)))),
    Edge("a negative minInsert, proper", [slot(50, 0, 1000)], [slot(50, 0, 700)], proper((0, 0), 100, 0, -200, 60, (60, 60)),
         min_insert=-300, max_insert=-100),
    Edge("a negative minInsert, windows", [slot(50, 0, 1000)], [slot(50, 0, 5000)],
         improper((0, 0), 83, 0, (30, 25), ((0, 5150, 5550), (0, 550, 950))), min_insert=-300, max_insert=-100),
    Edge("a negative start", [(50, 0, 100, 60)], [slot(50, 0, 200)], proper((0, 0), 100, 0, 340, 60, (60, 60))),
    # slot 1 of A is slot 0 once more: (1, 0) duplicates the winner, the second is (2, 0) with 30 + 40
    Edge("a duplicate of the winner", [slot(50, 0, 1000), slot(50, 0, 1000), slot(30, 0, 1020)], [slot(40, 0, 1200)],
         proper((0, 0), 90, 70, 300, 13, (30, 25))),
    Edge("the second is the discordant candidate", [slot(60, 0, 1000), slot(50, 1, 5000)], [slot(60, 1, 5200)],
         proper((1, 0), 110, 103, 300, 3, (3, 25))),
    Edge("the winner is the discordant candidate", [slot(60, 0, 1000), slot(40, 1, 5000)], [slot(60, 1, 5200)],
         improper((0, 0), 103, 100, (30, 25), ((1, 4750, 5250), (0, 1050, 1550)))),
    Edge("only mate A placed", [slot(50, 0, 1000)], [STATUS], improper((0, NO_SLOT), 50, 0, (30, 0), (NO_W, (0, 1050, 1550)))),
    Edge("only mate B placed", [STATUS], [STATUS, slot(50, 2, 3000)], improper((NO_SLOT, 1), 50, 0, (0, 25), ((2, 2550, 3050), NO_W))),
    Edge("none placed", [STATUS], [STATUS], NOTHING),
    Edge("status values in every slot", [(NONE, 0, 5, 7), (MALFORMED, 0, 0, 0), (TOO_WIDE, 0, 100, 1100), (TOO_LONG, 0, 100, 1100)],
         [(TOO_LONG, 0, 100, 1400), (TOO_WIDE, 0, 0, 0), (MALFORMED, 0, 0, 0), (NONE, NO_WINDOW, 0, 0)], NOTHING),
    Edge("minScore above every score", [slot(50, 0, 1000), slot(99, 0, 1000)], [slot(60, 0, 1200)], NOTHING, min_score=100),
    Edge("minScore at the score", [slot(50, 0, 1000), slot(100, 0, 1000)], [slot(100, 0, 1200)], proper((1, 0), 200, 0, 300, 60, (60, 60)),
         min_score=100),
    # read A's offsets are inverted: it has no counting slot and n_A = -50 in its window
    Edge("inverted read offsets", [slot(50, 0, 1000)], [slot(50, 0, 1000)], improper((NO_SLOT, 0), 50, 0, (0, 25), ((0, 550, 900), NO_W)),
         lengths=(-50, 100)),
    # B's window begins at -60 + 200 - 100 - 50 = -10; A's is [20 - 550, 20 - 50): both bounds become 0, and it still is a window
    Edge("window bounds raised to 0", [(50, 0, 100, 40)], [(50, 1, 100, 20)], improper((0, 0), 83, 0, (30, 25), ((1, 0, 0), (0, 0, 490)))),
    Edge("mappingQualities NULL, proper", [slot(50, 0, 1000), slot(50, 0, 1010)], [slot(40, 0, 1200)], proper((0, 0), 90, 90, 300, 0, (0, 0)),
         qualities=None),
    Edge("mappingQualities NULL, discordant", [slot(50, 0, 1000)], [slot(50, 1, 1200)],
         improper((0, 0), 83, 0, (0, 0), ((1, 750, 1250), (0, 1050, 1550))), qualities=None),
    Edge("mapqCap 0", [slot(50, 0, 1000)], [slot(40, 0, 1200)], proper((0, 0), 90, 0, 300, 0, (30, 25)), mapq_cap=0),
    Edge("mapqCap 254", [slot(50, 0, 1000)], [slot(40, 0, 1200)], proper((0, 0), 90, 0, 300, 254, (254, 254)), mapq_cap=254),
    # 254 (2^25 - 3) needs 33 bits; with the second (1 + 2^24 - 2) the quotient is 254 (2^24 - 2) / (2^25 - 3) = 126.99...
    Edge("scores near 2^24 without a second", [slot(BIG, 0, 1000)], [slot(BIG - 1, 0, 1200)],
         proper((0, 0), 2 * BIG - 1, 0, 300, 254, (254, 254)), mapq_cap=254),
    Edge("scores near 2^24 with a second", [slot(BIG, 0, 1000), slot(1, 0, 1010)], [slot(BIG - 1, 0, 1200)],
         proper((0, 0), 2 * BIG - 1, BIG, 300, 126, (126, 126)), mapq_cap=254),
]


def edge_cases(C=4):
    """the edges grouped by their params and by whether they give qualities: [(Case, [Edge])], every group one batch"""
    groups = {}
    for e in EDGES:
        groups.setdefault((tuple(sorted(e.params.items())), e.qualities is None), []).append(e)
    cases = []
    for (_, null), edges in groups.items():
        offsets, at = [3], 3
        slots = {name: [] for name in SLOT_INPUTS}
        for e in edges:
            for mate, length in zip((e.a, e.b), e.lengths):
                at += length
                offsets.append(at)
                padded = list(mate) + [STATUS] * (C - len(mate))
                slots["slotScores"].append([s[0] for s in padded])
                slots["sequences"].append([s[1] for s in padded])
                slots["slotReadEnds"].append([s[2] for s in padded])
                slots["slotTextEnds"].append([s[3] for s in padded])
        given = None if null else [q for e in edges for q in e.qualities]
        cases.append((Case(offsets, slots, given, dict(edges[0].params)), edges))
    return cases


def check_edges(got, edges, what=""):
    """the hand-computed values of a group of edges against the outputs of its batch"""
    proper_pairs = windows = 0
    for p, e in enumerate(edges):
        for name, value in e.want.items():
            if name in PAIR_OUTPUTS:
                assert int(got[name][p]) == value, (what, e.name, name, int(got[name][p]), value)
            elif name == "windows":
                for m in range(2):
                    have = tuple(int(got[k][2 * p + m]) for k in ("windowSequences", "windowBegins", "windowEnds"))
                    assert have == value[m], (what, e.name, "window of mate", m, have, value[m])
                    windows += value[m][0] != NO_WINDOW
            else:
                have = (int(got[name][2 * p]), int(got[name][2 * p + 1]))
                assert have == tuple(value), (what, e.name, name, have, value)
        proper_pairs += e.want["properPairs"]
    assert got["numProper"] == proper_pairs and got["numWindows"] == windows, (what, got["numProper"], got["numWindows"])


# ---- reverse complement ------------------------------------------------------------------------------------------------------
COMPLEMENT = {ord(x): ord(y) for x, y in zip("ACGTacgt", "TGCAtgca")}


def reverse_complement(chars, offsets, which, fill=0, num_read_chars=None):
    """byte by byte -> (out, malformed); what no well-formed read owns keeps `fill`"""
    chars = np.asarray(chars, np.uint8)
    limit = chars.size if num_read_chars is None else num_read_chars
    out, malformed = np.full(chars.size, fill, np.uint8), 0
    for r in range(len(offsets) - 1):
        begin, end = int(offsets[r]), int(offsets[r + 1])
        if begin > end or end > limit:
            malformed += 1
            continue
        n = end - begin
        selected = which == ALL or (which == ODD and r % 2 == 1) or (which == EVEN and r % 2 == 0)
        for i in range(n):
            if selected:
                c = int(chars[begin + n - 1 - i])
                out[begin + i] = COMPLEMENT.get(c, c)
            else:
                out[begin + i] = chars[begin + i]
    return out, malformed


def reads_buffer(seed, lengths, lead=0):
    """reads of these lengths back to back behind `lead` bytes no read owns: mixed case, ambiguity letters and other bytes among
    the letters -> (chars, offsets); the last read ends at the last byte"""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTacgtACGTacgtNnRYKMswbdhv-*\x00\xff", np.uint8)
    offsets = np.concatenate(([lead], lead + np.cumsum(np.asarray(lengths, np.int64)))).astype(np.uint64)
    chars = rng.choice(alphabet, int(offsets[-1])).astype(np.uint8)
    return chars, offsets


# ---- end to end: a FASTA file held on both strands, pairs as sequenced, the loop of the header ----
E2E = dict(pairs=96, length=100, fragment=400, min_insert=300, max_insert=500, window_pad=20, unpaired_penalty=17, min_score=30, mapq_cap=60,
           slots=4, band=2, min_votes=2, lookback=32, gap_penalty=2, max_ops=32, scoring=(1, 4, 6, 1), far=2000)
SWAP = {ord("a"): ord("c"), ord("c"): ord("g"), ord("g"): ord("t"), ord("t"): ord("a")}


def mirrored(sequence):
    return bytes(COMPLEMENT.get(c, c) for c in reversed(sequence))


class EndToEnd:
    """three records, each followed by its reverse complement, in a FASTA file; 96 pairs of an inward-facing library planted on
    either strand: mate 1 the first 100 characters of a fragment of 400, mate 2 AS SEQUENCED the reverse complement of its last
    100.  Every third pair's mate 2 carries a substitution at every 11th character (no seed of 14 fits between two: the seeds
    cannot place it); every sixteenth pair's mate 2 lies 2000 positions further on, outside the insert interval.  plan[p] =
    (record, position of mate 1, position of mate 2, kind) with kind "plain", "rescued" or "far".  The chains come from the host's
    own calls (tests/read_candidates_common.py, tests/read_chains_common.py) with three slots a read, in a table of stride four
    whose last column the window call gets."""

    def __init__(self, awfm, directory, seed=29):
        import read_candidates_common as rc
        import read_chains_common as ch
        import verify_chains_common as vc
        rng = np.random.default_rng(seed)
        letters = np.frombuffer(b"acgt", np.uint8)
        forward = [letters[rng.integers(0, 4, n)].tobytes() for n in (5000, 7001, 4003)]
        self.records = [r for f in forward for r in (f, mirrored(f))]
        self.fasta = os.path.join(str(directory), "strands.fa")
        with open(self.fasta, "wb") as f:
            for i, r in enumerate(self.records):
                f.write(b">r%d\n" % i + b"".join(r[j:j + 70] + b"\n" for j in range(0, len(r), 70)))
        n, F, far = E2E["length"], E2E["fragment"], E2E["far"]
        reads, self.plan = [], []
        for p in range(E2E["pairs"]):
            kind = "far" if p % 16 == 15 else "rescued" if p % 3 == 1 else "plain"
            s = int(rng.integers(0, len(self.records)))
            at = int(rng.integers(0, len(self.records[s]) - F - far))
            second = at + F - n + (far if kind == "far" else 0)
            mate = bytearray(self.records[s][second:second + n])
            if kind == "rescued":
                for k in range(5, n, 11):
                    mate[k] = SWAP[mate[k]]
            reads += [self.records[s][at:at + n], mirrored(bytes(mate))]
            self.plan.append((s, at, second, kind))
        self.sequenced = np.frombuffer(b"".join(reads), np.uint8)
        self.offsets = np.arange(2 * E2E["pairs"] + 1, dtype=np.uint64) * np.uint64(n)
        self.text, self.ends = vc.text_of(self.records)
        # call 1 on the host, then the chains of the reads on one strand
        self.chars, malformed = awfm.reverse_complement_reads_host(self.sequenced, self.offsets, ODD)
        assert malformed == 0
        same_strand = [bytes(self.chars[int(a):int(b)]) for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        self.ix = awfm.create_index_from_fasta(self.fasta, awfm.AwFmAlphabetDna, 8, 8, file_src=os.path.join(str(directory), "strands.awfmi"))
        inst = rc.host_pipeline(awfm, self.ix, same_strand)
        case = ch.candidate_case(awfm, inst, E2E["band"], E2E["slots"] - 1, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=E2E["min_votes"])
        got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=E2E["band"], lookback=E2E["lookback"], gap_penalty=E2E["gap_penalty"])
        narrow = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
        self.slots = {}
        for name in vc.SLOT_FIELDS:  # three columns of chains and a free one
            table = np.zeros((len(same_strand), E2E["slots"]), vc.SLOT_DTYPES[name])
            if name == "sequences":
                table[...] = NO_WINDOW
            table[:, :E2E["slots"] - 1] = narrow[name]
            self.slots[name] = table
        for p, (_, _, _, kind) in enumerate(self.plan):  # the seeds place every read but the rescued mates
            used = (self.slots["sequences"][2 * p + 1] != NO_WINDOW).any()
            assert used == (kind != "rescued"), (p, kind)
            assert (self.slots["sequences"][2 * p] != NO_WINDOW).any(), p

    def close(self):
        self.ix.dealloc()

    def loop(self, side):
        """chains -> slot scores -> pair -> window scores on the windows the pairing names -> slot scores -> pair -> affine
        alignment with pairSlots.  side: score(slots) -> dict, pair(slots, scored) -> dict, windows(first, slots) -> slots,
        align(slots, chosen) -> dict; returns (first pairing, second pairing, alignments)"""
        scored = side.score(self.slots)
        first = side.pair(self.slots, scored)
        slots = self.final_slots = side.windows(first, self.slots)
        scored = side.score(slots)
        second = side.pair(slots, scored)
        return first, second, side.align(slots, second["pairSlots"])

    def check(self, first, second, aligned):
        """every planted pair is found at its place: the condition on the inputs that the HOST twins meet"""
        n, F = E2E["length"], E2E["fragment"]
        for p, (s, at, mate_at, kind) in enumerate(self.plan):
            a, b = 2 * p, 2 * p + 1
            if kind == "far":  # not proper, before and after, and both reads got windows both times
                for pairing in (first, second):
                    assert pairing["properPairs"][p] == 0 and pairing["templateLengths"][p] == 0, (p, kind)
                    assert pairing["windowSequences"][a] == s and pairing["windowSequences"][b] == s, (p, kind)
                    assert int(pairing["windowBegins"][b]) == at + E2E["min_insert"] - n - E2E["window_pad"], (p, kind)
                    assert int(pairing["windowEnds"][b]) == at + E2E["max_insert"] + E2E["window_pad"], (p, kind)
                    assert int(pairing["windowEnds"][a]) == mate_at + n - E2E["min_insert"] + n + E2E["window_pad"], (p, kind)
            else:
                assert first["properPairs"][p] == (kind == "plain"), (p, kind)
                if kind == "rescued":  # the first pairing names the window, the window call fills the free column
                    assert first["pairSlots"][b] == NO_SLOT and first["windowSequences"][b] == s and first["windowSequences"][a] == NO_WINDOW
                    assert int(first["windowBegins"][b]) <= mate_at and mate_at + n <= int(first["windowEnds"][b]), p
                    assert second["pairSlots"][b] == E2E["slots"] - 1, p
                assert second["properPairs"][p] == 1 and int(second["templateLengths"][p]) == F, (p, kind, second["templateLengths"][p])
                assert second["windowSequences"][a] == NO_WINDOW and second["windowSequences"][b] == NO_WINDOW, p
                assert second["pairQualities"][p] == E2E["mapq_cap"] and second["mappingQualities"][a] == second["mappingQualities"][b] == E2E["mapq_cap"], p
            # affine alignment on pairSlots returns the planted intervals
            for r, where, clipped in ((a, at, 0), (b, mate_at, 5 if kind == "rescued" else 0)):
                assert 0 < int(aligned["scores"][r]) < TOO_LONG, (p, kind, r)
                assert int(aligned["readBegins"][r]) <= clipped and int(aligned["readEnds"][r]) >= n - clipped - (1 if clipped else 0), (p, kind, r)
                assert int(aligned["textBegins"][r]) == where + int(aligned["readBegins"][r]), (p, kind, r)
                assert int(aligned["textEnds"][r]) == where + int(aligned["readEnds"][r]), (p, kind, r)
        kinds = [k for _, _, _, k in self.plan]
        assert second["numProper"] == len(kinds) - kinds.count("far") and second["numWindows"] == 2 * kinds.count("far")
        assert first["numProper"] == kinds.count("plain") and first["numWindows"] == 2 * kinds.count("far") + kinds.count("rescued")


class HostSide:
    """the loop's four calls through the host twins"""

    def __init__(self, awfm, e2e):
        self.awfm, self.e = awfm, e2e
        self.common = dict(band_pad=8, max_drift=15, scoring=E2E["scoring"])

    def score(self, slots):
        return self.awfm.score_chains_affine_host(self.e.chars, self.e.offsets, slots, self.e.text, self.e.ends, min_score=E2E["min_score"],
                                                  mapq_cap=E2E["mapq_cap"], threads=16, **self.common)

    def pair(self, slots, scored):
        tables = dict({name: scored[name] for name in ("slotScores", "slotReadEnds", "slotTextEnds")}, sequences=slots["sequences"])
        return self.awfm.pair_mates_host(self.e.offsets, tables, E2E["min_insert"], E2E["max_insert"], mapping_qualities=scored["mappingQualities"],
                                         min_score=E2E["min_score"], unpaired_penalty=E2E["unpaired_penalty"], window_pad=E2E["window_pad"],
                                         mapq_cap=E2E["mapq_cap"], threads=16)

    def windows(self, pairing, slots):
        import verify_chains_common as vc
        got = self.awfm.score_windows_affine(self.e.chars, self.e.offsets, pairing["windowSequences"], pairing["windowBegins"], pairing["windowEnds"],
                                             self.e.text, self.e.ends, scoring=E2E["scoring"], min_score=E2E["min_score"], slots=slots,
                                             slot_stride=E2E["slots"], slot_column=E2E["slots"] - 1, threads=16)
        return {name: got[name] for name in vc.SLOT_FIELDS}

    def align(self, slots, chosen):
        return self.awfm.align_chains_affine_host(self.e.chars, self.e.offsets, slots, chosen, self.e.text, self.e.ends, max_ops=E2E["max_ops"],
                                                  threads=16, **self.common)
