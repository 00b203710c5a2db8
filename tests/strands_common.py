"""Strands (include/awfm_gpu.h "strands", csrc/awfm_strands.c) restated in plain Python loops for the tests of the host twins and
the device calls: every strand slot and every candidate (u1, u2) in turn, the header's rules in the header's order, Python
integers wrapped to 64-bit two's complement where the header says so; the orienting gather byte by byte; and cases: random slot
tables and the EDGE LIST, one pair an edge with hand-computed expectations (literals: the restatement is held to them as well).

The layout: R reads make 2R rows, row r the read as sequenced, row R + r its reverse complement; strand slot u = sigma * C + j is
slot j of row r + sigma * R."""
import numpy as np

NONE, MALFORMED, TOO_WIDE, TOO_LONG = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NO_SLOT = 0xFFFFFFFF     # AWFM_CHAINS_NO_SLOT
NO_WINDOW = 0xFFFFFFFF   # AWFM_CANDIDATES_NONE
SLOT_INPUTS = dict(sequences=np.uint32, slotScores=np.uint32, slotReadEnds=np.uint32, slotTextEnds=np.uint64)
READ_OUTPUTS = dict(strands=np.uint8, strandSlots=np.uint32, bestScores=np.uint32, secondScores=np.uint32, mappingQualities=np.uint8,
                    baseFlags=np.uint16)
ROW_OUTPUTS = dict(rowSlots=np.uint32, windowSequences=np.uint32, windowBegins=np.uint64, windowEnds=np.uint64)
PAIR_OUTPUTS = dict(properPairs=np.uint8, pairScores=np.uint32, pairSecondScores=np.uint32, templateLengths=np.int64, pairQualities=np.uint8)
COUNTERS = ("numReverse", "numProper", "numWindows", "numMalformed")
PARAMS = dict(min_insert=200, max_insert=500, min_score=0, unpaired_penalty=17, window_pad=50, mapq_cap=60)


def names(paired):
    return list(READ_OUTPUTS) + list(ROW_OUTPUTS) + (list(PAIR_OUTPUTS) if paired else []) + list(COUNTERS)


def dtypes():
    return dict(READ_OUTPUTS, **ROW_OUTPUTS, **PAIR_OUTPUTS)


def wrap(x):
    """x as a 64-bit two's complement number"""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


class Case:
    """offsets uint64[2R + 1], slots: the four arrays shaped (2R, C), params: the keyword arguments of choose_strands_host"""

    def __init__(self, offsets, slots, params):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.slots = {name: np.ascontiguousarray(slots[name], dtype=dtype) for name, dtype in SLOT_INPUTS.items()}
        self.params = dict(PARAMS, **params)
        self.num_rows = self.offsets.size - 1
        self.num_reads = self.num_rows // 2
        self.C = self.slots["sequences"].shape[1]

    def host(self, awfm, paired, **kw):
        return awfm.choose_strands_host(self.offsets, self.slots, paired=paired, **dict(self.params, **kw))

    def expected(self, paired, before=None):
        return expected(self, paired, before)


def read_rules(case, r):
    """rules 1 to 5 for read r -> dict(malformed, n, slots [2C], best u or None, bestScore, secondScore, quality)"""
    q, C, R = case.params, case.C, case.num_reads
    floor = max(q["min_score"], 1)
    f0, f1, v0, v1 = (int(case.offsets[i]) for i in (r, r + 1, R + r, R + r + 1))
    malformed = f0 > f1 or v0 > v1 or f1 - f0 != v1 - v0
    slots = []
    for u in range(2 * C):
        row, j = r + (u // C) * R, u % C
        score, sequence = int(case.slots["slotScores"][row, j]), int(case.slots["sequences"][row, j])
        read_end, text_end = int(case.slots["slotReadEnds"][row, j]), int(case.slots["slotTextEnds"][row, j])
        counts = (not malformed) and score < TOO_LONG and score >= floor
        slots.append(dict(counts=counts, score=score, sequence=sequence, end=(read_end, text_end), start=wrap(text_end - read_end), strand=u // C))
    best = None
    for u in range(2 * C):
        if slots[u]["counts"] and (best is None or slots[u]["score"] > slots[best]["score"]):
            best = u
    second = 0
    if best is not None:
        for u in range(2 * C):
            if slots[u]["counts"] and not same(slots, u, best):
                second = max(second, slots[u]["score"])
    best_score = 0 if best is None else slots[best]["score"]
    quality = 0 if best is None else q["mapq_cap"] * (best_score - second) // best_score
    return dict(malformed=malformed, n=wrap(f1 - f0), slots=slots, best=best, bestScore=best_score, secondScore=second, quality=quality)


def same(slots, u, v):
    """rule 3, and a strand slot is the same as itself"""
    x, y = slots[u], slots[v]
    return u == v or (x["strand"] == y["strand"] and x["counts"] and y["counts"] and x["sequence"] == y["sequence"] and x["end"] == y["end"])


def expected(case, paired, before=None):
    """the header's rules, read by read or pair by pair"""
    q, C, R = case.params, case.C, case.num_reads
    out = {name: np.zeros(R, dtype) for name, dtype in READ_OUTPUTS.items()}
    out.update({name: np.zeros(2 * R, dtype) for name, dtype in ROW_OUTPUTS.items()})
    if paired:
        out.update({name: np.zeros(R // 2, dtype) for name, dtype in PAIR_OUTPUTS.items()})
    counters = dict.fromkeys(COUNTERS, 0)
    counters.update(before or {})

    def store(r, read, chosen, quality, window):
        strand, slot = (0, NO_SLOT) if chosen is None else (chosen // C, chosen % C)
        counters["numReverse"] += strand
        counters["numMalformed"] += int(read["malformed"])
        out["strands"][r], out["strandSlots"][r], out["baseFlags"][r] = strand, slot, 0x10 if strand else 0
        out["bestScores"][r], out["secondScores"][r], out["mappingQualities"][r] = read["bestScore"], read["secondScore"], quality
        for sigma in range(2):
            row = sigma * R + r
            out["rowSlots"][row] = slot if chosen is not None and strand == sigma else NO_SLOT
            here = window is not None and window[0] == sigma
            out["windowSequences"][row] = window[1] if here else NO_WINDOW
            out["windowBegins"][row] = window[2] if here else 0
            out["windowEnds"][row] = window[3] if here else 0
        counters["numWindows"] += window is not None

    if not paired:
        for r in range(R):
            read = read_rules(case, r)
            store(r, read, read["best"], read["quality"], None)
        out.update(counters)
        return out
    for p in range(R // 2):
        reads = [read_rules(case, 2 * p), read_rules(case, 2 * p + 1)]
        candidates = []  # (value, concordant, u1, u2, T)
        for u1 in range(2 * C):
            for u2 in range(2 * C):
                x, y = reads[0]["slots"][u1], reads[1]["slots"][u2]
                if not (x["counts"] and y["counts"]):
                    continue
                concordant, T = False, 0
                if x["strand"] != y["strand"]:
                    A, B, n_B = (x, y, reads[1]["n"]) if x["strand"] == 0 else (y, x, reads[0]["n"])
                    T = wrap(B["start"] + n_B - A["start"])
                    concordant = x["sequence"] == y["sequence"] and q["min_insert"] <= T <= q["max_insert"]
                if concordant:
                    candidates.append((x["score"] + y["score"], True, u1, u2, T))
                elif u1 == reads[0]["best"] and u2 == reads[1]["best"]:
                    candidates.append((max(0, x["score"] + y["score"] - q["unpaired_penalty"]), False, u1, u2, 0))
        winner = None
        for k in candidates:  # the largest value, then the concordant one, then the lowest u1, then the lowest u2
            if winner is None or (k[0], k[1], -k[2], -k[3]) > (winner[0], winner[1], -winner[2], -winner[3]):
                winner = k
        second = 0
        for k in candidates:
            if same(reads[0]["slots"], k[2], winner[2]) and same(reads[1]["slots"], k[3], winner[3]):
                continue
            second = max(second, k[0])
        is_proper = winner is not None and winner[1]
        chosen = [reads[0]["best"], reads[1]["best"]]
        value = 0
        if winner is not None:
            chosen, value = [winner[2], winner[3]], winner[0]
        elif chosen[0] is not None:
            value = reads[0]["bestScore"]
        elif chosen[1] is not None:
            value = reads[1]["bestScore"]
        quality = q["mapq_cap"] * (winner[0] - second) // winner[0] if is_proper else 0
        counters["numProper"] += int(is_proper)
        out["properPairs"][p] = int(is_proper)
        out["pairScores"][p] = value & 0xFFFFFFFF
        out["pairSecondScores"][p] = second & 0xFFFFFFFF
        out["templateLengths"][p] = winner[4] if is_proper else 0
        out["pairQualities"][p] = quality
        for m in range(2):
            mine, mate = reads[m], reads[1 - m]
            mapq = mine["quality"]
            if is_proper:
                mapq = max(quality, mine["quality"] if chosen[m] == mine["best"] else 0)
            window = None
            if not is_proper and mate["best"] is not None:
                s = mate["slots"][mate["best"]]
                pad, S = q["window_pad"], s["start"]
                if s["strand"] == 0:
                    window = (1, s["sequence"], max(wrap(S + q["min_insert"] - mine["n"] - pad), 0), max(wrap(S + q["max_insert"] + pad), 0))
                else:
                    E = wrap(S + mate["n"])
                    window = (0, s["sequence"], max(wrap(E - q["max_insert"] - pad), 0), max(wrap(E - q["min_insert"] + mine["n"] + pad), 0))
            store(2 * p + m, mine, chosen[m], mapq, window)
    out.update(counters)
    return out


def assert_equal(got, want, names_, what=""):
    for name in names_:
        if name in COUNTERS:
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            g, w = np.asarray(got[name]), np.asarray(want[name])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
            if not np.array_equal(g, w):
                at = int(np.argwhere(g != w)[0][0])
                raise AssertionError(f"{what}: {name}[{at}] is {g[at]}, expected {w[at]} ({(g != w).sum()} differ)")


def random_case(seed, reads, C, params=None, big=False, unique_sums=False):
    """slot tables as slot scores might write them on 2R rows, made to collide: a few sequences, a fragment per pair of reads with
    mate 1 on a random strand and mate 2 on the other (starts on a coarse grid around it, so that many candidates are concordant
    and tie), decoys on the wrong strand, scores from a small range, a fifth of the slots a status, duplicates on one strand and
    the same end cell on the other, some reads malformed (inverted offsets, or rows of two lengths); big: scores just below 2^24;
    unique_sums: every score of a mate 1 is a multiple of 64 and every score of a mate 2 below 64 and all of a read's differ, so
    that no two candidates of a pair tie"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 200, reads).astype(np.int64)
    kind = rng.random(reads)
    forward = np.where(kind < 0.03, -rng.integers(1, 50, reads), lengths)
    reverse = np.where((kind >= 0.03) & (kind < 0.06), lengths + rng.integers(1, 5, reads), np.where((kind >= 0.06) & (kind < 0.08), -3, lengths))
    offsets = np.concatenate(([1000], 1000 + np.cumsum(np.concatenate((forward, reverse))))).astype(np.uint64)
    slots = {name: np.zeros((2 * reads, C), dtype) for name, dtype in SLOT_INPUTS.items()}
    for p in range((reads + 1) // 2):
        fragment, first_strand = int(rng.integers(0, 3000)), int(rng.integers(0, 2))
        for m in range(2):
            r = 2 * p + m
            if r >= reads:
                break
            pool = list(rng.permutation(60) + 1) if unique_sums else None
            for sigma in range(2):
                row = r + sigma * reads
                for j in range(C):
                    roll = rng.random()
                    if roll < 0.2:
                        slots["slotScores"][row, j] = int(rng.choice([NONE, MALFORMED, TOO_WIDE, TOO_LONG]))
                        slots["sequences"][row, j] = NO_WINDOW if rng.random() < 0.5 else int(rng.integers(0, 3))
                        continue
                    if roll < 0.3 and j > 0:  # the slot before once more: a duplicate when that one counts
                        for name in slots:
                            slots[name][row, j] = slots[name][row, j - 1]
                        if rng.random() < 0.3 and not unique_sums:
                            slots["slotScores"][row, j] = int(rng.integers(0, 12))
                        continue
                    if roll < 0.4 and sigma == 1:  # the other strand's end cell once more: never a duplicate
                        for name in slots:
                            slots[name][row, j] = slots[name][r, j]
                        if unique_sums and slots["slotScores"][row, j] < TOO_LONG:
                            slots["slotScores"][row, j] = int(pool.pop()) * (64 if m == 0 else 1)
                        continue
                    score = int(rng.integers(0, 12)) + ((1 << 24) - 12 if big and rng.random() < 0.7 else 0)
                    if unique_sums:
                        score = int(pool.pop()) * (64 if m == 0 else 1)
                    read_end = int(rng.integers(0, 200))
                    on_fragment = (sigma == first_strand) == (m == 0)  # this read's strand in the fragment
                    upstream = sigma == 0  # the read on strand 0 starts the fragment
                    start = fragment + (0 if upstream else 190) + 10 * int(rng.integers(-3, 4)) - (0 if on_fragment or rng.random() < 0.5 else 3000)
                    slots["slotScores"][row, j] = score
                    slots["sequences"][row, j] = int(rng.integers(0, 2))
                    slots["slotReadEnds"][row, j] = read_end
                    slots["slotTextEnds"][row, j] = max(start + read_end, 0)
    return Case(offsets, slots, params or {})


# ---- the edge list ----------------------------------------------------------------------------------------------------------
def slot(score, sequence, start, read_end=100):
    """(score, sequence, readEnd, textEnd) of a slot whose START is `start`"""
    return (score, sequence, read_end, start + read_end)


STATUS = (NONE, NO_WINDOW, 0, 0)
F, V = 0, 1  # strands, for (strand, slot) and for the row a window is on


class Edge:
    """one pair: the slots of m1 as sequenced (f1) and reverse-complemented (v1), likewise of m2; the lengths of the two reads and
    of their reverse rows (a negative length: inverted offsets); params; and the hand-computed outputs.
    reads: per read (best (strand, slot) or None, bestScore, secondScore, q_r) -- rules 1 to 5, what the unpaired call returns.
    pair: dict(proper, chosen ((strand, slot) or None per read), score, second, T, quality, mapq per read, windows per read:
    (row strand, sequence, begin, end) or None) -- what the paired call returns."""

    def __init__(self, name, f1, v1, f2, v2, reads, pair, lengths=(100, 100), reverse_lengths=None, malformed=0, **params):
        self.name, self.f1, self.v1, self.f2, self.v2, self.reads, self.pair = name, f1, v1, f2, v2, reads, pair
        self.lengths, self.reverse_lengths, self.malformed, self.params = lengths, reverse_lengths or lengths, malformed, params


def proper(chosen, score, second, T, quality, mapq):
    return dict(proper=1, chosen=chosen, score=score, second=second, T=T, quality=quality, mapq=mapq, windows=(None, None))


def improper(chosen, score, second, mapq, windows):
    return dict(proper=0, chosen=chosen, score=score, second=second, T=0, quality=0, mapq=mapq, windows=windows)


UNPLACED = (None, 0, 0, 0)
EDGES = [
    # 50 on both strands: the forward one is the best, the other the second, so q = 0; m2 has nothing, gets a window from m1's
    # best (strand 0, S = 1000): row V(m2), [1000 + 200 - 100 - 50, 1000 + 500 + 50)
    Edge("a tie between strands goes to strand 0", [slot(50, 0, 1000)], [slot(50, 0, 3000)], [STATUS], [STATUS],
         (((F, 0), 50, 50, 0), UNPLACED), improper(((F, 0), None), 50, 0, (0, 0), (None, (V, 0, 1050, 1550)))),
    # forward slot 1 is slot 0 once more and is skipped; the same end cell on the reverse strand is not: the second is 40, not 30;
    # q = 60 * 10 // 50
    Edge("a duplicate on one strand is skipped, the same end cell on the other strand is not",
         [slot(50, 0, 1000), slot(50, 0, 1000), slot(30, 0, 1020)], [slot(40, 0, 1000)], [STATUS], [STATUS],
         (((F, 0), 50, 40, 12), UNPLACED), improper(((F, 0), None), 50, 0, (12, 0), (None, (V, 0, 1050, 1550)))),
    # q = 60 * 15 // 60; only m1 placed, on the reverse strand: m2's window is on row F(m2), E = 2000 + 100:
    # [2100 - 500 - 50, 2100 - 200 + 100 + 50)
    Edge("the best on the reverse strand, the second on the other", [slot(45, 1, 1000)], [STATUS, slot(60, 0, 2000)], [STATUS], [STATUS],
         (((V, 1), 60, 45, 15), UNPLACED), improper(((V, 1), None), 60, 0, (15, 0), (None, (F, 0, 1550, 2050)))),
    # m1 on strand 0 at 1000, m2 on strand 1 at 1200: T = 1200 + 100 - 1000
    Edge("concordant, m1 forward and m2 reverse", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(40, 0, 1200)],
         (((F, 0), 50, 0, 60), ((V, 0), 40, 0, 60)), proper(((F, 0), (V, 0)), 90, 0, 300, 60, (60, 60))),
    # the fragment's other strand: m2 is A (strand 0, 1000), m1 is B (strand 1, 1200): T = 1200 + n_m1 - 1000
    Edge("concordant, m1 reverse and m2 forward", [STATUS], [slot(50, 0, 1200)], [slot(40, 0, 1000)], [STATUS],
         (((V, 0), 50, 0, 60), ((F, 0), 40, 0, 60)), proper(((V, 0), (F, 0)), 90, 0, 300, 60, (60, 60))),
    # n_B is the length of the read on strand 1: 80 here (m1), not 120
    Edge("T takes the length of the read on strand 1", [STATUS], [slot(50, 0, 1200, 80)], [slot(40, 0, 1000, 120)], [STATUS],
         (((V, 0), 50, 0, 60), ((F, 0), 40, 0, 60)), proper(((V, 0), (F, 0)), 90, 0, 280, 60, (60, 60)), lengths=(80, 120)),
    # (v1, f2) is concordant with 43 + 60 (A = f2 at 5000, B = v1 at 5200); the bests (f1, f2) lie on one strand: discordant with
    # 60 + 60 - 17.  The concordant one goes first; the other is no duplicate (u1 differs in strand), so the second is 103; m1 is
    # not placed at its best, so its own quality (60 * 17 // 60) does not count
    Edge("a concordant and a discordant candidate of equal value", [slot(60, 0, 1000)], [slot(43, 1, 5200)], [slot(60, 1, 5000)], [STATUS],
         (((F, 0), 60, 43, 17), ((F, 0), 60, 0, 60)), proper(((V, 0), (F, 0)), 103, 103, 300, 0, (0, 60))),
    # four candidates of value 90 in one orientation: the lowest u1, then the lowest u2
    Edge("u1 and u2 tie order within an orientation", [slot(50, 0, 1000), slot(50, 0, 1010)], [STATUS], [STATUS],
         [slot(40, 0, 1200), slot(40, 0, 1210)],
         (((F, 0), 50, 50, 0), ((V, 0), 40, 40, 0)), proper(((F, 0), (V, 0)), 90, 90, 300, 0, (0, 0))),
    # one candidate of value 90 in each orientation: u1 on strand 0 is the lower one; m2's best is its forward slot, so m2 is not
    # placed at its best
    Edge("u1 tie order between the orientations", [slot(50, 0, 1000)], [slot(50, 0, 1200)], [slot(40, 0, 1000)], [slot(40, 0, 1200)],
         (((F, 0), 50, 50, 0), ((F, 0), 40, 40, 0)), proper(((F, 0), (V, 0)), 90, 90, 300, 0, (0, 0))),
    # T would be 300 if the strands differed.  Discordant: 100 - 17.  Both bests on strand 0: both windows on the V rows,
    # [1200 + 200 - 100 - 50, 1200 + 550) and [1000 + 50, 1000 + 550)
    Edge("bests on one strand are never concordant", [slot(50, 0, 1000)], [STATUS], [slot(50, 0, 1200)], [STATUS],
         (((F, 0), 50, 0, 60), ((F, 0), 50, 0, 60)),
         improper(((F, 0), (F, 0)), 83, 0, (60, 60), ((V, 0, 1250, 1750), (V, 0, 1050, 1550)))),
    Edge("T at minInsert", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(50, 0, 1100)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)), proper(((F, 0), (V, 0)), 100, 0, 200, 60, (60, 60))),
    Edge("T at maxInsert", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(50, 0, 1400)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)), proper(((F, 0), (V, 0)), 100, 0, 500, 60, (60, 60))),
    # m1's window from m2's best on strand 1: E = 1099 + 100, row F(m1), [1199 - 550, 1199 - 200 + 150); m2's from m1's on strand 0
    Edge("T one below minInsert", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(50, 0, 1099)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)),
         improper(((F, 0), (V, 0)), 83, 0, (60, 60), ((F, 0, 649, 1149), (V, 0, 1050, 1550)))),
    Edge("T one above maxInsert", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(50, 0, 1401)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)),
         improper(((F, 0), (V, 0)), 83, 0, (60, 60), ((F, 0, 951, 1451), (V, 0, 1050, 1550)))),
    # an RF library is a negative interval: B lies before A
    Edge("a negative interval", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(50, 0, 700)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)), proper(((F, 0), (V, 0)), 100, 0, -200, 60, (60, 60)), min_insert=-300, max_insert=-100),
    # S(A) = 60 - 100 = -40: T = 200 + 100 + 40
    Edge("a negative start", [(50, 0, 100, 60)], [STATUS], [STATUS], [slot(50, 0, 200)],
         (((F, 0), 50, 0, 60), ((V, 0), 50, 0, 60)), proper(((F, 0), (V, 0)), 100, 0, 340, 60, (60, 60))),
    Edge("none placed", [STATUS], [STATUS], [STATUS], [STATUS], (UNPLACED, UNPLACED), improper((None, None), 0, 0, (0, 0), (None, None))),
    # m1's S = -60, m2's S = -80, both on strand 0: V(m1) gets [-80 + 200 - 100 - 50, -80 + 550), V(m2) [-60 + 50, -60 + 550)
    Edge("window bounds raised to 0, mates on strand 0", [(50, 0, 100, 40)], [STATUS], [(50, 1, 100, 20)], [STATUS],
         (((F, 0), 50, 0, 60), ((F, 0), 50, 0, 60)), improper(((F, 0), (F, 0)), 83, 0, (60, 60), ((V, 1, 0, 470), (V, 0, 0, 490)))),
    # m1 on strand 1 with S = -60: E = 40, F(m2) gets [40 - 550, 40 - 200 + 150): both bounds become 0, and it still is a window
    Edge("window bounds raised to 0, the mate on strand 1", [STATUS], [(50, 3, 100, 40)], [STATUS], [STATUS],
         (((V, 0), 50, 0, 60), UNPLACED), improper(((V, 0), None), 50, 0, (60, 0), (None, (F, 3, 0, 0)))),
    # m1's reverse row is 90 long, its forward row 100: no strand slot of m1 counts; its window takes n = 100
    Edge("a malformed read: rows of two lengths", [slot(70, 0, 1000)], [slot(70, 0, 1000)], [slot(50, 0, 1000)], [STATUS],
         (UNPLACED, ((F, 0), 50, 0, 60)), improper((None, (F, 0)), 50, 0, (0, 60), ((V, 0, 1050, 1550), None)),
         reverse_lengths=(90, 100), malformed=1),
    # m1's forward offsets are inverted: n = -50 in its window, [1000 + 200 + 50 - 50, 1550)
    Edge("a malformed read: inverted offsets", [slot(70, 0, 1000)], [slot(70, 0, 1000)], [slot(50, 0, 1000)], [STATUS],
         (UNPLACED, ((F, 0), 50, 0, 60)), improper((None, (F, 0)), 50, 0, (0, 60), ((V, 0, 1200, 1550), None)),
         lengths=(-50, 100), malformed=1),
    Edge("status values in every slot", [(NONE, 0, 5, 7), (MALFORMED, 0, 0, 0)], [(TOO_WIDE, 0, 100, 1100), (TOO_LONG, 0, 100, 1100)],
         [(TOO_LONG, 0, 100, 1400), (TOO_WIDE, 0, 0, 0)], [(MALFORMED, 0, 0, 0), (NONE, NO_WINDOW, 0, 0)],
         (UNPLACED, UNPLACED), improper((None, None), 0, 0, (0, 0), (None, None))),
    # a status among scores: it neither is the best (it is the largest number) nor the second
    Edge("a score with a status value", [(TOO_LONG, 0, 100, 1100), slot(50, 0, 1000)], [(NONE, 0, 100, 1100)], [STATUS],
         [(MALFORMED, 0, 100, 1300), slot(40, 0, 1200)],
         (((F, 1), 50, 0, 60), ((V, 1), 40, 0, 60)), proper(((F, 1), (V, 1)), 90, 0, 300, 60, (60, 60))),
    Edge("minScore above every score", [slot(50, 0, 1000)], [slot(99, 0, 1000)], [slot(60, 0, 1200)], [STATUS],
         (UNPLACED, UNPLACED), improper((None, None), 0, 0, (0, 0), (None, None)), min_score=100),
    Edge("mapqCap 0", [slot(50, 0, 1000)], [STATUS], [STATUS], [slot(40, 0, 1200)],
         (((F, 0), 50, 0, 0), ((V, 0), 40, 0, 0)), proper(((F, 0), (V, 0)), 90, 0, 300, 0, (0, 0)), mapq_cap=0),
    # q of m1: 254 * 20 // 50 = 101; the pair has no second
    Edge("mapqCap 254", [slot(50, 0, 1000)], [slot(30, 0, 7000)], [STATUS], [slot(40, 0, 1200)],
         (((F, 0), 50, 30, 101), ((V, 0), 40, 0, 254)), proper(((F, 0), (V, 0)), 90, 0, 300, 254, (254, 254)), mapq_cap=254),
]


def edge_cases(C=4):
    """the edges grouped by their params: [(Case, [Edge])], every group one batch of 2 R rows"""
    groups = {}
    for e in EDGES:
        groups.setdefault(tuple(sorted(e.params.items())), []).append(e)
    cases = []
    for edges in groups.values():
        lengths = [n for e in edges for n in e.lengths] + [n for e in edges for n in e.reverse_lengths]
        offsets = np.concatenate(([3], 3 + np.cumsum(np.asarray(lengths, np.int64))))
        slots = {name: [] for name in SLOT_INPUTS}
        for mates in ([m for e in edges for m in (e.f1, e.f2)], [m for e in edges for m in (e.v1, e.v2)]):
            for mate in mates:
                padded = list(mate) + [STATUS] * (C - len(mate))
                slots["slotScores"].append([s[0] for s in padded])
                slots["sequences"].append([s[1] for s in padded])
                slots["slotReadEnds"].append([s[2] for s in padded])
                slots["slotTextEnds"].append([s[3] for s in padded])
        cases.append((Case(offsets.astype(np.uint64), slots, dict(edges[0].params)), edges))
    return cases


def check_edges(got, edges, paired, what=""):
    """the hand-computed values of a group of edges against the outputs of its batch (the counters: this call's own)"""
    R = 2 * len(edges)
    tally = dict.fromkeys(COUNTERS, 0)
    for p, e in enumerate(edges):
        for m in range(2):
            r = 2 * p + m
            best, best_score, second_score, quality = e.reads[m]
            chosen, mapq, window = (e.pair["chosen"][m], e.pair["mapq"][m], e.pair["windows"][m]) if paired else (best, quality, None)
            strand, j = (0, NO_SLOT) if chosen is None else chosen
            have = tuple(int(got[k][r]) for k in ("strands", "strandSlots", "baseFlags", "bestScores", "secondScores", "mappingQualities"))
            assert have == (strand, j, 0x10 * strand, best_score, second_score, mapq), (what, e.name, "read", m, have)
            for sigma in range(2):
                row = sigma * R + r
                have = tuple(int(got[k][row]) for k in ("rowSlots", "windowSequences", "windowBegins", "windowEnds"))
                want = (j if chosen is not None and strand == sigma else NO_SLOT,) + (tuple(window[1:]) if window and window[0] == sigma else (NO_WINDOW, 0, 0))
                assert have == want, (what, e.name, "row", sigma, "of read", m, have, want)
            tally["numReverse"] += strand
            tally["numWindows"] += window is not None
        tally["numMalformed"] += e.malformed
        if paired:
            have = tuple(int(got[k][p]) for k in ("properPairs", "pairScores", "pairSecondScores", "templateLengths", "pairQualities"))
            assert have == tuple(e.pair[k] for k in ("proper", "score", "second", "T", "quality")), (what, e.name, have)
            tally["numProper"] += e.pair["proper"]
    assert {k: got[k] for k in COUNTERS} == tally, (what, {k: got[k] for k in COUNTERS}, tally)


# ---- orient -------------------------------------------------------------------------------------------------------------------
SLOT_COLUMNS = dict(sequences=np.uint32, chainAnchors=np.uint32, chainReadBegins=np.uint32, chainReadEnds=np.uint32,
                    chainBeginDiagonals=np.int64, chainEndDiagonals=np.int64, slotScores=np.uint32, slotReadEnds=np.uint32, slotTextEnds=np.uint64)
UNUSED = dict(sequences=NO_WINDOW, slotScores=NONE)  # what a malformed read's columns get; every other column 0
ORIENT_LENGTHS = list(range(10)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 300]


def orient_expected(chars, offsets, strands, columns=None, qualities=None, capacity=None, fill=0, num_read_chars=None, malformed_before=0):
    """byte by byte and column by column -> the dict orient_reads_host returns; what no well-formed read owns keeps `fill`"""
    chars, offsets = np.asarray(chars, np.uint8), [int(o) for o in offsets]
    R = (len(offsets) - 1) // 2
    limit = chars.size if num_read_chars is None else num_read_chars
    if capacity is None:
        capacity = offsets[R] - offsets[0] if offsets[R] >= offsets[0] else 0
    out = dict(readChars=np.full(capacity, fill, np.uint8), readOffsets=np.zeros(R + 1, np.uint64))
    if qualities is not None:
        out["qualities"] = np.full(capacity, fill, np.uint8)
    for name, a in (columns or {}).items():
        out[name] = np.zeros((R, np.asarray(a).shape[1]), SLOT_COLUMNS[name])
    malformed = malformed_before
    for r in range(R + 1):
        out["readOffsets"][r] = (offsets[r] - offsets[0]) & ((1 << 64) - 1)
    for r in range(R):
        f0, f1, v0, v1, s = offsets[r], offsets[r + 1], offsets[R + r], offsets[R + r + 1], int(strands[r])
        good = f0 <= f1 <= limit and v0 <= v1 <= limit and f1 - f0 == v1 - v0 and s <= 1 and f0 >= offsets[0] and f1 - offsets[0] <= capacity
        if not good:
            malformed += 1
            for name in columns or {}:
                out[name][r, :] = UNUSED.get(name, 0)
            continue
        n, to, source = f1 - f0, f0 - offsets[0], v0 if s else f0
        for i in range(n):
            out["readChars"][to + i] = chars[source + i]
            if qualities is not None:
                out["qualities"][to + i] = qualities[f0 + (n - 1 - i if s else i)]
        for name, a in (columns or {}).items():
            out[name][r, :] = np.asarray(a)[r + s * R, :]
    out["numMalformed"] = malformed
    return out


def orient_case(seed, lengths, lead=0, C=4, tail=0):
    """2R rows of these lengths (the forward rows, then the reverse rows) behind `lead` bytes no read owns and before `tail` more:
    random bytes, random strands, random columns and qualities -> dict(chars, offsets, strands, columns, qualities)"""
    rng = np.random.default_rng(seed)
    both = np.concatenate((np.asarray(lengths, np.int64), np.asarray(lengths, np.int64)))
    offsets = np.concatenate(([lead], lead + np.cumsum(both))).astype(np.uint64)
    size = int(offsets[-1]) + tail
    columns = {name: rng.integers(0, 1 << 31, (2 * len(lengths), C)).astype(dtype) for name, dtype in SLOT_COLUMNS.items()}
    return dict(chars=rng.integers(0, 256, size).astype(np.uint8), offsets=offsets, strands=rng.integers(0, 2, len(lengths)).astype(np.uint8),
                columns=columns, qualities=rng.integers(33, 127, size).astype(np.uint8))


def orient_order():
    """every length of ORIENT_LENGTHS four times, each behind a read of 0 to 3 characters that brings it to the next destination
    offset mod 4"""
    order, at = [], 0
    for d in range(4):
        for n in ORIENT_LENGTHS:
            filler = (d - at) % 4
            order += [filler, n]
            at += filler + n
    return order


def orient_alignments(case, order):
    """{(length, strand, source offset mod 4, destination offset mod 4)} of the reads of a case"""
    R, o = len(order), case["offsets"].astype(np.int64)
    return {(n, int(case["strands"][r]), int(o[(R if case["strands"][r] else 0) + r]) % 4, int(o[r] - o[0]) % 4) for r, n in enumerate(order)}


def assert_orient_equal(got, want, what=""):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for name in want:
        if name == "numMalformed":
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            g, w = np.asarray(got[name]), np.asarray(want[name])
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


# ---- end to end: a FASTA file indexed on ONE strand, FR pairs planted on both strands, the loop of the header ----
E2E = dict(pairs=96, length=100, fragment=400, min_insert=300, max_insert=500, window_pad=20, unpaired_penalty=17, min_score=30, mapq_cap=60,
           slots=4, band=2, min_votes=2, lookback=32, gap_penalty=2, max_ops=32, scoring=(1, 4, 6, 1), far=2000, seed=29)
E2E_COMMON = dict(band_pad=8, max_drift=15, scoring=E2E["scoring"])
COMPLEMENT = {ord(x): ord(y) for x, y in zip("ACGTacgt", "TGCAtgca")}
SWAP = {ord("a"): ord("c"), ord("c"): ord("g"), ord("g"): ord("t"), ord("t"): ord("a")}


def mirrored(sequence):
    return bytes(COMPLEMENT.get(c, c) for c in reversed(sequence))


class EndToEnd:
    """three records of random text, 20 kbp in all, in a FASTA file indexed as it is: ONE strand.  96 pairs of an inward-facing
    library, fragments of 400: the LEFT read is the fragment's first 100 characters as they stand in the text, the RIGHT read
    the reverse complement of its last 100.  Pairs with even p come from the forward strand (m1 left, m2 right), odd ones from
    the reverse strand (m1 right, m2 left).  Every read carries one substitution (at 37) -- a few, as sequenced reads do --; every
    third pair's m2 one at every 11th character on top (no seed of 14 fits between two: the seeds cannot place it on either
    strand, "rescued"); every sixteenth pair's right read lies 2000 positions further on, outside the insert interval ("far").
    plan[p] = dict(record, strands of m1 and m2, text positions of m1 and m2, kind).  The chains of the 2R rows come from the
    host's own calls (tests/read_candidates_common.py, tests/read_chains_common.py) with three slots a row, in a table of stride
    four whose last column the window call gets."""

    def __init__(self, awfm, directory, seed=E2E["seed"]):
        import os
        import read_candidates_common as rc
        import read_chains_common as ch
        import verify_chains_common as vc
        rng = np.random.default_rng(seed)
        letters = np.frombuffer(b"acgt", np.uint8)
        self.records = [letters[rng.integers(0, 4, n)].tobytes() for n in (7000, 8001, 4999)]
        self.fasta = os.path.join(str(directory), "one_strand.fa")
        with open(self.fasta, "wb") as f:
            for i, r in enumerate(self.records):
                f.write(b">r%d one strand\n" % i + b"".join(r[j:j + 70] + b"\n" for j in range(0, len(r), 70)))
        n, F, far = E2E["length"], E2E["fragment"], E2E["far"]
        reads, self.plan = [], []
        for p in range(E2E["pairs"]):
            kind = "far" if p % 16 == 15 else "rescued" if p % 3 == 1 else "plain"
            s = int(rng.integers(0, len(self.records)))
            at = int(rng.integers(0, len(self.records[s]) - F - far))
            right_at = at + F - n + (far if kind == "far" else 0)
            left, right = bytearray(self.records[s][at:at + n]), bytearray(self.records[s][right_at:right_at + n])
            forward = p % 2 == 0
            for segment, second in ((left, not forward), (right, forward)):
                segment[37] = SWAP[segment[37]]
                if kind == "rescued" and second:  # m2, as it stands in the text
                    for k in range(5, n, 11):
                        segment[k] = SWAP[segment[k]]
            reads += [bytes(left), mirrored(bytes(right))] if forward else [mirrored(bytes(right)), bytes(left)]
            self.plan.append(dict(record=s, strands=(0, 1) if forward else (1, 0), at=(at, right_at) if forward else (right_at, at), kind=kind))
        self.R, self.size = 2 * E2E["pairs"], 2 * E2E["pairs"] * n
        self.sequenced = np.frombuffer(b"".join(reads), np.uint8)
        self.read_offsets = np.arange(self.R + 1, dtype=np.uint64) * np.uint64(n)
        self.offsets = np.arange(2 * self.R + 1, dtype=np.uint64) * np.uint64(n)  # of the 2R rows
        self.qualities = np.concatenate((rng.integers(35, 75, self.size).astype(np.uint8), np.full(self.size, ord("!"), np.uint8)))
        self.text, self.ends = vc.text_of(self.records)
        reverse, malformed = awfm.reverse_complement_reads_host(self.sequenced, self.read_offsets, 0)
        assert malformed == 0
        self.chars = np.concatenate((self.sequenced, reverse))
        rows = [bytes(self.chars[int(a):int(b)]) for a, b in zip(self.offsets[:-1], self.offsets[1:])]
        self.ix = awfm.create_index_from_fasta(self.fasta, awfm.AwFmAlphabetDna, 8, 8, file_src=os.path.join(str(directory), "one_strand.awfmi"))
        inst = rc.host_pipeline(awfm, self.ix, rows)
        case = ch.candidate_case(awfm, inst, E2E["band"], E2E["slots"] - 1, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=E2E["min_votes"])
        got = case.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=E2E["band"], lookback=E2E["lookback"], gap_penalty=E2E["gap_penalty"])
        narrow = dict({name: got[name] for name in vc.SLOT_FIELDS[1:]}, sequences=case.sequences)
        self.slots = {}
        for name in vc.SLOT_FIELDS:  # three columns of chains and a free one
            table = np.zeros((len(rows), E2E["slots"]), vc.SLOT_DTYPES[name])
            if name == "sequences":
                table[...] = NO_WINDOW
            table[:, :E2E["slots"] - 1] = narrow[name]
            self.slots[name] = table
        self.record_names = awfm.record_names(self.ix)

    def close(self):
        self.ix.dealloc()

    def host_loop(self, awfm):
        """the header's loop through the host twins -> dict(first, second: the two strand choices, slots: the final table,
        oriented, aligned, strings, sam)"""
        import verify_chains_common as vc
        q = dict(min_insert=E2E["min_insert"], max_insert=E2E["max_insert"], min_score=E2E["min_score"], unpaired_penalty=E2E["unpaired_penalty"],
                 window_pad=E2E["window_pad"], mapq_cap=E2E["mapq_cap"])

        def choose(slots):
            scored = awfm.score_chains_affine_host(self.chars, self.offsets, slots, self.text, self.ends, min_score=E2E["min_score"],
                                                   mapq_cap=E2E["mapq_cap"], threads=16, **E2E_COMMON)
            tables = dict({name: scored[name] for name in ("slotScores", "slotReadEnds", "slotTextEnds")}, sequences=slots["sequences"])
            return tables, awfm.choose_strands_host(self.offsets, tables, paired=True, threads=16, **q)

        _, first = choose(self.slots)
        got = awfm.score_windows_affine(self.chars, self.offsets, first["windowSequences"], first["windowBegins"], first["windowEnds"], self.text,
                                        self.ends, scoring=E2E["scoring"], min_score=E2E["min_score"], slots=self.slots, slot_stride=E2E["slots"],
                                        slot_column=E2E["slots"] - 1, threads=16)
        slots = {name: got[name] for name in vc.SLOT_FIELDS}
        tables, second = choose(slots)
        columns = dict(slots, **{name: tables[name] for name in ("slotScores", "slotReadEnds", "slotTextEnds")})
        oriented = awfm.orient_reads_host(self.chars, self.offsets, second["strands"], slots=columns, qualities=self.qualities, threads=16)
        table = {name: oriented[name] for name in vc.SLOT_FIELDS}
        aligned = awfm.align_chains_affine_host(oriented["readChars"], oriented["readOffsets"], table, second["strandSlots"], self.text, self.ends,
                                                max_ops=E2E["max_ops"], threads=16, **E2E_COMMON)
        strings = awfm.alignment_strings_host(oriented["sequences"], second["strandSlots"], aligned["textBegins"], aligned["numOps"], aligned["ops"],
                                              self.text, self.ends, classic=True, threads=16)
        arrays = self.sam_arrays(oriented, second, aligned, strings)
        sam = awfm.sam_records_host(arrays, paired=True, threads=16)
        return dict(first=first, second=second, slots=slots, oriented=oriented, aligned=aligned, strings=strings, sam=sam)

    def sam_arrays(self, oriented, second, aligned, strings):
        return dict(readChars=oriented["readChars"], readOffsets=oriented["readOffsets"], qualities=oriented["qualities"],
                    recordNameOffsets=self.record_names[0], recordNameChars=self.record_names[1], sequences=oriented["sequences"],
                    slots=second["strandSlots"], scores=aligned["scores"], editDistances=aligned["editDistances"], textBegins=aligned["textBegins"],
                    textEnds=aligned["textEnds"], cigarOffsets=strings["cigarOffsets"], cigarChars=strings["cigarChars"],
                    mdOffsets=strings["mdOffsets"], mdChars=strings["mdChars"], mappingQualities=second["mappingQualities"],
                    secondScores=second["secondScores"], baseFlags=second["baseFlags"], properPairs=second["properPairs"])

    def check(self, got):
        """every planted pair is found on its strand at its place: the condition on the inputs that the HOST twins meet.  No read
        is left out: every pair is of one of the three kinds and each branch looks at both of its reads."""
        n, F, R, pad = E2E["length"], E2E["fragment"], self.R, E2E["window_pad"]
        first, second, aligned, oriented = got["first"], got["second"], got["aligned"], got["oriented"]
        lines = bytes(got["sam"]["lineChars"]).split(b"\n")[:-1]
        assert len(lines) == R and got["sam"]["numUnaligned"] == 0 and oriented["numMalformed"] == 0
        kinds = [plan["kind"] for plan in self.plan]
        for p, plan in enumerate(self.plan):
            kind, s, reads = plan["kind"], plan["record"], (2 * p, 2 * p + 1)
            for pairing in (first, second):  # reads the seeds place are on their strands from the start
                for m, r in enumerate(reads):
                    if pairing is second or not (kind == "rescued" and m == 1):
                        assert pairing["strands"][r] == plan["strands"][m] and pairing["strandSlots"][r] != NO_SLOT, (p, kind, m)
                        assert pairing["baseFlags"][r] == 0x10 * plan["strands"][m]
            if kind == "far":  # improper before and after; each read has a window around where its mate's place says, on the other strand
                for pairing in (first, second):
                    assert pairing["properPairs"][p] == 0 and pairing["templateLengths"][p] == 0, (p, kind)
                    for m, r in enumerate(reads):
                        row = r + R * (1 - plan["strands"][1 - m])
                        assert pairing["windowSequences"][row] == s and pairing["windowSequences"][r + R * plan["strands"][1 - m]] == NO_WINDOW, (p, m)
                        S = plan["at"][1 - m]
                        want = (S + E2E["min_insert"] - n - pad, S + E2E["max_insert"] + pad) if plan["strands"][1 - m] == 0 else \
                            (S + n - E2E["max_insert"] - pad, S + n - E2E["min_insert"] + n + pad)
                        assert (int(pairing["windowBegins"][row]), int(pairing["windowEnds"][row])) == (max(want[0], 0), max(want[1], 0)), (p, m)
            else:
                assert first["properPairs"][p] == (kind == "plain"), (p, kind)
                if kind == "rescued":  # the first choice names m2's window on the strand opposite to m1's, around its place
                    row = reads[1] + R * plan["strands"][1]
                    assert first["strandSlots"][reads[1]] == NO_SLOT and first["windowSequences"][row] == s, p
                    assert int(first["windowBegins"][row]) <= plan["at"][1] and plan["at"][1] + n <= int(first["windowEnds"][row]), p
                    assert first["windowSequences"][reads[0]] == NO_WINDOW and first["windowSequences"][R + reads[0]] == NO_WINDOW, p
                    assert second["strandSlots"][reads[1]] == E2E["slots"] - 1 and second["rowSlots"][row] == E2E["slots"] - 1, p
                assert second["properPairs"][p] == 1 and int(second["templateLengths"][p]) == F, (p, kind, second["templateLengths"][p])
                for r in reads:
                    assert second["windowSequences"][r] == NO_WINDOW and second["windowSequences"][R + r] == NO_WINDOW, p
                assert second["pairQualities"][p] == E2E["mapq_cap"] and all(second["mappingQualities"][r] == E2E["mapq_cap"] for r in reads), p
            # orient hands the chosen strand's bytes over, the qualities reversed on strand 1; affine alignment returns the planted places
            for m, r in enumerate(reads):
                row = r + R * plan["strands"][m]
                assert bytes(oriented["readChars"][r * n:(r + 1) * n]) == bytes(self.chars[row * n:(row + 1) * n]), (p, m)
                quality = self.qualities[r * n:(r + 1) * n]
                assert bytes(oriented["qualities"][r * n:(r + 1) * n]) == bytes(quality[::-1] if plan["strands"][m] else quality), (p, m)
                clipped = 5 if kind == "rescued" and m == 1 else 0
                assert 0 < int(aligned["scores"][r]) < TOO_LONG, (p, kind, m)
                assert int(aligned["readBegins"][r]) <= clipped and int(aligned["readEnds"][r]) >= n - clipped - (1 if clipped else 0), (p, kind, m)
                assert int(aligned["textBegins"][r]) == plan["at"][m] + int(aligned["readBegins"][r]), (p, kind, m)
                assert int(aligned["textEnds"][r]) == plan["at"][m] + int(aligned["readEnds"][r]), (p, kind, m)
            # the SAM lines of a plain pair, by hand: FLAG 99 / 147 from the forward strand, 83 / 163 from the reverse strand
            if kind == "plain":
                fields = [lines[r].split(b"\t") for r in reads]
                forward = plan["strands"] == (0, 1)
                assert [int(f[1]) for f in fields] == ([99, 147] if forward else [83, 163]), (p, fields[0][1], fields[1][1])
                for m in range(2):
                    f, leftmost = fields[m], plan["at"][m] < plan["at"][1 - m]
                    assert f[2] == b"r%d" % s and int(f[3]) == plan["at"][m] + 1 and f[5] == b"%dM" % n and f[6] == b"=", (p, m, f[:9])
                    assert int(f[7]) == plan["at"][1 - m] + 1 and int(f[8]) == (F if leftmost else -F), (p, m, f[:9])
                    assert f[9] == bytes(oriented["readChars"][reads[m] * n:(reads[m] + 1) * n]) and int(f[4]) == E2E["mapq_cap"], (p, m)
        assert second["numProper"] == len(kinds) - kinds.count("far") and second["numWindows"] == 2 * kinds.count("far")
        assert first["numProper"] == kinds.count("plain") and first["numWindows"] == 2 * kinds.count("far") + kinds.count("rescued")
        assert second["numReverse"] == R // 2 and second["numMalformed"] == 0
