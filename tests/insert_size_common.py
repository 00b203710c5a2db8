"""Insert size (include/awfm_gpu.h "insert size", csrc/awfm_insert.c) restated in plain Python loops for the tests of the host
twins and the device calls: the histogram a pair at a time, the interval a bin at a time, Python integers wrapped to 64-bit two's
complement where the header says so; and cases: the EDGE LIST, a few pairs an edge with hand-computed histograms, counters and
intervals (literals: the restatement is held to them as well), and random slot tables with a range chosen from the restatement's
own qualifying template lengths.  The slot tables are pair_mates_common's (Case, slot, random_case)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_mates_common as pm  # noqa: E402

MAX_INSERT = 1 << 40  # AWFM_PAIR_MAX_INSERT
MAX_BINS, MAX_SPREAD = 65536, 16
PARAMS = dict(low_template=0, high_template=999, min_score=0, min_quality=0, spread=2, min_samples=1, fallback_min=100, fallback_max=900)
ESTIMATE_BYTES = 64


def bins_of(ip):
    return ip["high_template"] - ip["low_template"] + 1


def qualifying(case, ip):
    """per pair: None when the pair does not qualify, else its T -- the header's HISTOGRAM rule"""
    C, floor = case.C, max(ip["min_score"], 1)
    result = []
    for p in range(case.num_pairs):
        best, starts = [], []
        for r in (2 * p, 2 * p + 1):
            begin, end = int(case.offsets[r]), int(case.offsets[r + 1])
            top = None
            for j in range(C):
                score = int(case.slots["slotScores"][r, j])
                if begin <= end and score < pm.TOO_LONG and score >= floor:
                    if top is None or score > int(case.slots["slotScores"][r, top]):
                        top = j
            best.append(top)
            if top is not None:
                starts.append(pm.wrap(int(case.slots["slotTextEnds"][r, top]) - int(case.slots["slotReadEnds"][r, top])))
        T = None
        if best[0] is not None and best[1] is not None:
            a, b = 2 * p, 2 * p + 1
            given = (0, 0) if case.qualities is None else (int(case.qualities[a]), int(case.qualities[b]))
            one_sequence = int(case.slots["sequences"][a, best[0]]) == int(case.slots["sequences"][b, best[1]])
            if one_sequence and given[0] >= ip["min_quality"] and given[1] >= ip["min_quality"]:
                n_b = pm.wrap(int(case.offsets[b + 1]) - int(case.offsets[b]))
                T = pm.wrap(starts[1] + n_b - starts[0])
        result.append(T)
    return result


def histogram_expected(case, ip, histogram=None, samples_before=0, outside_before=0):
    """-> (histogram uint64[bins], numSamples, numOutside), all three added to"""
    h = np.zeros(bins_of(ip), np.uint64) if histogram is None else np.array(histogram, dtype=np.uint64)
    samples, outside = samples_before, outside_before
    for T in qualifying(case, ip):
        if T is None:
            continue
        if ip["low_template"] <= T <= ip["high_template"]:
            h[T - ip["low_template"]] += np.uint64(1)
            samples += 1
        else:
            outside += 1
    return h, samples, outside


def interval_expected(histogram, ip):
    """the header's INTERVAL rule -> a dict of the eight fields (quartiles a list of three)"""
    h = [int(x) for x in histogram]
    N = sum(h)
    if N < max(ip["min_samples"], 1):
        return dict(minInsert=ip["fallback_min"], maxInsert=ip["fallback_max"], quartiles=[0, 0, 0], mean=0, numSamples=N, valid=0)
    quartiles = []
    for k in (1, 2, 3):
        rank, prefix = (k * N + 3) // 4, 0
        for i, count in enumerate(h):
            prefix += count
            if prefix >= rank:
                quartiles.append(ip["low_template"] + i)
                break
    w = ip["spread"] * max(quartiles[2] - quartiles[0], 1)
    lo, hi = max(quartiles[0] - w, -MAX_INSERT), min(quartiles[2] + w, MAX_INSERT)
    weighted = inliers = 0
    for i, count in enumerate(h):
        if lo <= ip["low_template"] + i <= hi:
            weighted += i * count
            inliers += count
    return dict(minInsert=lo, maxInsert=hi, quartiles=quartiles, mean=ip["low_template"] + weighted // inliers, numSamples=N, valid=1)


def params_of(awfm, ip):
    return awfm.insert_params(**ip)


# ---- the edge list ----------------------------------------------------------------------------------------------------------
def pair(T, score=50, sequence=0, qualities=(30, 25), start=1000):
    """one slot a mate, both reads 100 long, mate A's START at `start`, the template length T"""
    return ([pm.slot(score, sequence, start)], [pm.slot(score, sequence, start + T - 100)], (100, 100), qualities)


def estimated(lo, hi, quartiles, mean, N):
    return dict(minInsert=lo, maxInsert=hi, quartiles=list(quartiles), mean=mean, numSamples=N, valid=1)


def fallback(N, lo=100, hi=900):
    return dict(minInsert=lo, maxInsert=hi, quartiles=[0, 0, 0], mean=0, numSamples=N, valid=0)


class Edge:
    """pairs: [(slots of mate A, slots of mate B, the two read lengths (negative: inverted offsets), the two input qualities)];
    null: mappingQualities is NULL; params over PARAMS; want: the hand-computed {T: count}, numSamples, numOutside and interval"""

    def __init__(self, name, pairs, histogram, samples, outside, interval, null=False, **params):
        self.name, self.pairs, self.null = name, pairs, null
        self.params = dict(PARAMS, **params)
        self.histogram, self.samples, self.outside, self.interval = histogram, samples, outside, interval

    def case(self, C=4):
        offsets, at = [1003], 1003  # (room for reads of negative length)
        slots = {name: [] for name in pm.SLOT_INPUTS}
        given = []
        for a, b, lengths, qualities in self.pairs:
            for mate, length in zip((a, b), lengths):
                at += length
                offsets.append(at)
                padded = list(mate) + [pm.STATUS] * (C - len(mate))
                slots["slotScores"].append([s[0] for s in padded])
                slots["sequences"].append([s[1] for s in padded])
                slots["slotReadEnds"].append([s[2] for s in padded])
                slots["slotTextEnds"].append([s[3] for s in padded])
            given += list(qualities)
        return pm.Case(offsets, slots, None if self.null else given, {})

    def dense(self):
        """the hand-computed histogram as an array"""
        h = np.zeros(bins_of(self.params), np.uint64)
        for T, count in self.histogram.items():
            h[T - self.params["low_template"]] = count
        return h


FAR = 1 << 41  # a START from which a template length of -2^40 still ends at a position >= 0
EDGES = [
    # ranks (N + 3) / 4, (2 N + 3) / 4, (3 N + 3) / 4
    Edge("N = 1", [pair(300)], {300: 1}, 1, 0, estimated(298, 302, (300, 300, 300), 300, 1)),            # ranks 1 1 1, w = 2 * max(0, 1)
    Edge("N = 2", [pair(300), pair(310)], {300: 1, 310: 1}, 2, 0, estimated(280, 330, (300, 300, 310), 305, 2)),  # ranks 1 1 2, w = 20
    Edge("N = 3", [pair(T) for T in (320, 300, 310)], {300: 1, 310: 1, 320: 1}, 3, 0, estimated(260, 360, (300, 310, 320), 310, 3)),  # 1 2 3
    Edge("N = 4", [pair(T) for T in (300, 310, 320, 330)], {300: 1, 310: 1, 320: 1, 330: 1}, 4, 0,
         estimated(260, 360, (300, 310, 320), 315, 4)),                                                  # ranks 1 2 3; mean 1260 / 4
    Edge("N = 5", [pair(T) for T in (300, 310, 320, 330, 340)], {300: 1, 310: 1, 320: 1, 330: 1, 340: 1}, 5, 0,
         estimated(270, 370, (310, 320, 330), 320, 5)),                                                  # ranks 2 3 4
    Edge("q3 = q1, spread 0", [pair(300)] * 3, {300: 3}, 3, 0, estimated(300, 300, (300, 300, 300), 300, 3), spread=0),
    Edge("q3 = q1, spread 16", [pair(300)] * 3, {300: 3}, 3, 0, estimated(284, 316, (300, 300, 300), 300, 3), spread=16),
    # 199 and 501 qualify and lie outside; q = 200, 200, 500, w = 600, mean = 200 + (0 + 300) / 2
    Edge("T at lowTemplate and at highTemplate, and one outside each end", [pair(T) for T in (200, 500, 199, 501)], {200: 1, 500: 1}, 2, 2,
         estimated(-400, 1100, (200, 200, 500), 350, 2), low_template=200, high_template=500),
    # bins 199 and 200: the mean is -500 + floor(399 / 2) = -301, the floor of -300.5 (a division that truncated would give -300)
    Edge("a negative range, a negative T and the floor of the mean", [pair(-300), pair(-301)], {-300: 1, -301: 1}, 2, 0,
         estimated(-303, -298, (-301, -301, -300), -301, 2), low_template=-500, high_template=-100),
    Edge("a range of one bin", [pair(300), pair(300), pair(301), pair(299)], {300: 2}, 2, 2, estimated(298, 302, (300, 300, 300), 300, 2),
         low_template=300, high_template=300),
    Edge("N = minSamples - 1", [pair(300), pair(310)], {300: 1, 310: 1}, 2, 0, fallback(2), min_samples=3),
    Edge("N = minSamples", [pair(300), pair(310), pair(320)], {300: 1, 310: 1, 320: 1}, 3, 0, estimated(260, 360, (300, 310, 320), 310, 3),
         min_samples=3),
    Edge("minSamples 0 and an empty histogram", [([pm.STATUS], [pm.STATUS], (100, 100), (30, 25))], {}, 0, 0, fallback(0), min_samples=0),
    Edge("a quality at minQuality and one below it", [pair(300, qualities=(30, 25)), pair(310, qualities=(30, 24)), pair(320, qualities=(24, 30))],
         {300: 1}, 1, 0, estimated(298, 302, (300, 300, 300), 300, 1), min_quality=25),
    Edge("qualities NULL and minQuality 0", [pair(300)], {300: 1}, 1, 0, estimated(298, 302, (300, 300, 300), 300, 1), null=True),
    Edge("qualities NULL and minQuality 1", [pair(300)], {}, 0, 0, fallback(0), null=True, min_quality=1),
    # the second pair: A's best slot names sequence 0, a lower slot of A and B's best name sequence 1
    Edge("best slots of different sequences", [([pm.slot(50, 0, 1000)], [pm.slot(50, 1, 1200)], (100, 100), (30, 25)),
                                               ([pm.slot(60, 0, 1000), pm.slot(50, 1, 1000)], [pm.slot(60, 1, 1200)], (100, 100), (30, 25))],
         {}, 0, 0, fallback(0)),
    Edge("one mate without a counting slot", [([pm.slot(50, 0, 1000)], [pm.STATUS], (100, 100), (30, 25)),
                                              ([pm.STATUS], [pm.slot(50, 0, 1200)], (100, 100), (30, 25))], {}, 0, 0, fallback(0)),
    Edge("inverted read offsets", [([pm.slot(50, 0, 1000)], [pm.slot(50, 0, 1200)], (-50, 100), (30, 25)),
                                   ([pm.slot(50, 0, 1000)], [pm.slot(50, 0, 1200)], (100, -50), (30, 25))], {}, 0, 0, fallback(0)),
    # (0, 0) gives 1200 + 100 - 1000; (1, 0) 280, (0, 1) 350, (1, 1) 330
    Edge("a tie of scores: the lowest slot is the best", [([pm.slot(50, 0, 1000), pm.slot(50, 0, 1020)], [pm.slot(40, 0, 1200), pm.slot(40, 0, 1250)],
                                                          (100, 100), (30, 25))], {300: 1}, 1, 0, estimated(298, 302, (300, 300, 300), 300, 1)),
    # slot 0 of A holds AWFM_VERIFY_TOO_LONG, the largest "score" there is: slot 1 is the best, T = 1200 + 100 - 1010
    Edge("a score that is a status value", [([(pm.TOO_LONG, 0, 100, 1100), pm.slot(50, 0, 1010)], [pm.slot(40, 0, 1200)], (100, 100), (30, 25))],
         {290: 1}, 1, 0, estimated(288, 292, (290, 290, 290), 290, 1)),
    Edge("minScore at a score and above one", [([pm.slot(59, 0, 1000), pm.slot(60, 0, 1010)], [pm.slot(60, 0, 1200)], (100, 100), (30, 25)),
                                               ([pm.slot(59, 0, 1000)], [pm.slot(60, 0, 1200)], (100, 100), (30, 25))],
         {290: 1}, 1, 0, estimated(288, 292, (290, 290, 290), 290, 1), min_score=60),
    # w = 16 * 20: maxInsert = 2^40 + 320 is clamped, minInsert = 2^40 - 20 - 320 is not
    Edge("an interval clamped at 2^40", [pair(MAX_INSERT - d) for d in (20, 10, 0)], {MAX_INSERT - 20: 1, MAX_INSERT - 10: 1, MAX_INSERT: 1}, 3, 0,
         estimated(MAX_INSERT - 340, MAX_INSERT, (MAX_INSERT - 20, MAX_INSERT - 10, MAX_INSERT), MAX_INSERT - 10, 3),
         low_template=MAX_INSERT - 1000, high_template=MAX_INSERT, spread=16),
    Edge("an interval clamped at -2^40", [pair(-MAX_INSERT + d, start=FAR) for d in (0, 10, 20)],
         {-MAX_INSERT: 1, -MAX_INSERT + 10: 1, -MAX_INSERT + 20: 1}, 3, 0,
         estimated(-MAX_INSERT, -MAX_INSERT + 340, (-MAX_INSERT, -MAX_INSERT + 10, -MAX_INSERT + 20), -MAX_INSERT + 10, 3),
         low_template=-MAX_INSERT, high_template=-MAX_INSERT + 1000, spread=16),
]


def check_estimate(got, want, what=""):
    for name in ("minInsert", "maxInsert", "quartiles", "mean", "numSamples", "valid"):
        assert got[name] == want[name], (what, name, got[name], want[name])


# ---- random tables ----------------------------------------------------------------------------------------------------------
def random_table(seed, pairs, C, **params):
    """pair_mates_common.random_case and a range chosen from the restatement's own qualifying T: from about the sixteenth
    smallest up to one below the largest, so that some qualifying pairs fall outside (the largest always) and most inside
    -> (Case, params)"""
    case = pm.random_case(seed, pairs, C, qualities=seed % 4 != 3)
    ip = dict(PARAMS, min_quality=0 if case.qualities is None else 3, min_score=seed % 3, **params)
    Ts = sorted(T for T in qualifying(case, ip) if T is not None)
    if len(Ts) >= 2 and Ts[-1] > Ts[0]:
        low = Ts[len(Ts) // 16]
        high = max(Ts[-1] - 1, low)
        ip.update(low_template=low, high_template=min(high, low + MAX_BINS - 1))
    return case, ip


def check_condition(case, ip):
    """what the tests ask of a random table of 64 pairs and more, on the restatement's counts"""
    _, samples, outside = histogram_expected(case, ip)
    if case.num_pairs >= 64:
        assert 8 * samples >= case.num_pairs and outside >= 1, (case.num_pairs, case.C, samples, outside)
    return samples, outside


# ---- end to end: pair_mates_common.EndToEnd with the interval estimated after the first slot scores ----
E2E_INSERT = dict(low_template=0, high_template=4095, min_score=pm.E2E["min_score"], min_quality=1, spread=16, min_samples=8, fallback_min=0,
                  fallback_max=4095)
# the plain pairs plant T = 400 and are most of the samples (the far pairs, a sixteenth, give 2400): all three quartiles are 400,
# w = 16 * max(0, 1), the interval [384, 416]
E2E_QUARTILES, E2E_INTERVAL = [400, 400, 400], (384, 416)


class EstimatingHostSide(pm.HostSide):
    """the loop's calls through the host twins, the interval estimated after the first slot scores and kept"""

    def __init__(self, awfm, e2e):
        super().__init__(awfm, e2e)
        self.estimate = None

    def pair(self, slots, scored):
        tables = dict({name: scored[name] for name in ("slotScores", "slotReadEnds", "slotTextEnds")}, sequences=slots["sequences"])
        if self.estimate is None:
            self.estimate = self.awfm.estimate_insert_size_host(self.e.offsets, tables, self.awfm.insert_params(**E2E_INSERT),
                                                                mapping_qualities=scored["mappingQualities"], threads=16)
        E = pm.E2E
        return self.awfm.pair_mates_host(self.e.offsets, tables, self.estimate["minInsert"], self.estimate["maxInsert"],
                                         mapping_qualities=scored["mappingQualities"], min_score=E["min_score"], unpaired_penalty=E["unpaired_penalty"],
                                         window_pad=E["window_pad"], mapq_cap=E["mapq_cap"], threads=16)


def check_end_to_end(e, estimate, second, aligned):
    """the estimate is the planted library's, and every planted plain and rescued pair comes out proper at its planted place"""
    assert estimate["valid"] == 1 and estimate["quartiles"] == E2E_QUARTILES and estimate["mean"] == 400, estimate
    assert (estimate["minInsert"], estimate["maxInsert"]) == E2E_INTERVAL, estimate
    kinds = [k for _, _, _, k in e.plan]
    assert estimate["numSamples"] >= kinds.count("plain"), estimate
    n, F = pm.E2E["length"], pm.E2E["fragment"]
    for p, (s, at, mate_at, kind) in enumerate(e.plan):
        a, b = 2 * p, 2 * p + 1
        if kind == "far":
            assert second["properPairs"][p] == 0, p
            continue
        assert second["properPairs"][p] == 1 and int(second["templateLengths"][p]) == F, (p, kind)
        for r, where, clipped in ((a, at, 0), (b, mate_at, 5 if kind == "rescued" else 0)):
            assert 0 < int(aligned["scores"][r]) < pm.TOO_LONG, (p, kind, r)
            assert int(aligned["readBegins"][r]) <= clipped and int(aligned["readEnds"][r]) >= n - clipped - (1 if clipped else 0), (p, kind, r)
            assert int(aligned["textBegins"][r]) == where + int(aligned["readBegins"][r]), (p, kind, r)
            assert int(aligned["textEnds"][r]) == where + int(aligned["readEnds"][r]), (p, kind, r)
    assert second["numProper"] == len(kinds) - kinds.count("far")
