"""Shared by the tests of awfmScoreChainsAffine / awfmGpuScoreChainsAffine (include/awfm_gpu.h, "slot scores and mapping quality"):
the per-slot definition is tests/align_affine_common.py's `local` (imported, not restated), the per-read rules are restated here
over Python integers, and the edge list of the per-read rules carries hand-computed values.  Slots, letters, texts and batches
are those of tests/align_chains_common.py."""
import os

import numpy as np

import align_affine_common as af
import align_chains_common as ac
import verify_chains_common as vc

NONE, MALFORMED, TOO_WIDE, TOO_LONG, NO_SLOT = af.NONE, af.MALFORMED, af.TOO_WIDE, af.TOO_LONG, af.NO_SLOT
DNA, AMINO = af.DNA, af.AMINO
SLOT_OUTPUTS = dict(slotScores=np.uint32, slotReadEnds=np.uint32, slotTextEnds=np.uint64)
READ_OUTPUTS = dict(bestSlots=np.uint32, bestScores=np.uint32, secondSlots=np.uint32, secondScores=np.uint32, mappingQualities=np.uint8)
COUNTERS = ("numUnscored", "numMapped")
ALL_OUTPUTS = list(SLOT_OUTPUTS) + list(READ_OUTPUTS) + list(COUNTERS)
MAX_MAPQ = 254


def read_rules(values, read_ends, text_ends, sequences, min_score, cap):
    """the five per-read rules over one read's C results -> (bestSlot, bestScore, secondSlot, secondScore, mapq)"""
    floor = max(min_score, 1)
    counting = [j for j, v in enumerate(values) if v < TOO_LONG and v >= floor]
    if not counting:
        return NO_SLOT, 0, NO_SLOT, 0, 0
    best = max(counting, key=lambda j: (values[j], -j))
    rest = [j for j in counting if j != best and
            (sequences[j], read_ends[j], text_ends[j]) != (sequences[best], read_ends[best], text_ends[best])]
    second = max(rest, key=lambda j: (values[j], -j)) if rest else NO_SLOT
    second_score = values[second] if rest else 0
    return best, values[best], second, second_score, cap * (values[best] - second_score) // values[best]


class Case(af.Case):
    """a verification case under the scoring call (`chosen` is what the per-slot restatement sets slot by slot)"""

    def score(self, awfm, w, x, scoring=af.DEFAULT, min_score=0, cap=60, **kw):
        return awfm.score_chains_affine_host(self.read_chars, self.offsets, self.slots, self.text, self.ends, self.alphabet, band_pad=w,
                                             max_drift=x, scoring=scoring, min_score=min_score, mapq_cap=cap,
                                             num_read_chars=self.num_read_chars, **kw)

    def expected_scores(self, w, x, scoring=af.DEFAULT, min_score=0, cap=60, unscored_before=0, mapped_before=0):
        """the whole call restated in Python: af.local per slot, read_rules per read"""
        want = {name: np.zeros((self.num_reads, self.C), dtype) for name, dtype in SLOT_OUTPUTS.items()}
        want.update({name: np.zeros(self.num_reads, dtype) for name, dtype in READ_OUTPUTS.items()})
        unscored, mapped = unscored_before, mapped_before
        kept = self.chosen
        for r in range(self.num_reads):
            for j in range(self.C):
                self.chosen = np.full(self.num_reads, j, np.uint32)
                status = self.status(r, w, x)
                if not isinstance(status, tuple):
                    want["slotScores"][r, j] = status
                    unscored += status != NONE
                    continue
                S, E, lo, hi = status
                score, _, _, re, _, te, _ = af.local(self.read(r), bytes(self.text[S:E]), lo, hi, scoring, self.alphabet)
                want["slotScores"][r, j], want["slotReadEnds"][r, j], want["slotTextEnds"][r, j] = score, re, te
            rules = read_rules([int(v) for v in want["slotScores"][r]], [int(v) for v in want["slotReadEnds"][r]],
                               [int(v) for v in want["slotTextEnds"][r]], [int(v) for v in self.slots["sequences"][r]], min_score, cap)
            for name, value in zip(READ_OUTPUTS, rules):
                want[name][r] = value
            mapped += rules[0] != NO_SLOT
        self.chosen = kept
        return dict(want, numUnscored=unscored, numMapped=mapped)

    def by_the_affine_call(self, awfm, w, x, scoring=af.DEFAULT, threads=4):
        """slotScores, slotReadEnds, slotTextEnds as awfmAlignChainsAffine gives them with slots[:] = j, j = 0 .. C - 1"""
        want = {name: np.zeros((self.num_reads, self.C), dtype) for name, dtype in SLOT_OUTPUTS.items()}
        kept = self.chosen
        for j in range(self.C):
            self.chosen = np.full(self.num_reads, j, np.uint32)
            got = self.host(awfm, w, x, scoring, max_ops=1, threads=threads, outputs=["scores", "readEnds", "textEnds"])
            want["slotScores"][:, j], want["slotReadEnds"][:, j], want["slotTextEnds"][:, j] = got["scores"], got["readEnds"], got["textEnds"]
        self.chosen = kept
        return want


def as_scored(case):
    chosen = getattr(case, "chosen", np.zeros(case.num_reads, np.uint32))
    return Case(case.read_chars.tobytes(), case.offsets, case.slots, chosen, case.text.tobytes(), case.ends, case.alphabet, case.num_read_chars)


def random_case(*args, **kw):
    """ac.random_case's reads and slots: slot 0 of a read is its own locus, the others are loci elsewhere; some unused, some
    malformed, some hanging over a record end"""
    return as_scored(ac.random_case(*args, **kw))


def assert_equal(got, want, names=None, what=""):
    for name in (names or want):
        if name in COUNTERS:
            assert got[name] == want[name], (what, name, got[name], want[name])
        else:
            bad = np.argwhere(np.asarray(got[name]) != np.asarray(want[name]))
            assert not len(bad), (what, name, bad[:5].tolist(), int(got[name][tuple(bad[0])]), int(want[name][tuple(bad[0])]))


class Builder:
    """a text of records and reads with up to C slots each, added one at a time with what the read must get: (bestSlot, bestScore,
    secondSlot, secondScore, mapq) under (1, 4, 6, 1), and what its slots must score"""

    def __init__(self, records, C, alphabet=DNA):
        base = vc.Builder(records, False, alphabet)
        self.text, self.ends, self.alphabet, self.C = base.text, base.ends, alphabet, C
        self.reads, self.rows, self.values, self.scores, self.names = [], [], [], [], []

    def add(self, name, read, slots, value, scores):
        """slots: a list of (sequence, bD, eD) or None (unused) or a raw row of six"""
        rows = []
        for slot in list(slots) + [None] * (self.C - len(slots)):
            if slot is None:
                rows.append((NONE, 0, 0, 0, 0, 0))
            elif len(slot) == 3:
                rows.append((slot[0], 1, 0, len(read), slot[1], slot[2]))
            else:
                rows.append(tuple(slot))
        self.reads.append(bytes(read))
        self.rows.append(rows)
        self.values.append(value)
        self.scores.append(list(scores) + [NONE] * (self.C - len(scores)))
        self.names.append(name)

    def case(self, skew=0):
        offsets = np.cumsum([skew] + [len(r) for r in self.reads])
        slots = {name: np.array([[int(row[k]) for row in rows] for rows in self.rows], vc.SLOT_DTYPES[name]) for k, name in enumerate(vc.SLOT_FIELDS)}
        return Case(b"#" * skew + b"".join(self.reads), offsets, slots, np.zeros(len(self.reads), np.uint32), self.text, self.ends, self.alphabet)

    def check(self, got):
        bad = []
        for r, (name, value, scores) in enumerate(zip(self.names, self.values, self.scores)):
            have = tuple(int(got[f][r]) for f in READ_OUTPUTS)
            if have != value or [int(v) for v in got["slotScores"][r]] != scores:
                bad.append((name, have, value, got["slotScores"][r].tolist(), scores))
        assert not bad, bad

    def unscored(self):
        return sum(v in (MALFORMED, TOO_WIDE, TOO_LONG) for scores in self.scores for v in scores)

    def mapped(self):
        return sum(value[0] != NO_SLOT for value in self.values)


def _letters(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"acgt", np.uint8), n))


T0 = _letters(101, 300)
READ = T0[10:110]  # 100 exact characters of record 0 (and of record 1, its copy) on diagonal 10
#: record 1 is record 0 once more; nothing matches record 2; record 3 holds READ[20 .. 57) at 40 .. 77, diagonal 20, and nothing else
RULE_RECORDS = [T0, T0, b"n" * 300, b"n" * 40 + READ[20:57] + b"n" * 63]
OWN, DUPLICATE, COPY, COPY_SHIFTED, NOTHING, DECOY = (0, 10, 10), (0, 12, 12), (1, 10, 10), (1, 12, 12), (2, 10, 10), (3, 20, 20)


def rules_builder(C=4, cap=60):
    """the edge list of the per-read rules under (1, 4, 6, 1), w = 8, x = 15 and minScore 0: every value computed by hand.  A slot
    on READ's own diagonal scores 100 and ends in the cell (100, 110); so does one on diagonal 12 (its band [4, 20] holds
    diagonal 10), and so do both in the copy; a slot in record 2 scores 0; the decoy slot scores 37 and ends in (57, 77):
    floor(60 * 63 / 100) = 37."""
    b = Builder(RULE_RECORDS, C)
    none, alone, tied, q = (NO_SLOT, 0, NO_SLOT, 0, 0), (0, 100, NO_SLOT, 0, cap), (0, 100, 1, 100, 0), cap * 63 // 100
    cases = [("no slot at all", READ, [], none, []),
             ("no slot counts: score 0", READ, [NOTHING], none, [0]),
             ("n = 0", b"", [OWN], none, [0]),
             ("one slot: second is 0 and mapq = cap", READ, [OWN], alone, [100]),
             ("two equal scores: the lowest slot is best, second = best, mapq 0", READ, [OWN, COPY], tied, [100, 100]),
             ("a duplicate: diagonals 10 and 12 of one sequence give one end cell", READ, [OWN, DUPLICATE], alone, [100, 100]),
             ("the same end cell in another sequence is a competitor", READ, [OWN, COPY_SHIFTED], tied, [100, 100]),
             ("best 100, second 37", READ, [OWN, DECOY], (0, 100, 1, 37, q), [100, 37]),
             ("second 37 ahead of best 100", READ, [DECOY, OWN], (1, 100, 0, 37, q), [37, 100]),
             ("a duplicate plus a true second", READ, [OWN, DECOY, DUPLICATE], (0, 100, 1, 37, q), [100, 37, 100]),
             ("two seconds of one score: the lowest slot", READ, [NOTHING, OWN, DECOY, DECOY], (1, 100, 2, 37, q), [0, 100, 37, 37]),
             ("status slots are ignored and counted", READ, [(4, 10, 10), OWN, (0, 0, 16)], (1, 100, NO_SLOT, 0, cap), [MALFORMED, 100, TOO_WIDE]),
             ("a duplicate of the best in the lowest slot is the best", READ, [DUPLICATE, OWN, COPY], (0, 100, 2, 100, 0), [100, 100, 100])]
    for name, read, slots, value, scores in cases:
        if len(slots) <= C:
            b.add(name, read, slots, value, scores)
    return b


def e2e_records(directory):
    """vc.planted_with_decoys' records, reads and decoys, and behind them an exact copy of the record of the first planted read
    that has no decoy -> (FASTA path, records, reads, planted, decoy_of, copies: {record: its copy})"""
    _, records, reads, planted, decoy_of = vc.planted_with_decoys(directory)
    source = next(plant[0] for r, plant in enumerate(planted) if plant is not None and r not in decoy_of)
    copies = {source: len(records)}
    records.append(records[source])
    path = os.path.join(directory, "mapped.fa")
    with open(path, "wb") as f:
        for i, record in enumerate(records):
            f.write(b">r%d\n" % i + b"".join(record[j:j + 70] + b"\n" for j in range(0, len(record), 70)))
    return path, records, reads, planted, decoy_of, copies


E2E_BAND, E2E_MIN_VOTES, E2E_SLOTS, E2E_GAP_PENALTY, E2E_CAP = 2, 2, 4, 1, 60


def e2e_host_case(awfm, directory):
    """the host's pipeline on e2e_records' FASTA file: longest suffix matches -> locate -> local positions (tests/
    read_candidates_common.py), awfmReadCandidates, awfmReadChains with the parameters of the device's end-to-end test -> (the
    case whose slots they wrote, records, planted, decoy_of, copies)"""
    import read_candidates_common as rc
    import read_chains_common as ch
    path, records, reads, planted, decoy_of, copies = e2e_records(directory)
    ix = awfm.create_index_from_fasta(path, awfm.AwFmAlphabetDna, 8, 8, file_src=os.path.join(directory, "mapped_host.awfmi"))
    inst = rc.host_pipeline(awfm, ix, reads)
    candidates = ch.candidate_case(awfm, inst, E2E_BAND, E2E_SLOTS, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=E2E_MIN_VOTES)
    chains = candidates.host(awfm, max_hits_per_seed=rc.E2E_MAX_HITS, band=E2E_BAND, gap_penalty=E2E_GAP_PENALTY)
    ix.dealloc()
    slots = dict({name: chains[name] for name in vc.SLOT_FIELDS[1:]}, sequences=candidates.sequences)
    text, ends = vc.text_of(records)
    offsets = np.concatenate(([0], np.cumsum([len(read) for read in reads])))
    case = Case(b"".join(reads), offsets, slots, np.zeros(len(reads), np.uint32), text.tobytes(), ends)
    return case, records, planted, decoy_of, copies


def assert_planted_reads_mapped(case, got, planted, decoy_of, copies, cap=E2E_CAP):
    """EVERY planted read's best slot is its own record; where its decoy has a slot, the decoy's score is the second and strictly
    smaller, and mapq > 0; a read of the duplicated record meets its copy at the same score: mapq 0 -> (decoys met, copies met)"""
    decoys_met = copies_met = 0
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        best = int(got["bestSlots"][r])
        assert best != NO_SLOT and int(case.slots["sequences"][r, best]) == record, (r, plant, got["slotScores"][r].tolist(), case.slots["sequences"][r].tolist())
        assert int(got["bestScores"][r]) == int(got["slotScores"][r, best]) >= 120 - 5 * 5 - 7, (r, plant)  # four or five edits planted
        second = int(got["secondSlots"][r])
        scored = [j for j in range(case.C) if got["slotScores"][r, j] < TOO_LONG and got["slotScores"][r, j] > 0]
        if r in decoy_of and any(int(case.slots["sequences"][r, j]) == decoy_of[r] for j in scored):
            decoys_met += 1
            assert second != NO_SLOT and int(case.slots["sequences"][r, second]) == decoy_of[r], (r, plant, got["slotScores"][r].tolist())
            assert 0 < int(got["secondScores"][r]) < int(got["bestScores"][r]) and int(got["mappingQualities"][r]) > 0, (r, plant)
        if record in copies:
            copies_met += 1
            assert second != NO_SLOT and int(case.slots["sequences"][r, second]) == copies[record], (r, plant, case.slots["sequences"][r].tolist())
            assert got["secondScores"][r] == got["bestScores"][r] and int(got["mappingQualities"][r]) == 0, (r, plant)
        if second == NO_SLOT:
            assert int(got["mappingQualities"][r]) == cap, (r, plant)
    return decoys_met, copies_met
