"""Shared by tests/test_gap_runs.py and tests/test_gpu_gap_runs.py: reads that carry ONE GAP RUN of 4 to 63 characters (windows: 2
to 300) between two exact flanks, for the five alignment calls of the read path.  A gap of g characters reaches lane k + g of
a banded row from lane k, and the kernels get it there by a log-step prefix scan over the group's lanes: a run of up to four
characters is served by the steps 1 and 2 alone, so only longer runs exercise the steps 4, 8, 16 and 32.  The window kernel
carries E and its origin from lane to lane, from column block to column block and from one reload of its boundary rows to the
next; only a gap that is open across such an edge reads those words.

Every case is built with the builders of the five *_common modules, its conditions (the restated script holds the planted run)
are asserted by the CPU test on the restatement alone, and `scan_model` is the kernel's row with the scan written out as the
kernel runs it, with the steps to run as an argument: complete it equals af.local, with one step missing it must not.

THE FLANK RULE.  A gap of d characters between flanks of a and c characters is taken, not clipped, when min(a, c) match >
gapOpen + d gapExtend: under (1, 4, 6, 1) min(a, c) > d + 6, under (2, 4, 4, 2) > d + 2, under (255, 255, 255, 255) > d + 1.
Under unit costs (chain alignment) the read is global and the alternative to the gap is a flank of mismatches, three in four
characters of random DNA: 0.75 min(a, c) > d with room for the spread.  Under (1, 0, 0, 1) a mismatch is free, the alternative is
one flank's diagonal for the whole read, and what it collects along the other flank -- a match in four characters, more with a
gap of one here and there -- has to stay below that flank's length less d: flanks of 1.6 d + 10 lost the run in 3 of 32 trials,
flanks of 2 d + 10 in none.  flank(d) = 2 d + 10 serves them all.  The
deleted characters avoid the letter ahead of them and the first one avoids the letter behind the run, so that neither a shifted
nor, under unit costs, a split run ties with the planted one; inserted characters are n (x in proteins), which match nothing."""
import contextlib

import numpy as np

import align_affine_common as af
import score_chains_common as sc
import verify_chains_common as vc
import window_scores_common as ws

DNA, AMINO = vc.DNA, vc.AMINO
RUNS = (4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 62, 63)
AMINO_RUNS = (5, 17, 33, 63)
EXPENSIVE = (af.DEFAULT, (2, 4, 4, 2), (255, 255, 255, 255))
CHEAP = ((1, 1, 0, 1), (1, 0, 0, 1))  # opening and extending tie
SCORINGS = EXPENSIVE + CHEAP
UNIT_MAX_OPS, CAP = 320, 60  # (under unit costs a near miss goes through its short flank by substitutions)
OP_OF_KIND = {"D": af.OP_D, "I": af.OP_I}


def max_ops(scoring):
    """the planted scripts have five runs at the most; where a mismatch costs nothing a script changes run with every character"""
    return 8 if scoring in EXPENSIVE else 320


def flank(d):
    return 2 * d + 10


def natural_group(w, x):
    width = x + 2 * w + 1
    return 16 if width <= 16 else 32 if width <= 32 else 64


def letters_of(alphabet):
    return np.frombuffer(b"acgt" if alphabet == DNA else vc.AMINO_LETTERS.encode(), np.uint8)


class Plant:
    """one read and its record: left flank of a, a run of d (kind D: text characters missing from the read; kind I: characters
    the text lacks), right flank of c; the left flank begins at record offset p.  near: None, or why the run must NOT be taken"""

    def __init__(self, rng, alphabet, kind, d, a, c, near=None):
        letters = letters_of(alphabet)
        self.kind, self.d, self.a, self.c, self.near, self.alphabet = kind, d, a, c, near, alphabet
        self.p, tail = int(rng.integers(70, 90)), int(rng.integers(70, 90))
        A, C = bytes(rng.choice(letters, a)), bytes(rng.choice(letters, c))
        head, rest = bytes(rng.choice(letters, self.p)), bytes(rng.choice(letters, tail))
        if kind == "D":
            gap = bytearray(rng.choice([v for v in letters if v != A[-1]], d))
            gap[0] = int(rng.choice([v for v in letters if v not in (A[-1], C[0])]))
            self.read, self.record = A + C, head + A + bytes(gap) + C + rest
        else:
            self.read, self.record = A + (b"n" if alphabet == DNA else b"x") * d + C, head + A + C + rest
        self.bD, self.eD = self.p, self.p + (d if kind == "D" else -d)
        self.name = f"{d}{kind} after {a}, {c} behind" + (f" ({near})" if near else "")
        self.s = self.decoy_s = self.decoy_diagonal = self.back = None  # its record, its decoy's, and (read, record) for a band of pad

    def decoy(self, rng):
        """a record that holds the first half of the right flank at offset 300, and the diagonal it lies on"""
        letters = letters_of(self.alphabet)
        half = self.read[len(self.read) - self.c:len(self.read) - self.c + self.c // 2]
        return bytes(rng.choice(letters, 300)) + half + bytes(rng.choice(letters, 380)), 300 - (len(self.read) - self.c)


def there_and_back(rng, p):
    """for verification, which is global at both ends, in a band that is all pad: a deletion of d and an insertion of d (kind I: the
    other way round) around a middle of 2 d + 12 exact characters -> (read, record); the read lies 40 characters into the record"""
    letters = letters_of(p.alphabet)
    A, M, Z = (bytes(rng.choice(letters, k)) for k in (p.d + 10, 2 * p.d + 12, p.d + 10))
    gap = bytearray(rng.choice([v for v in letters if v != A[-1]], p.d))
    gap[0] = int(rng.choice([v for v in letters if v not in (A[-1], M[0])]))
    nothing = (b"n" if p.alphabet == DNA else b"x") * p.d
    read, body = (A + M + nothing + Z, A + bytes(gap) + M + Z) if p.kind == "D" else (A + nothing + M + Z, A + M + bytes(gap) + Z)
    return read, bytes(rng.choice(letters, 40)) + body + bytes(rng.choice(letters, 40))


class Batch:
    """the reads of one (w, x) over the corpus's one text: `case` with one slot a read (verification, chain alignment, affine
    alignment), `scored` with three (the same band from its other end or, in a pad band, the run's other diagonal: a duplicate; and
    for every third read a decoy elsewhere), and what verification sees where the band is all pad: `verified`, whose reads come
    back to their diagonal"""

    def __init__(self, w, x, plants, alphabet, records):
        self.w, self.x, self.plants, self.alphabet, self.group = w, x, plants, alphabet, natural_group(w, x)
        self.decoys = [r for r, p in enumerate(plants) if p.decoy_s is not None]
        scored = sc.Builder(records, 3, alphabet)
        for p in plants:
            own = (p.s, p.bD, p.eD) if x else (p.s, p.bD, p.bD)
            twin = (p.s, p.eD, p.bD) if x else (p.s, p.eD, p.eD)
            scored.add(p.name, p.read, [own, twin, None if p.decoy_s is None else (p.decoy_s, p.decoy_diagonal, p.decoy_diagonal)], None, [])
        self.scored = scored.case()
        self.case = sc.Case(self.scored.read_chars.tobytes(), self.scored.offsets, {name: a[:, :1] for name, a in self.scored.slots.items()},
                            np.zeros(len(plants), np.uint32), self.scored.text.tobytes(), self.scored.ends, alphabet)
        self.verified, self.distances = self.case, [p.d for p in plants]
        if not x:
            b = vc.Builder(records, False, alphabet)
            for p in plants:
                read, s = p.back
                b.add(p.name, read, 0, len(read), s, 40, 40 + len(read), 2 * p.d)
            self.verified, self.distances = b.case(), [2 * p.d for p in plants]

    def max_rows(self):
        return max(int(np.diff(case.offsets.astype(np.int64)).max()) for case in (self.case, self.verified))


def _placements(kind, d, index):
    """(a, c) twice: the run at a chunk edge -- a deletion behind row 61 .. 67 (125 .. 131, 189 .. 195 where the flank rule needs
    more rows), an insertion astride rows 64 | 65 (128 | 129, 192 | 193) -- and elsewhere: a deletion mid-chunk, an insertion astride
    the next chunk edge"""
    f = flank(d)
    c = f + index % 3
    if kind == "D":
        edge = next(base + index % 7 for base in (61, 125, 189) if f <= base)
        mid = f + 2 if 12 <= (f + 2) % 64 <= 52 else f + 24
        return (edge, c), (mid, c + 1)
    first, second = [edge - d // 2 for edge in (64, 128, 192, 256) if edge - d // 2 >= f][:2]
    return (first, c), (second, c + 1)


def banded_corpus(alphabet=DNA, seed=77):
    """-> the batches, one per (w, x): (0, 63) and (0, d) for every d (the run begins in lane 0 and ends in lane d, in (0, d) the
    band's last), (8, 15) and (24, 15) for d <= 15 (from lane w on: across lanes 15 | 16 and 31 | 32), (d, 0) for d <= 31 (the run
    lives in the pad and ends in the band's last lane), and for DNA the near misses in a (0, 63) of their own, last.  The batches
    share one text: every read's own record, a decoy record for every third, a record for verification's read in a band of pad"""
    rng = np.random.default_rng(seed + alphabet)
    by_band = {}
    for index, d in enumerate(RUNS if alphabet == DNA else AMINO_RUNS):
        for kind in "DI":
            edge, other = (Plant(rng, alphabet, kind, d, a, c) for a, c in _placements(kind, d, index))
            by_band.setdefault((0, 63), []).append(edge)
            by_band.setdefault((0, d), []).extend([edge, other] if d < 63 else [other])
            if d <= 15 and alphabet == DNA:
                by_band.setdefault((8, 15), []).append(edge if index % 2 else other)
                by_band.setdefault((24, 15), []).append(other if index % 2 else edge)
            if d <= 31 and alphabet == DNA:
                by_band.setdefault((d, 0), []).extend([edge, other] if d in (4, 17, 31) else [other if index % 2 else edge])
    groups = sorted(by_band.items()) + ([((0, 63), near_misses(rng))] if alphabet == DNA else [])
    records = []
    for (w, x), plants in groups:
        for p in plants:
            if p.s is None:
                p.s = len(records)
                records.append(p.record)
                if p.s % 3 == 0:
                    record, p.decoy_diagonal = p.decoy(rng)
                    p.decoy_s = len(records)
                    records.append(record)
            if not x and p.back is None:
                read, record = there_and_back(rng, p)
                p.back = (read, len(records))
                records.append(record)
    return [Batch(w, x, plants, alphabet, records) for (w, x), plants in groups]


def near_misses(rng):
    """under (1, 4, 6, 1) a run of d between flanks of a and c adds a + c - (6 + d) to nothing: a right flank of d + 5 loses to the
    clip behind the left flank, one of d + 6 ties with it and the smaller i wins: the clip; a left flank of d + 5 or d + 6 brings
    H <= 0 into the right flank, which therefore begins anew: the clip; one of d + 7 brings 1"""
    plants = []
    for d in (5, 17, 33):
        for kind in "DI":
            plants += [Plant(rng, DNA, kind, d, flank(d), d + 5, "right flank one short: clipped"),
                       Plant(rng, DNA, kind, d, flank(d), d + 6, "right flank ties: clipped"),
                       Plant(rng, DNA, kind, d, d + 5, flank(d), "left flank one short: clipped"),
                       Plant(rng, DNA, kind, d, d + 6, flank(d), "left flank ties: clipped"),
                       Plant(rng, DNA, kind, d, d + 7, flank(d), "left flank pays by one")]
    return plants


@contextlib.contextmanager
def shared_local():
    """af.local computed once per (read, record, band, scoring) for everything that restates through it inside the block: the
    affine call, the scoring call (whose duplicate slots have the same band) and the conditions"""
    plain, memo = af.local, _LOCAL_MEMO

    def local(R, T, lo, hi, scoring=af.DEFAULT, alphabet=DNA):
        key = (R, T, lo, hi, scoring, alphabet)
        if key not in memo:
            memo[key] = plain(R, T, lo, hi, scoring, alphabet)
        return memo[key]

    af.local = local
    try:
        yield local
    finally:
        af.local = plain


_LOCAL_MEMO = {}


def gap_runs(runs):
    return [(run, op) for run, op in runs if op in (af.OP_I, af.OP_D)]


def band_of(batch, r):
    """(R, T, lo, hi) of read r's own slot"""
    S, E, lo, hi = batch.case.status(r, batch.w, batch.x)
    return batch.case.read(r), bytes(batch.case.text[S:E]), lo, hi


# ---- the kernel's row, the scan written out ----
NEG = -(1 << 30)  # kBandNeg


def scan_model(R, T, lo, hi, scoring, alphabet, G, steps):
    """alignReadAffine + affineRow<G> (csrc/awfm_align_affine_kernel.h, awfm_band_kernel.h) over NumPy vectors of G lanes: lane k is
    diagonal lo + k, a lane carries H and F of the row before, F comes from lane k + 1, and E from the scan AS THE KERNEL RUNS IT --
    H~ + k e shifted by one lane, then for every step of `steps` "take the value `step` lanes below if k >= step and it is larger"
    -- with the five trace bits a cell and the kernel's walk back over them -> af.local's tuple"""
    ma, mm, o, e = scoring
    first = o + e
    n, L, width = len(R), len(T), hi - lo + 1
    assert width <= G
    if n == 0 or n + hi < 0 or lo + 1 > L:
        return 0, 0, 0, 0, 0, 0, []
    k = np.arange(G, dtype=np.int64)
    u_min, u_max = max(-lo, 0), L - lo
    text_letters = np.array([-2 if vc.letter(alphabet, c) is None else vc.letter(alphabet, c) for c in T], np.int64)
    in_band = k < width
    prev_h = np.where(in_band & (k >= u_min) & (k <= u_max), 0, NEG)
    prev_f = np.full(G, NEG, np.int64)
    best_h, best_i = np.zeros(G, np.int64), np.zeros(G, np.int64)
    trace = []
    for i in range(1, n + 1):
        u = i + k
        in_matrix = in_band & (u >= u_min) & (u <= u_max)
        at = lo + u - 1
        x = vc.letter(alphabet, R[i - 1])
        sub = ~(in_matrix & (at >= 0) & (text_letters[np.clip(at, 0, L - 1)] == (-1 if x is None else x)))
        up_h, up_f = np.append(prev_h[1:], NEG), np.append(prev_f[1:], NEG)
        M = prev_h + np.where(sub, -mm, ma)
        f_opens, f_extends = up_h - first, up_f - e
        F = np.maximum(f_opens, f_extends)
        tilde = np.where(in_matrix, np.maximum(np.maximum(M, F), 0), NEG)
        v = np.concatenate(([NEG], (tilde + k * e)[:-1]))
        for step in steps:
            other = np.concatenate((np.full(step, NEG, np.int64), v[:-step]))
            v = np.where((k >= step) & (other > v), other, v)
        E = v - (first - e) - k * e
        h = np.where(in_matrix, np.maximum(tilde, E), NEG)
        left_h = np.concatenate(([NEG], h[:-1]))
        source = np.where(~in_matrix | (h == 0), 0, np.where(M == h, np.where(sub, 2, 1), np.where(F == h, 3, 4)))
        trace.append((source, f_opens >= f_extends, E == left_h - first))
        better = h > best_h
        best_h, best_i = np.where(better, h, best_h), np.where(better, i, best_i)
        prev_h, prev_f = h, np.where(in_matrix, F, NEG)
    score = int(best_h.max())
    if score == 0:
        return 0, 0, 0, 0, 0, 0, []
    i = int(best_i[best_h == score].min())
    lane = int(np.flatnonzero((best_h == score) & (best_i == i))[0])
    read_end, text_end = i, lo + i + lane
    script, state, distance = [af.OP_S] * (n - i), 0, 0
    for _ in range(2 * n + 64):
        if i <= 0:
            break
        source, f_opens, e_opens = (int(bits[lane]) for bits in trace[i - 1])
        if state == 0:
            if source == 0:
                break
            if source <= 2:
                script.append(af.OP_X if source == 2 else af.OP_EQ)
                distance += source == 2
                i -= 1
                continue
            state = 1 if source == 3 else 2
        distance += 1
        if state == 1:
            script.append(af.OP_I)
            state = 0 if f_opens else 1
            i, lane = i - 1, lane + 1
        else:
            script.append(af.OP_D)
            state = 0 if e_opens else 2
            lane -= 1
    script += [af.OP_S] * i
    return score, distance, i, read_end, lo + i + lane, text_end, af.merge(reversed(script))


def all_steps(G):
    return [1 << b for b in range(G.bit_length() - 1)]


# ---- windows ----
WINDOW_RUNS = (2, 3, 4, 12, 13, 48, 100, 300)
WINDOW_MAX_LENGTH = 1024


def window_flank(d):
    return d + 12


class WindowPlant:
    """kind D: the window's characters [col, col + d) are missing from the read; kind I: d characters that match nothing stand in
    the read ahead of the window's character col, behind the read's first `a` characters.  The read's first character lies on the
    window's character col - a"""

    def __init__(self, name, kind, d, col, W, a=None, c=None):
        self.name, self.kind, self.d, self.col, self.W = name, kind, d, col, W
        self.a, self.c = a or window_flank(d), c or window_flank(d) + 1
        assert col - self.a >= 0 and col + (d if kind == "D" else 0) + self.c <= W, name


def window_plants():
    plants = []

    def add(what, kind, d, col, W, a=None, c=None):
        plants.append(WindowPlant(f"{d}{kind} {what}", kind, d, col, W, a, c))

    # a lane owns Q characters: the edges of lanes of 4, 8 and 12 meet at the multiples of 24; W <= 256 | 512 | 768: Q = 4 | 8 | 12
    for W, edge in ((250, 120), (500, 240), (740, 360)):
        for d in (2, 3, 4, 12, 13, 48, 100):
            if window_flank(d) + d // 2 <= edge - 2 and edge + d + window_flank(d) + 1 <= W:
                add(f"astride the lane edge at {edge} of {W}", "D", d, edge - max(d // 2, 1), W)
        add(f"from the lane edge at {edge} of {W} on", "D", 4, edge, W)
        add(f"up to the lane edge at {edge} of {W}", "D", 13, edge - 13, W)
        add(f"one character either side of the lane edge at {edge} of {W}", "D", 2, edge - 1, W)
    # a block is 64 Q characters: 256 (Q = 4), 512 (4, 8), 768 (4, 12), 1024 (4, 8), 1536 (4, 8, 12)
    for edge in (256, 512, 768):
        for d in (2, 3, 4, 12, 13, 48, 100):
            add(f"astride the block edge at {edge}", "D", d, edge - max(d // 2, 1), edge + 240)
        for d in (4, 13):
            add(f"from the block edge at {edge} on", "D", d, edge, edge + 240)
            add(f"up to the block edge at {edge}", "D", d, edge - d, edge + 240)
    add("astride the block edges at 1024", "D", 13, 1018, 1100)
    add("astride the block edge at 1536", "D", 13, 1530, 1700)
    add("over the whole block 768 .. 1024 of lanes of 4", "D", 300, 740, 1400)
    add("over twenty-five whole lanes of 12", "D", 300, 312, 1000, a=312)
    # insertions: rows a + 1 .. a + d carry F; the boundary rows are reloaded every 64, the read's words every 256
    for d in (2, 3, 4, 12, 13, 48):
        a = 64 - max(d // 2, 1) if 64 - max(d // 2, 1) >= window_flank(d) else 60
        add("astride rows 64 | 65 in the first block", "I", d, 100, 250, a=a)
        add("astride rows 64 | 65 in a later block", "I", d, 900, 1000, a=a)
    for d in (2, 3, 4, 12, 13, 48, 100):
        a = 256 - max(d // 2, 1)
        add("astride rows 256 | 257 in the first block of lanes of 12", "I", d, 300, 700, a=a)
        add("astride rows 256 | 257 in a later block", "I", d, 900, 1100, a=a)
    add("astride rows 320 | 321 .. 576 | 577", "I", 300, 900, 1300, a=312, c=313)
    return plants


def window_corpus(seed=79):
    """-> (ws.Case, the plants): every read in a window of its own of one record, the windows beginning at every offset mod 4"""
    rng = np.random.default_rng(seed)
    letters = letters_of(DNA)
    plants = window_plants()
    reads, windows, records = [], [], [b"acg"]
    for index, p in enumerate(plants):
        begin = 40 + index % 4
        body = bytearray(rng.choice(letters, begin + p.W + 60))
        at = begin + p.col
        if p.kind == "D":
            ahead, behind = body[at - 1], body[at + p.d]
            body[at:at + p.d] = bytes(rng.choice([v for v in letters if v != ahead], p.d))
            body[at] = int(rng.choice([v for v in letters if v not in (ahead, behind)]))
            read = bytes(body[at - p.a:at]) + bytes(body[at + p.d:at + p.d + p.c])
        else:
            read = bytes(body[at - p.a:at]) + b"n" * p.d + bytes(body[at:at + p.c])
        reads.append(read)
        records.append(bytes(body))
        windows.append((len(records) - 1, begin, begin + p.W))
    text, ends = ws.text_of(records)
    return ws.Case(reads, windows, text, ends), plants
