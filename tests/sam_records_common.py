"""What the tests of "SAM records" (include/awfm_gpu.h) share: a builder of hand-made batches, a plain-Python restatement of the
definition that works on the call's arrays alone (fields joined by tabs, Python integers), and a parser of SAM lines that
rebuilds the text under an alignment from SEQ, CIGAR and MD."""
import re

import numpy as np

TOO_LONG = 0xFFFFFFFC  # AWFM_VERIFY_TOO_LONG
NO_SLOT = 0xFFFFFFFF
NAMES = ("lineOffsets", "lineChars", "numUnaligned", "numOverflow")
OPTIONAL = ("qualities", "names", "md", "mappingQualities", "secondScores", "baseFlags", "properPairs")
RECORD_NAMES = (b"chr1", b"r2", b"", b"a_rather_long_record_name|with.punctuation")


def read(seq=b"ACGT", qual=None, name=b"q", score=7, nm=1, slot=0, records=(0, 1), begin=4, end=None, cigar=None, md=b"4", mapq=60, xs=0, flag=0):
    """one read of a hand-made batch; end: begin + len(seq) unless given; cigar: all M unless given"""
    seq = bytes(seq)
    return dict(seq=seq, qual=bytes(qual) if qual is not None else bytes(33 + (i * 7) % 60 for i in range(len(seq))), name=bytes(name), score=score,
                nm=nm, slot=slot, records=tuple(records), begin=begin, end=begin + len(seq) if end is None else end,
                cigar=(b"%dM" % len(seq) if seq else b"") if cigar is None else bytes(cigar), md=bytes(md), mapq=mapq, xs=xs, flag=flag)


def packed(strings, dtype=np.uint64):
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in strings]))).astype(dtype)
    return offsets, np.frombuffer(b"".join(strings), np.uint8).copy()


class Batch:
    """reads -> the arrays of struct AwFmSamInputs; `without`: the optional inputs that are NULL (OPTIONAL); proper: per pair;
    inverted: reads whose end offset is moved one byte before their begin"""

    def __init__(self, reads, C=2, paired=False, proper=None, without=(), record_names=RECORD_NAMES, inverted=()):
        self.reads, self.C, self.paired, self.n = list(reads), C, paired, len(reads)
        assert not paired or self.n % 2 == 0
        assert all(w in OPTIONAL for w in without)
        a = {}
        a["readOffsets"], a["readChars"] = packed([r["seq"] for r in reads])
        for r in inverted:
            assert 0 < r + 1 < self.n and a["readOffsets"][r] >= 1
            a["readOffsets"][r + 1] = a["readOffsets"][r] - np.uint64(1)
        a["qualities"] = packed([r["qual"] for r in reads])[1]
        assert a["qualities"].size == a["readChars"].size
        a["nameOffsets"], a["nameChars"] = packed([r["name"] for r in reads])
        a["recordNameOffsets"], a["recordNameChars"] = packed(record_names)
        a["sequences"] = np.array([(list(r["records"]) + [0] * C)[:C] for r in reads], np.uint32).reshape(self.n, C)
        for name, key, dtype in (("slots", "slot", np.uint32), ("scores", "score", np.uint32), ("editDistances", "nm", np.uint32),
                                 ("textBegins", "begin", np.uint64), ("textEnds", "end", np.uint64), ("mappingQualities", "mapq", np.uint8),
                                 ("secondScores", "xs", np.uint32), ("baseFlags", "flag", np.uint16)):
            a[name] = np.array([r[key] for r in reads], dtype)
        a["cigarOffsets"], a["cigarChars"] = packed([r["cigar"] for r in reads])
        a["mdOffsets"], a["mdChars"] = packed([r["md"] for r in reads])
        a["properPairs"] = np.array(proper if proper is not None else [0] * (self.n // 2), np.uint8)
        for w in without:
            for name in {"names": ("nameOffsets", "nameChars"), "md": ("mdOffsets", "mdChars")}.get(w, (w,)):
                a[name] = None
        self.arrays = a

    def cut(self, n):
        """the first n reads, as a batch of its own over the same arrays"""
        other = Batch.__new__(Batch)
        other.reads, other.C, other.paired, other.n = self.reads[:n], self.C, self.paired, n
        other.arrays = dict(self.arrays)
        for name in ("readOffsets", "nameOffsets", "cigarOffsets", "mdOffsets"):
            if other.arrays[name] is not None:
                other.arrays[name] = other.arrays[name][:n + 1].copy()
        return other


def _aligned(a, r, C):
    score, slot = int(a["scores"][r]), int(a["slots"][r])
    if score == 0 or score >= TOO_LONG or slot >= C:
        return None
    s = int(a["sequences"][r, slot])
    if s >= len(a["recordNameOffsets"]) - 1 or int(a["readOffsets"][r + 1]) < int(a["readOffsets"][r]):
        return None
    return s


def _piece(offsets, chars, i):
    return chars[int(offsets[i]):int(offsets[i + 1])].tobytes()


def line_of(a, r, C, paired):
    """the SAM line of read r by the header's definition, from the arrays alone"""
    m = r ^ 1
    s, sm = _aligned(a, r, C), (_aligned(a, m, C) if paired else None)
    begin, end = int(a["readOffsets"][r]), int(a["readOffsets"][r + 1])
    n = max(end - begin, 0)
    qname = _piece(a["nameOffsets"], a["nameChars"], r) if a["nameOffsets"] is not None else b"%d" % (r // 2 if paired else r)
    flag = int(a["baseFlags"][r]) if a["baseFlags"] is not None else 0
    flag |= 0x4 if s is None else 0
    if paired:
        flag |= 0x1 | (0x80 if r & 1 else 0x40)
        if a["properPairs"] is not None and a["properPairs"][r // 2] and s is not None and sm is not None:
            flag |= 0x2
        flag |= 0x8 if sm is None else 0
        if a["baseFlags"] is not None and int(a["baseFlags"][m]) & 0x10:
            flag |= 0x20
    record = lambda i: _piece(a["recordNameOffsets"], a["recordNameChars"], i)  # noqa: E731
    if s is not None:
        place, rname, pos = s, record(s), int(a["textBegins"][r]) + 1
    elif sm is not None:
        place, rname, pos = sm, record(sm), int(a["textBegins"][m]) + 1
    else:
        place, rname, pos = None, b"*", 0
    mapq = 0 if s is None else 255 if a["mappingQualities"] is None else int(a["mappingQualities"][r])
    cigar = (_piece(a["cigarOffsets"], a["cigarChars"], r) if s is not None else b"") or b"*"
    if sm is None:
        rnext, pnext = b"*", 0
    else:
        rnext, pnext = (b"=" if place == sm else record(sm)), int(a["textBegins"][m]) + 1
    tlen = 0
    if s is not None and sm is not None and s == sm:
        mine, mates = int(a["textBegins"][r]), int(a["textBegins"][m])
        span = (max(int(a["textEnds"][r]), int(a["textEnds"][m])) - min(mine, mates)) % (1 << 64)
        span = span if mine < mates or (mine == mates and r % 2 == 0) else (-span) % (1 << 64)
        tlen = span - (1 << 64) if span >> 63 else span  # 64-bit two's complement
    seq = a["readChars"][begin:begin + n].tobytes() or b"*"
    qual = (a["qualities"][begin:begin + n].tobytes() if a["qualities"] is not None else b"") or b"*"
    fields = [qname, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, rnext, b"%d" % pnext, b"%d" % tlen, seq, qual]
    if s is not None:
        fields += [b"NM:i:%d" % int(a["editDistances"][r]), b"AS:i:%d" % int(a["scores"][r])]
        if a["secondScores"] is not None:
            fields.append(b"XS:i:%d" % int(a["secondScores"][r]))
        if a["mdOffsets"] is not None and _piece(a["mdOffsets"], a["mdChars"], r):
            fields.append(b"MD:Z:" + _piece(a["mdOffsets"], a["mdChars"], r))
    return b"\t".join(fields) + b"\n"


def lines_of(batch):
    return [line_of(batch.arrays, r, batch.C, batch.paired) for r in range(batch.n)]


def expected(batch, capacity=None, arena=True, fill=0, unaligned_before=0, overflow_before=0):
    """every output of the call on the batch, by the restatement"""
    lines = lines_of(batch)
    offsets = np.concatenate(([0], np.cumsum([len(x) for x in lines]))).astype(np.uint64)
    capacity = int(offsets[-1]) if capacity is None else capacity
    chars, overflow = np.full(capacity, fill, np.uint8), 0
    for r, x in enumerate(lines):
        if int(offsets[r + 1]) <= capacity:
            chars[int(offsets[r]):int(offsets[r + 1])] = np.frombuffer(x, np.uint8)
        else:
            overflow += 1
    unaligned = sum(_aligned(batch.arrays, r, batch.C) is None for r in range(batch.n))
    return dict(lineOffsets=offsets, lineChars=chars, numUnaligned=unaligned_before + unaligned, numOverflow=overflow_before + (overflow if arena else 0))


def assert_same(got, want, names=NAMES, what=""):
    for name in names:
        if name.startswith("num"):
            assert int(got[name]) == int(want[name]), (what, name, got[name], want[name])
            continue
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError((what, name, "first difference at", at, g[max(at - 20, 0):at + 20].tobytes(), w[max(at - 20, 0):at + 20].tobytes()))


# ---- the hand-made batches ----
def unaligned_reads():
    """one read per reason a read is UNALIGNED, beside a read that is fine; the inverted one is made by Batch(inverted=...)"""
    return [read(b"ACGTA", name=b"fine"), read(b"ACG", name=b"score0", score=0), read(b"ACGTT", name=b"tooLong", score=TOO_LONG),
            read(b"AC", name=b"almostTooLong", score=TOO_LONG - 1), read(b"ACGTAC", name=b"noSlot", slot=NO_SLOT), read(b"A", name=b"slotC", slot=2),
            read(b"ACGTACG", name=b"noRecord", records=(len(RECORD_NAMES), 0)), read(b"ACGT", name=b"lastRecord", records=(len(RECORD_NAMES) - 1, 0)),
            read(b"ACGTACGTA", name=b"inverted"), read(b"ACGTAC", name=b"afterInverted")]


UNALIGNED_INVERTED = (8,)
UNALIGNED_COUNT = 6  # score0, tooLong, noSlot, slotC, noRecord, inverted


def boundary_reads():
    """values at the decimal boundaries, lengths 0 to 5, empty strings; an even number of reads"""
    reads = []
    for i, begin in enumerate((8, 9, 98, 99, (1 << 32) - 2, (1 << 32) - 1, (1 << 40) - 1, 0)):  # POS 9 10 99 100 2^32-1 2^32 2^40 1
        reads.append(read(b"ACGTN"[:i % 6], begin=begin, name=b"pos%d" % i, records=(i % 3, 0)))
    for i, mapq in enumerate((0, 9, 10, 254, 255)):
        reads.append(read(b"acgtacg"[:3 + i], mapq=mapq, name=b"mapq%d" % mapq, xs=i))
    for nm, score in ((0, 1), ((1 << 24) - 1, (1 << 24) - 1), (5, 0), (0xFFFFFFFF, TOO_LONG - 1)):
        reads.append(read(b"TTTTT", nm=nm, score=score, xs=score // 2, name=b"nm"))
    for flag in (0, 0x10, 0x100, 0x800, 4095):
        reads.append(read(b"GG", flag=flag, name=b"flag%d" % flag))
    reads += [read(b"", name=b"empty"), read(b"", name=b"emptyUnaligned", score=0), read(b"ACGT", cigar=b"", md=b"", name=b"noStrings"),
              read(b"ACGT", cigar=b"2M1I1M", md=b"", name=b"noMd"), read(b"ACGT", cigar=b"", md=b"4", name=b""), read(b"A" * 151, name=b"x" * 40)]
    return reads + ([read(b"C")] if len(reads) % 2 else [])


def pair_reads():
    """pairs in the four aligned / unaligned combinations, in one record and in two, the tie on textBegins, spans of 2^40, mates on
    the other strand -> (reads, proper)"""
    big = 1 << 40
    pairs = [
        (read(b"ACGTA", begin=100, name=b"p0"), read(b"TTGCA", begin=300, name=b"p0", flag=0x10), 1),        # proper, same record
        (read(b"ACGTA", begin=300, name=b"p1", flag=0x10), read(b"TTGCA", begin=100, name=b"p1"), 1),        # the odd read is leftmost
        (read(b"ACGTA", begin=50, name=b"tie"), read(b"TTGCATT", begin=50, name=b"tie"), 1),                 # tie: the even read is first
        (read(b"ACGTA", begin=50, end=60, name=b"tie2"), read(b"TT", begin=50, end=52, name=b"tie2"), 0),    # tie, the even read ends last
        (read(b"ACGTA", begin=7, name=b"two"), read(b"TTGCA", begin=9, records=(1, 0), name=b"two"), 1),     # two records: RNEXT a name, TLEN 0
        (read(b"ACGTA", begin=7, name=b"sameName", slot=1, records=(3, 0)), read(b"TTGCA", begin=9, name=b"sameName"), 0),  # slot 1 names record 0
        (read(b"ACGTA", begin=5, name=b"half"), read(b"TTGCA", score=0, name=b"half", flag=0x10), 1),        # the mate is unaligned: proper is dropped
        (read(b"ACGTA", score=0, name=b"half2"), read(b"TTGCA", begin=(1 << 32) - 1, records=(3, 0), name=b"half2"), 1),
        (read(b"ACGTA", score=0, name=b"none"), read(b"", score=0, name=b"none"), 1),                        # both unaligned
        (read(b"ACGTA", begin=5, name=b"big"), read(b"TTGCA", begin=big, end=5 + big, name=b"big"), 0),      # TLEN +-2^40
        (read(b"ACGTA", begin=big, end=5 + big, name=b"big2"), read(b"TTGCA", begin=5, name=b"big2"), 0),
        (read(b"ACGTA", begin=5, end=5, name=b"zero"), read(b"TTGCA", begin=5, end=5, name=b"zero"), 1),      # TLEN 0 in one record
        (read(b"ACGTA", begin=9, end=2, name=b"wrapped"), read(b"TTGCA", begin=9, end=1, name=b"wrapped"), 0),  # e < b: two's complement
    ]
    return [r for a, b, _ in pairs for r in (a, b)], [p for _, _, p in pairs]


def hand_batch(paired, without=(), count=204):
    """the three lists above, then plain reads up to `count` (QNAME numbers pass 9 / 10 and 99 / 100, paired too)"""
    pairs, proper = pair_reads()
    reads = pairs + unaligned_reads()
    inverted = tuple(len(pairs) + r for r in UNALIGNED_INVERTED)
    reads += boundary_reads()
    assert len(reads) % 2 == 0
    rng = np.random.default_rng(3)
    while len(reads) < count:
        length = int(rng.choice((0, 1, 3, 4, 5, 150, 151)))
        seq = rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), length).tobytes()
        reads.append(read(seq, begin=int(rng.integers(0, 1000)), records=(int(rng.integers(0, 5)), 1), score=int(rng.integers(0, 3)) * 50,
                          md=b"%d" % length, name=b"read%d" % len(reads), mapq=int(rng.integers(0, 61)), flag=int(rng.choice((0, 0x10)))))
    proper = proper + [int(v) for v in rng.integers(0, 2, len(reads) // 2 - len(proper))]
    return Batch(reads, C=2, paired=paired, proper=proper, without=without, inverted=inverted)


def mixed_batch(seed, n, paired=False, without=(), C=3, lengths=(0, 1, 3, 4, 5, 150, 151), long_read=None):
    """n random reads of the given lengths, mixed; long_read: (place, length) of one long read"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTNacgtn", np.uint8)
    reads = []
    for r in range(n):
        length = long_read[1] if long_read and long_read[0] == r else int(rng.choice(lengths))
        seq = rng.choice(letters, length).tobytes()
        kind = int(rng.integers(0, 8))
        reads.append(read(seq, qual=rng.integers(33, 127, length).astype(np.uint8).tobytes(), name=b"r%d/%d" % (r // 2, r % 2) if r % 5 else b"",
                          score=0 if kind == 0 else int(rng.integers(1, 1 << int(rng.integers(1, 25)))), nm=int(rng.integers(0, 1 << int(rng.integers(1, 25)))),
                          slot=int(rng.integers(0, C + (1 if kind == 1 else 0))), records=tuple(int(v) for v in rng.integers(0, len(RECORD_NAMES) + (1 if kind == 2 else 0), C)),
                          begin=int(rng.integers(0, 1 << int(rng.integers(1, 41)))), cigar=(b"%dM" % length if length and kind != 3 else b""),
                          md=b"" if kind == 4 else b"%dA%d" % (length // 2, length - length // 2), mapq=int(rng.integers(0, 256)),
                          xs=int(rng.integers(0, 1000)), flag=int(rng.integers(0, 4096))))
    return Batch(reads, C=C, paired=paired, proper=[int(v) for v in rng.integers(0, 2, n // 2)], without=without)


# ---- a parser, for the end-to-end tests ----
def parse(line):
    assert line.endswith(b"\n") and line.count(b"\n") == 1, line
    fields = line[:-1].split(b"\t")
    assert len(fields) >= 11, line
    record = dict(zip(("qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual"), fields))
    for name in ("flag", "pos", "mapq", "pnext", "tlen"):
        assert re.fullmatch(rb"-?(0|[1-9][0-9]*)", record[name]), line
        record[name] = int(record[name])
    record["tags"] = {}
    for tag in fields[11:]:
        assert re.fullmatch(rb"[A-Z][A-Z]:[iZ]:.+", tag), line
        record["tags"][tag[:2].decode()] = int(tag[5:]) if tag[3:4] == b"i" else tag[5:]
    return record


def cigar_runs(cigar):
    runs = [(int(n), op) for n, op in re.findall(rb"([0-9]+)([MIDS=X])", cigar)]
    assert b"".join(b"%d%s" % (n, op) for n, op in runs) == cigar, cigar
    return runs


def text_under(seq, cigar, md):
    """the text an alignment lies on, rebuilt from SEQ, the classic CIGAR and MD; also checks that the CIGAR's read length is SEQ's"""
    runs = cigar_runs(cigar)
    assert sum(n for n, op in runs if op in b"MIS=X") == len(seq), (cigar, len(seq))
    assert re.fullmatch(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md), md
    aligned, i = bytearray(), 0  # the read's letters under M, a gap for every D
    for n, op in runs:
        if op in b"M=X":
            aligned += seq[i:i + n].upper()
        elif op == b"D":
            aligned += b"-" * n
        i += n if op != b"D" else 0
    out, at = bytearray(), 0
    for token in re.findall(rb"[0-9]+|\^[A-Z]+|[A-Z]", md):
        if token.isdigit():
            assert b"-" not in aligned[at:at + int(token)], (cigar, md)
            out += aligned[at:at + int(token)]
            at += int(token)
        elif token.startswith(b"^"):
            assert aligned[at:at + len(token) - 1] == b"-" * (len(token) - 1), (cigar, md)
            out += token[1:]
            at += len(token) - 1
        else:
            assert aligned[at:at + 1] not in (b"-", token), (cigar, md)
            out += token
            at += 1
    assert at == len(aligned), (cigar, md)
    return bytes(out)


def check_mates(first, second):
    """RNEXT / PNEXT / TLEN of two mates mirror each other"""
    for a, b in ((first, second), (second, first)):
        if b["flag"] & 0x4:
            assert a["rnext"] == b"*" and a["pnext"] == 0 and a["flag"] & 0x8, (a, b)
        else:
            assert a["pnext"] == b["pos"] and a["rnext"] == (b"=" if a["rname"] == b["rname"] else b["rname"]) and not a["flag"] & 0x8, (a, b)
    assert first["tlen"] == -second["tlen"] and first["qname"] == second["qname"]
    assert first["flag"] & 0x41 == 0x41 and second["flag"] & 0x81 == 0x81 and (first["flag"] & 0x2) == (second["flag"] & 0x2)


def check_end_to_end(e, lines, aligned, header):
    """every line of the pairs of pair_mates_common.EndToEnd parsed: the fields' forms, the CIGAR's read length, the text rebuilt
    from SEQ, CIGAR and MD against the record at POS, the mates against each other, the planted pairs proper at their places"""
    import pair_mates_common as pm
    assert header.count(b"@SQ") == len(e.records) and all(b"SN:r%d\tLN:%d\n" % (i, len(r)) in header for i, r in enumerate(e.records))
    records = [parse(x) for x in lines]
    assert len(records) == 2 * pm.E2E["pairs"]
    names = {b"r%d" % i: r for i, r in enumerate(e.records)}
    for r, rec in enumerate(records):
        assert rec["qname"] == b"%d" % (r // 2) and rec["seq"] == e.chars[int(e.offsets[r]):int(e.offsets[r + 1])].tobytes() and rec["qual"] == b"*"
        if rec["flag"] & 0x4:
            assert rec["cigar"] == b"*" and not rec["tags"] and rec["mapq"] == 0
            continue
        assert rec["cigar"] != b"*" and set(rec["tags"]) == {"NM", "AS", "XS", "MD"} and rec["tags"]["AS"] == int(aligned["scores"][r])
        under = text_under(rec["seq"], rec["cigar"], rec["tags"]["MD"])
        assert names[rec["rname"]][rec["pos"] - 1:rec["pos"] - 1 + len(under)].upper() == under, (r, rec)
        assert rec["pos"] - 1 == int(aligned["textBegins"][r]) and rec["pos"] - 1 + len(under) == int(aligned["textEnds"][r])
    for p, (s, at, mate_at, kind) in enumerate(e.plan):
        first, second = records[2 * p], records[2 * p + 1]
        check_mates(first, second)
        assert first["rname"] == second["rname"] == b"r%d" % s and not (first["flag"] | second["flag"]) & 0x4, (p, kind)
        assert bool(first["flag"] & 0x2) == (kind != "far"), (p, kind)
        lo, hi = min(first["pos"], second["pos"]) - 1, max(first["pos"] - 1 + 0, second["pos"] - 1)
        assert first["tlen"] > 0 and lo <= at + 5 and hi >= mate_at and abs(first["tlen"] - (mate_at + pm.E2E["length"] - at)) <= 12, (p, kind, first, second)
