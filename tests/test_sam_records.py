"""awfmSamRecords (include/awfm_gpu.h, "SAM records"), the host twin that is the definition of the device call, against the
plain-Python restatement of tests/sam_records_common.py and against lines written out by hand: every reason a read is unaligned,
reads of length 0, empty CIGAR and MD, names and qualities given and absent, every optional array NULL, pairs in all four
combinations, the decimal boundaries of every number, the capacities, the counters, guard bytes, every refusal; awfmRecordNames and
awfmSamHeader on a FASTA file whose headers carry descriptions; and a small text through the whole host pipeline, every line
parsed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_records_common as sm  # noqa: E402

PATTERN = 0xA5


def host(awfm, batch, **arguments):
    return awfm.sam_records_host(batch.arrays, max_candidates=batch.C, paired=batch.paired, fill=PATTERN, **arguments)


def check(awfm, batch, what="", **arguments):
    got = host(awfm, batch, **arguments)
    want = sm.expected(batch, arguments.get("line_capacity"), fill=PATTERN, unaligned_before=arguments.get("unaligned_before", 0),
                       overflow_before=arguments.get("overflow_before", 0))
    sm.assert_same(got, want, what=what)
    return got


def test_constants_are_the_headers(awfm):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "awfm_gpu.h")).read()
    assert "#define AWFM_SAM_PAIRED 1u" in header and awfm.SAM_PAIRED == 1
    assert "#define AWFM_VERIFY_TOO_LONG 0xFFFFFFFCu" in header and sm.TOO_LONG == 0xFFFFFFFC


def test_lines_written_out_by_hand(awfm):
    reads = [sm.read(b"ACGTA", qual=b"IIII#", name=b"pair", score=5, nm=0, begin=99, cigar=b"5M", md=b"5", mapq=60, xs=3, flag=0),
             sm.read(b"TTGCA", qual=b"#IIII", name=b"pair", score=4, nm=1, begin=299, cigar=b"2M1X2M", md=b"2C2", mapq=9, xs=0, flag=0x10),
             sm.read(b"GG", qual=b"!!", name=b"lone", score=0), sm.read(b"", qual=b"", name=b"mate", score=2, nm=0, begin=9, records=(1, 0), cigar=b"", md=b"")]
    paired = sm.Batch(reads, paired=True, proper=[1, 1])
    lines = [b"pair\t99\tchr1\t100\t60\t5M\t=\t300\t205\tACGTA\tIIII#\tNM:i:0\tAS:i:5\tXS:i:3\tMD:Z:5\n",
             b"pair\t147\tchr1\t300\t9\t2M1X2M\t=\t100\t-205\tTTGCA\t#IIII\tNM:i:1\tAS:i:4\tXS:i:0\tMD:Z:2C2\n",
             b"lone\t69\tr2\t10\t0\t*\t=\t10\t0\tGG\t!!\n",
             b"mate\t137\tr2\t10\t60\t*\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:2\tXS:i:0\n"]
    assert sm.lines_of(paired) == lines
    got = host(awfm, paired)
    assert awfm.strings_of(got["lineOffsets"], got["lineChars"]) == lines and got["numUnaligned"] == 1 and got["numOverflow"] == 0
    single = sm.Batch(reads, without=("names", "qualities", "mappingQualities", "secondScores", "md", "baseFlags", "properPairs"))
    lines = [b"0\t0\tchr1\t100\t255\t5M\t*\t0\t0\tACGTA\t*\tNM:i:0\tAS:i:5\n", b"1\t0\tchr1\t300\t255\t2M1X2M\t*\t0\t0\tTTGCA\t*\tNM:i:1\tAS:i:4\n",
             b"2\t4\t*\t0\t0\t*\t*\t0\t0\tGG\t*\n", b"3\t0\tr2\t10\t255\t*\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:2\n"]
    assert sm.lines_of(single) == lines
    got = host(awfm, single)
    assert awfm.strings_of(got["lineOffsets"], got["lineChars"]) == lines


def test_every_reason_a_read_is_unaligned(awfm):
    for paired in (False, True):
        batch = sm.Batch(sm.unaligned_reads(), paired=paired, inverted=sm.UNALIGNED_INVERTED)
        got = check(awfm, batch, what=("unaligned", paired), unaligned_before=100)
        assert got["numUnaligned"] == 100 + sm.UNALIGNED_COUNT
        lines = awfm.strings_of(got["lineOffsets"], got["lineChars"])
        flags = [int(x.split(b"\t")[1]) & 0x4 for x in lines]
        assert flags == [0, 4, 4, 0, 4, 4, 4, 0, 4, 0]
        assert lines[8].split(b"\t")[9] == b"*"  # inverted offsets: a read of length 0


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_hand_made_batches_with_every_optional_array_null_in_turn(awfm, paired):
    for without in [()] + [(w,) for w in sm.OPTIONAL] + [sm.OPTIONAL]:
        batch = sm.hand_batch(paired, without)
        got = check(awfm, batch, what=("hand", paired, without))
        lines = awfm.strings_of(got["lineOffsets"], got["lineChars"])
        if without == ("names",):  # QNAME numbers pass 9 / 10 and 99 / 100
            assert [x.split(b"\t")[0] for x in lines] == [b"%d" % (r // 2 if paired else r) for r in range(batch.n)] and batch.n // 2 > 100
        if not without and paired:
            spans = {int(x.split(b"\t")[8]) for x in lines}
            assert {0, 1 << 40, -(1 << 40), 205, -205, 7, -7} <= spans
        if not without and not paired:
            fields = [x.split(b"\t") for x in lines]
            assert {b"9", b"10", b"99", b"100", b"%d" % ((1 << 32) - 1), b"%d" % (1 << 32), b"%d" % (1 << 40)} <= {f[3] for f in fields}
            assert {b"0", b"9", b"10", b"254", b"255"} <= {f[4] for f in fields} and b"4095" in {f[1] for f in fields}
            tags = {t for f in fields for t in f[11:]}
            assert {b"NM:i:0", b"NM:i:%d" % ((1 << 24) - 1), b"AS:i:%d" % ((1 << 24) - 1), b"AS:i:1", b"NM:i:4294967295"} <= tags


def test_random_batches(awfm):
    for seed, paired in ((1, False), (2, True)):
        check(awfm, sm.mixed_batch(seed, 300, paired), what=("mixed", paired))
    check(awfm, sm.mixed_batch(3, 5, long_read=(2, 20000)), what="long")


def test_results_for_1_and_16_threads_are_equal(awfm):
    batch = sm.mixed_batch(4, 1 << 12, paired=True)
    one, many = host(awfm, batch, threads=1), host(awfm, batch, threads=16)
    sm.assert_same(one, many, what="threads")
    sm.assert_same(one, sm.expected(batch, fill=PATTERN), what="threads")


def test_capacities(awfm):
    batch = sm.hand_batch(True)
    offsets = sm.expected(batch)["lineOffsets"]
    total = int(offsets[-1])
    middle = (int(offsets[100]) + int(offsets[101])) // 2
    for capacity in (total, total - 1, middle, int(offsets[100]), 0):
        got = check(awfm, batch, what=("capacity", capacity), line_capacity=capacity, overflow_before=7)
        assert got["numOverflow"] == 7 + sum(int(v) > capacity for v in offsets[1:])
    only = host(awfm, batch, outputs=("lineOffsets", "numUnaligned", "numOverflow"), overflow_before=7)
    assert np.array_equal(only["lineOffsets"], offsets) and only["numOverflow"] == 7  # offsets only: no line is missed


def test_no_byte_outside_the_arena_is_written(awfm):
    batch = sm.hand_batch(False)
    want = sm.expected(batch)
    total = int(want["lineOffsets"][-1])
    for capacity in (total, total - 1, total // 2):
        memory = np.full(total + 128, PATTERN, np.uint8)
        offsets = np.zeros(batch.n + 1, np.uint64)
        held = {name: np.ascontiguousarray(a) for name, a in batch.arrays.items() if a is not None}
        sin = awfm.sam_inputs(held["readChars"].size, len(sm.RECORD_NAMES), **{name: a.ctypes.data for name, a in held.items()})
        sout = awfm.sam_outputs(lineOffsets=offsets.ctypes.data, lineChars=memory.ctypes.data + 64, lineCapacity=capacity)
        from avxwindowfmindex_amd import _lib
        assert _lib.lib().awfmSamRecords(C.byref(sin), batch.n, batch.C, 0, C.byref(sout), 3) == awfm.AwFmSuccess
        cut = sm.expected(batch, capacity, fill=PATTERN)
        assert np.array_equal(memory[64:64 + capacity], cut["lineChars"]) and (memory[:64] == PATTERN).all() and (memory[64 + capacity:] == PATTERN).all()


def test_every_output_null_in_turn_and_no_reads(awfm):
    batch = sm.hand_batch(True)
    want = sm.expected(batch, fill=PATTERN)
    for names in (("lineOffsets",), ("numUnaligned",), ("numOverflow",), ("lineOffsets", "lineChars"), ()):
        got = host(awfm, batch, outputs=names)
        assert sorted(got) == sorted(names)
        sm.assert_same(got, want, names=names, what=names)
    got = awfm.sam_records_host(batch.arrays, max_candidates=batch.C, num_reads=0, fill=PATTERN, line_capacity=16, unaligned_before=3, overflow_before=4)
    assert (got["lineOffsets"].view(np.uint8) == PATTERN).all() and (got["lineChars"] == PATTERN).all()  # numReads == 0 touches nothing
    assert got["numUnaligned"] == 3 and got["numOverflow"] == 4


def test_every_refusal(awfm):
    from avxwindowfmindex_amd import _lib
    batch = sm.hand_batch(True)
    held = {name: np.ascontiguousarray(a) for name, a in batch.arrays.items()}
    offsets, arena = np.zeros(batch.n + 1, np.uint64), np.zeros(1 << 16, np.uint8)

    def call(n=batch.n, slots=batch.C, flags=awfm.SAM_PAIRED, drop=(), records=len(sm.RECORD_NAMES), out=None, inputs=True):
        sin = awfm.sam_inputs(held["readChars"].size, records, **{name: a.ctypes.data for name, a in held.items() if name not in drop})
        sout = awfm.sam_outputs(lineOffsets=offsets.ctypes.data, lineChars=arena.ctypes.data, lineCapacity=arena.size) if out is None else out
        return _lib.lib().awfmSamRecords(C.byref(sin) if inputs else None, n, slots, flags, C.byref(sout) if sout is not False else None, 2)

    null, illegal = -4, awfm.AwFmIllegalPositionError
    assert "AwFmNullPtrError = -4" in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "AwFmIndex.h")).read().replace("  ", " ")
    assert call() == awfm.AwFmSuccess
    for name in ("readChars", "readOffsets", "sequences", "slots", "scores", "editDistances", "textBegins", "textEnds", "cigarOffsets", "cigarChars",
                 "recordNameOffsets", "recordNameChars"):
        assert call(drop=(name,)) == null, name
    assert call(drop=("recordNameOffsets", "recordNameChars"), records=0) == awfm.AwFmSuccess  # no record names: nobody is aligned
    for name in ("nameOffsets", "nameChars", "mdOffsets", "mdChars"):  # half a pair
        assert call(drop=(name,)) == null, name
    assert call(inputs=False) == null and call(out=False) == null
    assert call(out=awfm.sam_outputs(lineChars=arena.ctypes.data, lineCapacity=arena.size)) == null  # an arena without its offsets
    for slots in (0, 17):
        assert call(slots=slots) == illegal
    assert call(flags=2) == illegal and call(flags=3) == illegal and call(flags=1 << 31) == illegal
    assert call(n=batch.n - 1) == illegal and call(n=batch.n - 1, flags=0) == awfm.AwFmSuccess  # odd and paired
    assert call(n=1 << 32, flags=0) == illegal and call(n=1 << 32) == illegal
    assert call(n=0, drop=("readChars",), slots=0, flags=7) == awfm.AwFmSuccess  # no reads: nothing is looked at
    # the order: a missing array before a bad number
    assert call(drop=("slots",), slots=0) == null and call(out=awfm.sam_outputs(lineChars=arena.ctypes.data), flags=2) == null


FASTA = (b">chr1 Homo sapiens chromosome 1, primary assembly\nACGTACGTAC\nGTAC\n"
         b">scaffold_2\tlength=9 tab after the name\nTTTTGGGGA\n"
         b">lonely\nACGTTGCAACGTTGCAAC\n"
         b">  leading blanks are skipped\nAC\n")


def test_record_names_and_sam_header(awfm, tmp_path):
    from avxwindowfmindex_amd import _lib
    path = tmp_path / "described.fa"
    path.write_bytes(FASTA)
    ix = awfm.create_index_from_fasta(str(path), awfm.AwFmAlphabetDna, 2, 2, file_src=str(tmp_path / "described.awfmi"))
    try:
        names = [b"chr1", b"scaffold_2", b"lonely", b"leading"]
        assert ix.header(0).startswith(b"chr1 Homo") or ix.header(0).startswith("chr1 Homo")
        offsets, chars = awfm.record_names(ix)
        assert awfm.strings_of(offsets, chars) == names
        want = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, length) for n, length in zip(names, (14, 9, 18, 2)))
        assert awfm.sam_header(ix) == want
        L = _lib.lib()
        # capacities: names and lines are written whole or not at all, nothing beyond the capacity, the sizes are the true ones
        for capacity in (0, 3, 4, 13, 14, len(b"".join(names)) - 1):
            memory, sized = np.full(64, PATTERN, np.uint8), np.zeros(5, np.uint64)
            assert L.awfmRecordNames(ix.ptr, sized.ctypes.data, memory.ctypes.data, capacity) == awfm.AwFmSuccess and np.array_equal(sized, offsets)
            fit = [n for i, n in enumerate(names) if int(offsets[i + 1]) <= capacity]
            assert memory[:len(b"".join(fit))].tobytes() == b"".join(fit) and (memory[len(b"".join(fit)):] == PATTERN).all()
        for capacity in (0, 21, 22, 40, len(want) - 1):
            memory = np.full(len(want) + 8, PATTERN, np.uint8)
            assert L.awfmSamHeader(ix.ptr, memory.ctypes.data, capacity) == len(want)
            lines, fit = want.splitlines(keepends=True), 0
            while fit < len(lines) and len(b"".join(lines[:fit + 1])) <= capacity:
                fit += 1
            assert memory[:len(b"".join(lines[:fit]))].tobytes() == b"".join(lines[:fit]) and (memory[len(b"".join(lines[:fit])):] == PATTERN).all()
        assert L.awfmRecordNames(None, offsets.ctypes.data, None, 0) == -4 and L.awfmRecordNames(ix.ptr, None, None, 0) == -4
        assert L.awfmSamHeader(None, None, 0) == 0
    finally:
        ix.dealloc()
    plain = awfm.create_index(np.frombuffer(b"acgtacgtacgtacgt", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    try:  # an index without a FASTA trailer has no names
        assert _lib.lib().awfmRecordNames(plain.ptr, np.zeros(2, np.uint64).ctypes.data, None, 0) == awfm.AwFmUnsupportedVersionError
        assert awfm.sam_header(plain) == b""
    finally:
        plain.dealloc()


def test_end_to_end_through_the_host_pipeline(awfm, tmp_path):
    import pair_mates_common as pm
    e = pm.EndToEnd(awfm, tmp_path)
    try:
        side = pm.HostSide(awfm, e)
        _, second, aligned = e.loop(side)
        scored = side.score(e.final_slots)
        strings = awfm.alignment_strings_host(e.final_slots["sequences"], second["pairSlots"], aligned["textBegins"], aligned["numOps"], aligned["ops"],
                                              e.text, e.ends, classic=True)
        assert strings["numSkipped"] == 0 and strings["numOverflow"] == 0
        name_offsets, name_chars = awfm.record_names(e.ix)
        arrays = dict(readChars=e.chars, readOffsets=e.offsets, recordNameOffsets=name_offsets, recordNameChars=name_chars,
                      sequences=e.final_slots["sequences"], slots=second["pairSlots"], scores=aligned["scores"], editDistances=aligned["editDistances"],
                      textBegins=aligned["textBegins"], textEnds=aligned["textEnds"], cigarOffsets=strings["cigarOffsets"], cigarChars=strings["cigarChars"],
                      mdOffsets=strings["mdOffsets"], mdChars=strings["mdChars"], mappingQualities=second["mappingQualities"],
                      secondScores=scored["secondScores"], properPairs=second["properPairs"])
        got = awfm.sam_records_host(arrays, paired=True, threads=16)
        assert got["numUnaligned"] == 0 and got["numOverflow"] == 0
        sm.check_end_to_end(e, awfm.strings_of(got["lineOffsets"], got["lineChars"]), aligned, awfm.sam_header(e.ix))
    finally:
        e.close()
