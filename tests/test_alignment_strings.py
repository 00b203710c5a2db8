"""awfmAlignmentStrings (include/awfm_gpu.h, "alignment strings"), the host twin that is the definition of the device call, against
the plain-Python restatement of tests/alignment_strings_common.py and the definition's hand values: both CIGAR forms, MD:Z, the
decimal edges, NONE and every SKIPPED condition, all byte values as text letters, capacities, NULL outputs, counters and the
parameter rules.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alignment_strings_common as sc  # noqa: E402

FILL = 0xA5
NAMES = ("cigarOffsets", "cigarChars", "mdOffsets", "mdChars", "numSkipped", "numOverflow")
_CASES = {}


def case_of(kind, alphabet=sc.DNA):
    """the cases and their restatements, computed once"""
    key = (kind, alphabet)
    if key not in _CASES:
        if kind == "hand":
            case, skipped = sc.hand_case(), []
        elif kind == "edges":
            case, skipped = sc.edge_case(alphabet), []
        elif kind == "skipped":
            case, skipped = sc.skipped_case(alphabet)
        else:
            case, skipped = sc.random_case(91 + alphabet, 700, alphabet), None
        _CASES[key] = (case, skipped, {classic: sc.expected(case, classic, fill=FILL) for classic in (False, True)})
    return _CASES[key]


def host(awfm, case, **arguments):
    arguments.setdefault("fill", FILL)
    return awfm.alignment_strings_host(text=case.text, sequence_ends=case.ends, alphabet=case.alphabet, **case.arrays(), **arguments)


def test_constants_are_the_headers(awfm):
    assert (sc.DNA, sc.AMINO) == (awfm.AwFmAlphabetDna, awfm.AwFmAlphabetAmino) and awfm.STRINGS_CIGAR_M == 1
    assert sc.NO_SLOT == awfm.CHAINS_NO_SLOT and {k: v.encode() for k, v in awfm.ALIGN_OP_LETTERS.items()} == sc.LETTERS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "awfm_gpu.h")).read()
    assert "#define AWFM_STRINGS_CIGAR_M 1u" in header and "#define AWFM_ALIGN_MAX_LENGTH (1u << 16)" in header and "#define AWFM_ALIGN_MAX_OPS 4096u" in header


@pytest.mark.parametrize("classic", [False, True])
def test_hand_values(awfm, classic):
    case, _, want = case_of("hand")
    for r, h in enumerate(sc.HAND):  # the restatement gives the definition's table ...
        assert want[classic]["strings"][r] == (h[4] if classic else h[3], h[5]), (r, want[classic]["strings"][r])
    got = host(awfm, case, classic=classic)  # ... and so does the twin
    sc.assert_same(got, want[classic])
    assert awfm.strings_of(got["cigarOffsets"], got["cigarChars"]) == [h[4] if classic else h[3] for h in sc.HAND]
    assert awfm.strings_of(got["mdOffsets"], got["mdChars"]) == [h[5] for h in sc.HAND]
    assert got["numSkipped"] == 0 and got["numOverflow"] == 0


@pytest.mark.parametrize("alphabet", [sc.DNA, sc.AMINO])
@pytest.mark.parametrize("classic", [False, True])
def test_decimal_edges_ends_and_merging(awfm, alphabet, classic):
    case, _, want = case_of("edges", alphabet)
    assert want[classic]["numSkipped"] == 0 and all(s[0] and s[1] for s in want[classic]["strings"])  # every read of the list is valid
    sc.assert_same(host(awfm, case, classic=classic), want[classic])
    # '=', X, '=' is one M; nothing merges across I, D or S
    r = next(i for i, read in enumerate(case.reads) if read.runs == sc.script("3= 1I 2X 1D 4= 1S"))
    assert want[True]["strings"][r][0] == b"3M1I2M1D4M1S" and want[False]["strings"][r][0] == b"3=1I2X1D4=1S"
    r = next(i for i, read in enumerate(case.reads) if read.runs == sc.script("1X 1= 1X 1= 1X"))
    assert want[True]["strings"][r][0] == b"5M"
    for edge in sc.DECIMAL_EDGES:  # the numbers themselves stand in the strings
        assert any(str(edge).encode() + b"D" in s[0] for s in want[False]["strings"]), edge
        if edge <= sc.MAX_LENGTH:
            assert any(s == (str(edge).encode() + b"=", str(edge).encode()) for s in want[False]["strings"]), edge
            assert any(s[0] == str(edge).encode() + b"M" for s in want[True]["strings"]), edge


@pytest.mark.parametrize("alphabet", [sc.DNA, sc.AMINO])
def test_every_skipped_condition_beside_reads_that_are_fine(awfm, alphabet):
    case, skipped, want = case_of("skipped", alphabet)
    per_read = [sc.read_strings(case, r, False) for r in range(case.num_reads)]
    assert [r for r, s in enumerate(per_read) if s == "skipped"] == skipped and per_read[-2] is None
    assert all(isinstance(per_read[r - 1], tuple) and isinstance(per_read[r + 1], tuple) for r in skipped)
    for classic in (False, True):
        got = host(awfm, case, classic=classic)
        sc.assert_same(got, want[classic])
        assert got["numSkipped"] == len(skipped)
    # nothing of the text is read through a skipped read: in a copy of the text EVERY byte that no valid read's script covers is
    # changed -- the bytes under the skipped scripts among them -- and every output stays what it was
    covered = np.zeros(len(case.text), bool)
    for r, strings in enumerate(per_read):
        if isinstance(strings, tuple):
            covered[sc.text_under(case, r)] = True
    poisoned = sc.Case(case.reads, case.text, case.ends, alphabet, C=case.C, max_ops=case.max_ops)
    poisoned.text[~covered] ^= 0x5F
    under = [sc.text_under(case, r) for r in skipped]
    changed = [u is not None and len(u) > 0 and not covered[u].all() for u in under]
    whole = [u is not None and len(u) > 0 and not covered[u].any() for u in under]
    # at least the eight reads at position 1000 that name a slot and a record: every byte under them is changed; the reads past a
    # record's end share bytes with valid neighbours, the others name no slot or record or begin beyond the text
    assert sum(whole) >= 8 and sum(changed) > sum(whole), (changed, whole)
    for classic in (False, True):
        sc.assert_same(host(awfm, poisoned, classic=classic), want[classic])
    assert not np.array_equal(poisoned.text, case.text) and sc.expected(poisoned, fill=FILL)["strings"] == want[False]["strings"]


def test_text_is_not_read_beyond_its_length(awfm):
    """the last record's end lies beyond the text: its reads are skipped, the others are not"""
    case, _, _ = case_of("hand")
    short = sc.Case(case.reads, case.text[:-3], case.ends, sc.DNA, C=case.C, max_ops=case.max_ops)
    want = sc.expected(short, fill=FILL)
    assert want["numSkipped"] == 1 and want["strings"][-1] == (b"", b"") and want["strings"][0][0]
    sc.assert_same(host(awfm, short), want)


@pytest.mark.parametrize("alphabet", [sc.DNA, sc.AMINO])
def test_letter_of_every_byte_value(awfm, alphabet):
    text = bytes(range(256)) * 2
    reads = [sc.Read(0, c, [(1, sc.X)]) for c in range(256)] + [sc.Read(0, c, [(1, sc.EQ), (1, sc.D), (1, sc.EQ)]) for c in range(256)]
    reads += [sc.Read(0, 0, [(256, sc.X)]), sc.Read(0, 3, [(1, sc.S), (256, sc.D), (2, sc.I)])]
    case = sc.Case(reads, text, None, alphabet, C=1, max_ops=3)
    want = sc.expected(case, fill=FILL)
    table = sc.letter_table(alphabet)
    other = b"X" if alphabet == sc.AMINO else b"N"
    assert table[ord("a")] == ord("A") and table[ord("z")] == ord("Z") and table[ord("Q")] == ord("Q") and bytes([table[ord("$")]]) == other
    assert sum(1 for c in range(256) if bytes([table[c]]) == other) >= 256 - 52
    for c in range(256):
        assert want["strings"][c][1] == b"0" + table[c:c + 1] + b"0" and want["strings"][256 + c][1] == b"1^" + bytes([table[(c + 1) % 256]]) + b"1"
    sc.assert_same(host(awfm, case), want)


def test_no_record_table_is_one_sequence(awfm):
    case = sc.Case([sc.Read(0, 2, sc.script("2= 1X")), sc.Read(0, 2, sc.script("2= 1X"), sequence=1), sc.Read(0, 8, sc.script("2= 1X"))],
                   b"ACGTACGTAC", None, sc.DNA)
    want = sc.expected(case, fill=FILL)
    assert want["strings"][0] == (b"2=1X", b"2A0") and want["numSkipped"] == 2
    sc.assert_same(host(awfm, case), want)


@pytest.mark.parametrize("classic", [False, True])
def test_random_scripts(awfm, classic):
    for alphabet in (sc.DNA, sc.AMINO):
        case, _, want = case_of("random", alphabet)
        assert 0 < want[classic]["numSkipped"] < case.num_reads // 4
        sc.assert_same(host(awfm, case, classic=classic, threads=1), want[classic])


THREADED_READS = 1 << 13  # the thread pool runs a loop of fewer than 4096 items on the calling thread (csrc/awfm_threads.c)


def test_results_for_1_and_16_threads_are_equal(awfm):
    """2^13 reads, so that 16 threads get a chunk of 512 each: skipped reads in every chunk, and capacities at which the reads
    that overflow fill whole chunks; the lengths pass, the writes and the per-thread counters against 1 thread and the restatement"""
    threads_source = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avxwindowfmindex_amd", "csrc", "awfm_threads.c")).read()
    assert "numThreads <= 1 || n < 4096" in threads_source and THREADED_READS >= 4096
    case = sc.random_case(93, THREADED_READS, sc.DNA, C=4, max_ops=16, text_length=1 << 15, num_records=7)
    full = sc.expected(case, fill=FILL)
    chunk = THREADED_READS // 16
    per_read = [sc.read_strings(case, r, False) for r in range(case.num_reads)]
    assert all(any(s == "skipped" for s in per_read[c:c + chunk]) and any(isinstance(s, tuple) for s in per_read[c:c + chunk])
               for c in range(0, THREADED_READS, chunk))
    totals = int(full["cigarOffsets"][-1]), int(full["mdOffsets"][-1])
    for classic, cigar_capacity, md_capacity in ((False, totals[0], totals[1]), (True, None, None), (False, totals[0] // 2, totals[1] // 3),
                                                 (True, 0, totals[1]), (False, 0, 0)):
        want = sc.expected(case, classic, cigar_capacity, md_capacity, fill=FILL, skipped_before=5, overflow_before=6)
        results = [host(awfm, case, classic=classic, cigar_capacity=cigar_capacity, md_capacity=md_capacity, threads=threads, skipped_before=5,
                        overflow_before=6) for threads in (1, 16)]
        sc.assert_same(results[1], results[0], what=("16 threads against 1", classic, cigar_capacity, md_capacity))
        sc.assert_same(results[1], want, what=("16 threads against the restatement", classic, cigar_capacity, md_capacity))
    # at half the capacity the overflowing reads are those of the upper chunks, all of them
    assert sc.expected(case, False, totals[0] // 2, totals[1], fill=FILL)["numOverflow"] > sum(1 for s in per_read if isinstance(s, tuple)) // 3


def _last_with(strings, which):
    return max(r for r, s in enumerate(strings) if s[which])


def test_capacities(awfm):
    case, _, want = case_of("random")
    full = want[False]
    totals = int(full["cigarOffsets"][-1]), int(full["mdOffsets"][-1])
    for cigar_capacity, md_capacity in ((totals[0], totals[1]), (totals[0] - 1, totals[1]), (totals[0], totals[1] - 1), (totals[0] - 1, totals[1] - 1),
                                        (0, totals[1]), (totals[0], 0), (0, 0), (totals[0] // 2, totals[1] // 3), (totals[0] + 5, totals[1] + 9)):
        expect = sc.expected(case, False, cigar_capacity, md_capacity, fill=FILL, overflow_before=3)
        got = host(awfm, case, cigar_capacity=cigar_capacity, md_capacity=md_capacity, overflow_before=3)
        sc.assert_same(got, expect, what=(cigar_capacity, md_capacity))
        assert np.array_equal(got["cigarOffsets"], full["cigarOffsets"]) and np.array_equal(got["mdOffsets"], full["mdOffsets"])  # whatever the capacities are
    # one byte less: the last non-empty read is not written and is counted, the bytes before it are intact
    got = host(awfm, case, cigar_capacity=totals[0] - 1, md_capacity=totals[1])
    last = _last_with(full["strings"], 0)
    cut = int(full["cigarOffsets"][last])
    assert got["numOverflow"] == 1 and np.array_equal(got["cigarChars"][:cut], full["cigarChars"][:cut]) and (got["cigarChars"][cut:] == FILL).all()
    assert np.array_equal(got["mdChars"], full["mdChars"])
    # a read missing from both arenas is counted once
    got = host(awfm, case, cigar_capacity=0, md_capacity=0)
    assert got["numOverflow"] == sum(1 for s in full["strings"] if s[0])


def test_every_output_null_in_turn_and_alone(awfm):
    case, _, want = case_of("random")
    full = want[True]
    totals = dict(cigar_capacity=int(full["cigarOffsets"][-1]), md_capacity=int(full["mdOffsets"][-1]))
    for name in NAMES:
        got = host(awfm, case, classic=True, outputs=[name], **totals) if not name.endswith("Chars") else None
        if got is not None:  # alone (an arena cannot be: it needs its offsets)
            assert list(got) == [name]
            sc.assert_same(got, sc.expected(case, True, fill=FILL, cigar_arena=False, md_arena=False), names=[name], what=name)
        missing = [n for n in NAMES if n != name and not (name.endswith("Offsets") and n == name[:-7] + "Chars")]
        got = host(awfm, case, classic=True, outputs=missing, **totals)  # NULL in turn (its arena with it)
        assert sorted(got) == sorted(missing)
        sc.assert_same(got, full, names=missing, what=("without", name))
    # sizing: offsets without arenas, then arenas of exactly that size
    sized = host(awfm, case, outputs=["cigarOffsets", "mdOffsets"])
    assert int(sized["cigarOffsets"][-1]) == int(want[False]["cigarOffsets"][-1]) and int(sized["mdOffsets"][-1]) == totals["md_capacity"]
    none = host(awfm, case, outputs=[])
    assert none == {}


def test_counters_are_added_to(awfm):
    case, skipped, want = case_of("skipped")
    got = host(awfm, case, skipped_before=1000, overflow_before=(1 << 40) + 7, cigar_capacity=10, md_capacity=10 ** 6)
    expect = sc.expected(case, False, 10, 10 ** 6, fill=FILL, skipped_before=1000, overflow_before=(1 << 40) + 7)
    sc.assert_same(got, expect)
    assert got["numSkipped"] == 1000 + len(skipped) and got["numOverflow"] > (1 << 40) + 7


def test_parameter_rules(awfm):
    from avxwindowfmindex_amd import _lib
    import ctypes as C
    case, _, _ = case_of("hand")
    n = case.num_reads
    arrays = case.arrays()
    keep = {name: np.ascontiguousarray(a) for name, a in arrays.items()}
    offsets, chars, counter = np.full(n + 1, 7, np.uint64), np.full(64, FILL, np.uint8), np.full(1, 5, np.uint64)

    def call(num_reads=n, C_=case.C, max_ops=case.max_ops, flags=0, drop=None, text=case.text, ends=case.ends, num_records=None, out=None, no_out=False):
        fields = [None if name == drop else keep[name].ctypes.data for name in ("sequences", "slots", "text_begins", "num_ops", "ops")]
        sin = _lib.AwFmStringInputs(*fields)
        sout = awfm.string_outputs(**(dict(cigarOffsets=offsets.ctypes.data, numSkipped=counter.ctypes.data) if out is None else out))
        return _lib.lib().awfmAlignmentStrings(C.byref(sin), num_reads, C_, max_ops, flags, None if text is None else text.ctypes.data, len(case.text),
                                               None if ends is None else ends.ctypes.data, len(case.ends) if num_records is None else num_records,
                                               case.alphabet, None if no_out else C.byref(sout), 2)

    success, null, illegal = awfm.AwFmSuccess, sc.NULL_ERROR, awfm.AwFmIllegalPositionError
    assert call() == success and offsets[0] == 0 and counter[0] == 5
    offsets[:] = 7
    # numReads == 0 succeeds and touches nothing, whatever else is wrong
    assert call(num_reads=0, C_=0, max_ops=0, flags=99, drop="ops", no_out=True) == success and (offsets == 7).all() and counter[0] == 5
    for drop in ("sequences", "slots", "text_begins", "num_ops", "ops"):
        assert call(drop=drop) == null, drop
    assert call(no_out=True) == null and call(text=None) == null and call(ends=None) == null
    assert call(out=dict(cigarChars=chars.ctypes.data, cigarCapacity=64)) == null  # an arena without its offsets
    assert call(out=dict(mdChars=chars.ctypes.data, mdCapacity=64, cigarOffsets=offsets.ctypes.data)) == null
    assert (chars == FILL).all()
    for wrong in (dict(num_reads=1 << 32), dict(C_=0), dict(C_=17), dict(max_ops=0), dict(max_ops=sc.MAX_OPS + 1), dict(flags=2), dict(flags=3),
                  dict(flags=1 << 31)):
        assert call(**wrong) == illegal, wrong
    assert call(C_=16, max_ops=sc.MAX_OPS, flags=1, num_reads=1) == success  # (the limits themselves; one read: rows of 4096 words are not there)
    assert (offsets[2:] == 7).all() and counter[0] == 5
    with pytest.raises(Exception):
        host(awfm, case, flags=4)
