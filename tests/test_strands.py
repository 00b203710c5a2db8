"""awfmChooseStrands and awfmOrientReads (include/awfm_gpu.h "strands", csrc/awfm_strands.c), the host twins, against the plain-Python
restatement of tests/strands_common.py: on the edge list, whose hand-computed literals hold both, and on random tables for 1, 4, 5
and 16 slots a row, paired and unpaired; two equivalences that tie the definition to the merged ones -- with the reverse rows
unused the per-read outputs are slot scores' rules on the forward rows, and with one orientation's rows unused the paired outputs
are awfmPairMates' on the same-strand table --; every output NULL in turn, counters that start nonzero, every refusal; and the
orienting gather at every read length around the edges of its layout, every alignment of source and destination, with each kind
of malformed read, up to the last byte of its buffers, and with its refusals.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_mates_common as pm  # noqa: E402
import score_chains_common as sc  # noqa: E402
import strands_common as st  # noqa: E402

SETTINGS = ({}, dict(min_score=4, unpaired_penalty=3, window_pad=0, mapq_cap=254), dict(min_insert=-400, max_insert=-150, unpaired_penalty=0))
BEFORE = dict(numReverse=5, numProper=9, numWindows=1 << 33, numMalformed=2)


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("slots", [4, 16])
def test_edge_list_equals_the_restatement_and_the_hand_computed_values(awfm, slots, paired):
    for case, edges in st.edge_cases(slots):
        want = case.expected(paired)
        st.check_edges(want, edges, paired, what=f"restatement C={slots}")
        for threads in (1, 16):
            got = case.host(awfm, paired, threads=threads)
            st.assert_equal(got, want, st.names(paired), what=f"{edges[0].name} C={slots}")
            st.check_edges(got, edges, paired, what=f"host C={slots}")


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("slots", [1, 4, 5, 16])
def test_random_tables_equal_the_restatement(awfm, slots, paired):
    for k, reads in enumerate((2, 130, 6, 600)):
        case = st.random_case(100 * slots + reads, reads, slots, SETTINGS[k % 3], big=k % 2 == 1)
        want = case.expected(paired, BEFORE)
        assert want["numMalformed"] > 2 or reads < 100
        if paired and reads >= 100:
            assert want["numProper"] > 9 + reads // 32 and want["numWindows"] > (1 << 33) + reads // 32 and want["numReverse"] > 5 + reads // 8
        st.assert_equal(case.host(awfm, paired, threads=16, before=BEFORE, fill=0xA5), want, st.names(paired), what=f"{reads} reads")


def test_an_odd_number_of_reads_unpaired(awfm):
    case = st.random_case(7, 33, 4)
    st.assert_equal(case.host(awfm, False), case.expected(False), st.names(False))


def _unused(case, rows):
    """the case with every slot of these rows unused"""
    slots = {name: a.copy() for name, a in case.slots.items()}
    slots["sequences"][rows, :] = st.NO_WINDOW
    slots["slotScores"][rows, :] = st.NONE
    slots["slotReadEnds"][rows, :] = 0
    slots["slotTextEnds"][rows, :] = 0
    return st.Case(case.offsets, slots, case.params)


def _well_formed(case):
    """the case with every reverse row as long as its forward row, and no inverted row"""
    R = case.num_reads
    lengths = np.abs(np.diff(case.offsets[:R + 1].astype(np.int64)))
    offsets = np.concatenate(([1000], 1000 + np.cumsum(np.concatenate((lengths, lengths))))).astype(np.uint64)
    return st.Case(offsets, case.slots, case.params)


@pytest.mark.parametrize("slots", [1, 4, 5, 16])
def test_with_the_reverse_rows_unused_the_reads_are_slot_scores_reads(awfm, slots):
    """equivalence (a): strandSlots, bestScores, secondScores and mappingQualities are bestSlots, bestScores, secondScores and
    mappingQualities of slot scores' per-read rules 1 to 5 (tests/score_chains_common.py read_rules) on the forward rows"""
    for k, reads in enumerate((9, 300)):
        case = _well_formed(st.random_case(300 + slots + k, reads, slots, SETTINGS[k + 1]))
        case = _unused(case, np.arange(reads, 2 * reads))
        got = case.host(awfm, False, threads=16)
        q = case.params
        for r in range(reads):
            best, best_score, _, second_score, mapq = sc.read_rules([int(v) for v in case.slots["slotScores"][r]],
                                                                    [int(v) for v in case.slots["slotReadEnds"][r]],
                                                                    [int(v) for v in case.slots["slotTextEnds"][r]],
                                                                    [int(v) for v in case.slots["sequences"][r]], q["min_score"], q["mapq_cap"])
            have = tuple(int(got[k][r]) for k in ("strandSlots", "bestScores", "secondScores", "mappingQualities", "strands"))
            assert have == (best, best_score, second_score, mapq, 0), (r, have)
        assert got["numReverse"] == 0 and (got["rowSlots"][reads:] == st.NO_SLOT).all() and np.array_equal(got["rowSlots"][:reads], got["strandSlots"])


@pytest.mark.parametrize("first_forward", [True, False], ids=["F(m1),V(m2)", "F(m2),V(m1)"])
@pytest.mark.parametrize("slots", [1, 4, 5, 16])
def test_with_one_orientation_unused_the_pairs_are_pair_mates_pairs(awfm, slots, first_forward):
    """equivalence (b): paired, with rows V(m1) and F(m2) unused everywhere, every pair and read output equals awfmPairMates on the
    interleaved table (F(m1), V(m2)) given q_r as its input qualities; likewise with the other two rows unused against (F(m2),
    V(m1)), whose mate A is m2.  The windows are compared at the rows they name.  In the second table pair mates breaks a tie
    between candidates by m2's slot first and this call by m1's, so that table is drawn with unique_sums: no two candidates of
    a pair have one value, and the tie rules (held by the edge list) stay out of this comparison."""
    for k, reads in enumerate((8, 400)):
        case = _well_formed(st.random_case(500 + slots + k, reads, slots, SETTINGS[k + 1], unique_sums=not first_forward))
        R = reads
        m1, m2 = np.arange(0, R, 2), np.arange(1, R, 2)
        case = _unused(case, np.concatenate((R + m1, m2) if first_forward else (m1, R + m2)))
        got = case.host(awfm, True, threads=16)
        q_r = case.host(awfm, False, threads=16)["mappingQualities"]
        # the same-strand table: read 2p is mate A (the one on strand 0), read 2p + 1 mate B (the one on strand 1)
        rows = np.empty(R, np.int64)
        rows[0::2], rows[1::2] = (m1, R + m2) if first_forward else (m2, R + m1)
        reads_of = np.empty(R, np.int64)  # the read of each row of the table
        reads_of[0::2], reads_of[1::2] = (m1, m2) if first_forward else (m2, m1)
        lengths = np.diff(case.offsets[:R + 1].astype(np.int64))[reads_of]
        offsets = np.concatenate(([0], np.cumsum(lengths))).astype(np.uint64)
        table = {name: a[rows] for name, a in case.slots.items()}
        want = awfm.pair_mates_host(offsets, table, mapping_qualities=q_r[reads_of], threads=16, **case.params)
        for name in st.PAIR_OUTPUTS:
            assert np.array_equal(got[name], want[name]), name
        assert got["numProper"] == want["numProper"] and got["numWindows"] == want["numWindows"]
        assert np.array_equal(got["strandSlots"][reads_of], want["pairSlots"]) and np.array_equal(got["rowSlots"][rows], want["pairSlots"])
        assert np.array_equal(got["mappingQualities"][reads_of], want["mappingQualities"])
        assert np.array_equal(got["strands"][reads_of], np.where(want["pairSlots"] == st.NO_SLOT, 0, np.tile([0, 1], R // 2)))
        # a read's window is on the row of the strand it would pair on: the table's row of that read
        for name in ("windowSequences", "windowBegins", "windowEnds"):
            assert np.array_equal(got[name][rows], want[name]), name
        others = np.setdiff1d(np.arange(2 * R), rows)
        assert (got["windowSequences"][others] == st.NO_WINDOW).all() and (got["rowSlots"][others] == st.NO_SLOT).all()


def test_every_output_null_in_turn(awfm):
    case = st.random_case(3, 40, 4)
    for paired in (False, True):
        want = case.expected(paired)
        for missing in st.names(paired):
            for outputs in ([n for n in st.names(paired) if n != missing], [missing]):
                got = case.host(awfm, paired, outputs=outputs, fill=0x5A)
                assert sorted(got) == sorted(outputs)
                st.assert_equal(got, want, outputs, what=str(outputs))
    # unpaired, the pair arrays are not written
    lib = awfm._lib.lib()
    guard = np.full(20, 0x5A, np.uint8)
    sin = awfm.strand_inputs(case.offsets.ctypes.data, *(case.slots[name].ctypes.data for name, _ in awfm.PAIR_SLOT_INPUTS))
    sout = awfm.strand_outputs(properPairs=guard.ctypes.data)
    params = awfm.pair_params(**case.params)
    assert lib.awfmChooseStrands(C.byref(sin), 40, 4, 0, C.byref(params), C.byref(sout), 2) == awfm.AwFmSuccess and (guard == 0x5A).all()
    assert lib.awfmChooseStrands(C.byref(sin), 40, 4, 1, C.byref(params), C.byref(sout), 2) == awfm.AwFmSuccess
    assert np.array_equal(guard, case.expected(True)["properPairs"])


def test_choose_strands_refusals(awfm):
    case = st.random_case(4, 10, 4)
    lib, bad, null = awfm._lib.lib(), awfm.AwFmIllegalPositionError, -4
    pointers = [case.offsets.ctypes.data] + [case.slots[name].ctypes.data for name, _ in awfm.PAIR_SLOT_INPUTS]
    out = np.full(10, 0x5A5A5A5A, np.uint32)
    sout, good, params = awfm.strand_outputs(strandSlots=out.ctypes.data), awfm.strand_inputs(*pointers), awfm.pair_params(200, 500)

    def raw(inputs, reads, outputs, settings=params, slots=4, flags=1):
        return lib.awfmChooseStrands(None if inputs is None else C.byref(inputs), reads, slots, flags, None if settings is None else C.byref(settings),
                                     None if outputs is None else C.byref(outputs), 2)

    assert raw(None, 10, sout) == null and raw(good, 10, None) == null and raw(good, 10, sout, None) == null
    for k in range(5):
        assert raw(awfm.strand_inputs(*[0 if j == k else v for j, v in enumerate(pointers)]), 10, sout) == null, k
    assert raw(good, 10, sout, slots=0) == bad and raw(good, 10, sout, slots=17) == bad and raw(good, 1 << 31, sout) == bad
    assert raw(good, 10, sout, flags=2) == bad and raw(good, 10, sout, flags=3) == bad and raw(good, 9, sout) == bad
    for kw in (dict(min_insert=501), dict(min_insert=-(1 << 40) - 1), dict(max_insert=(1 << 40) + 1), dict(mapq_cap=255)):
        assert raw(good, 10, sout, awfm.pair_params(**dict(dict(min_insert=200, max_insert=500), **kw))) == bad, kw
    assert (out == 0x5A5A5A5A).all()
    # unpaired, the interval is not read; mapqCap is
    assert raw(good, 9, sout, awfm.pair_params(501, 200), flags=0) == awfm.AwFmSuccess
    assert raw(good, 9, sout, awfm.pair_params(200, 500, mapq_cap=255), flags=0) == bad
    assert raw(None, 0, None, None) == awfm.AwFmSuccess  # numReads == 0 touches nothing
    # the order: a NULL argument before a bad count of slots, that before a bad flag, that before a bad interval
    assert raw(None, 10, sout, slots=0) == null and raw(good, 10, sout, awfm.pair_params(501, 200), flags=2) == bad


# ---- orient ---------------------------------------------------------------------------------------------------------------------
def _orient(awfm, case, **kw):
    return awfm.orient_reads_host(case["chars"], case["offsets"], case["strands"], slots=case["columns"], qualities=case["qualities"], **kw)


def _orient_expected(case, **kw):
    return st.orient_expected(case["chars"], case["offsets"], case["strands"], case["columns"], case["qualities"], **kw)


@pytest.mark.parametrize("slots", [1, 4, 16])
def test_orient_every_length_at_every_alignment(awfm, slots):
    """tests/strands_common.py orient_order: every length of the list at every destination offset mod 4, behind leads 0 to 3 and
    with random strands and their opposites, so that every length meets every combination of source and destination offset mod 4
    from either row; the qualities reversed; the last read ends at the last byte of its buffers"""
    order = st.orient_order()
    seen = set()
    for lead in range(4):
        case = st.orient_case(lead, order, lead=lead, C=slots)
        for flip in (0, 1):
            case["strands"] ^= np.uint8(flip)
            seen |= st.orient_alignments(case, order)
            want = _orient_expected(case, fill=0xEE)
            assert want["numMalformed"] == 0 and int(want["readOffsets"][-1]) == want["readChars"].size == (case["chars"].size - lead) // 2
            for threads in (1, 16):
                st.assert_orient_equal(_orient(awfm, case, fill=0xEE, threads=threads), want, what=f"lead {lead} flip {flip}")
    assert seen == {(n, s, a, b) for n in st.ORIENT_LENGTHS for s in range(2) for a in range(4) for b in range(4)}
    # the qualities of a read on strand 1 are the forward row's, mirrored and not complemented; its characters the reverse row's
    case = st.orient_case(1, [5, 7], C=slots)
    case["strands"][:] = (1, 0)
    got = _orient(awfm, case)
    assert bytes(got["qualities"][:5]) == bytes(case["qualities"][:5][::-1]) and bytes(got["qualities"][5:]) == bytes(case["qualities"][5:12])
    assert bytes(got["readChars"][:5]) == bytes(case["chars"][12:17]) and bytes(got["readChars"][5:]) == bytes(case["chars"][5:12])


def test_orient_columns_and_qualities_are_optional(awfm):
    case = st.orient_case(2, [30, 0, 65, 9], lead=1)
    want = _orient_expected(case)
    got = awfm.orient_reads_host(case["chars"], case["offsets"], case["strands"])
    assert sorted(got) == ["numMalformed", "readChars", "readOffsets"] and np.array_equal(got["readChars"], want["readChars"])
    for name in st.SLOT_COLUMNS:
        got = awfm.orient_reads_host(case["chars"], case["offsets"], case["strands"], slots={name: case["columns"][name]})
        assert np.array_equal(got[name], want[name]) and np.array_equal(got["readOffsets"], want["readOffsets"]), name


def test_orient_malformed_reads(awfm):
    """each kind: inverted forward or reverse offsets, rows beyond numReadChars, rows of two lengths, a strand above 1, a read
    that ends beyond the capacity, a read that begins before the first: nothing of theirs is written but the unused columns"""
    base = st.orient_case(5, [20, 21, 22, 23, 24, 25, 26, 27], lead=2, tail=4)
    R = 8
    for kind in range(7):
        case = {k: (v.copy() if isinstance(v, np.ndarray) else {n: a.copy() for n, a in v.items()}) for k, v in base.items()}
        kw = {}
        o = case["offsets"]
        if kind == 0:
            o[3], o[4] = o[4], o[3]  # read 3 ends before it begins, its neighbours are longer than their reverse rows
        elif kind == 1:
            o[R + 3], o[R + 4] = o[R + 4], o[R + 3]
        elif kind == 2:
            kw["num_read_chars"] = int(o[2 * R - 1])  # the last reverse row ends beyond
        elif kind == 3:
            o[R + 5] += 1  # rows 4 and 5 of the reverse half have other lengths than the forward ones
        elif kind == 4:
            case["strands"][[1, 6]] = (2, 255)
        elif kind == 5:
            kw["capacity"] = int(o[R - 1] - o[0]) + 3  # the last read ends beyond the capacity
        else:
            o[0] = o[1] + 1  # every later read begins at or after the first; read 0 is inverted
        want = _orient_expected(case, fill=0x77, malformed_before=3, **kw)
        assert 3 < want["numMalformed"] < 3 + R, (kind, want["numMalformed"])  # some reads of each case, never all
        st.assert_orient_equal(_orient(awfm, case, fill=0x77, malformed_before=3, threads=4, **kw), want, what=f"kind {kind}")


def test_orient_refusals(awfm):
    case = st.orient_case(6, [10, 11], C=4)
    lib, bad, null = awfm._lib.lib(), awfm.AwFmIllegalPositionError, -4
    chars, offsets, strands = case["chars"], case["offsets"], case["strands"]
    out_chars, out_offsets = np.full(21, 0x5A, np.uint8), np.zeros(3, np.uint64)
    column, out_column = case["columns"]["chainAnchors"], np.zeros((2, 4), np.uint32)

    def raw(inputs, outputs, reads=2, slots=4):
        return lib.awfmOrientReads(None if inputs is None else C.byref(inputs), reads, slots, None if outputs is None else C.byref(outputs), 2)

    def inputs(read_chars=chars.ctypes.data, read_offsets=offsets.ctypes.data, s=strands.ctypes.data, qualities=0, size=chars.size, **columns):
        return awfm.orient_inputs(awfm.verify_inputs(read_chars, size, read_offsets, **{k: v for k, v in columns.items() if k in dict(awfm.VERIFY_SLOT_INPUTS)}),
                                  s, qualities, **{k: v for k, v in columns.items() if k not in dict(awfm.VERIFY_SLOT_INPUTS)})

    def outputs(read_chars=out_chars.ctypes.data, capacity=21, read_offsets=out_offsets.ctypes.data, **columns):
        return awfm.orient_outputs(read_chars, capacity, read_offsets, **columns)

    assert raw(inputs(), outputs()) == awfm.AwFmSuccess and bytes(out_chars) == bytes(st.orient_expected(chars, offsets, strands)["readChars"])
    out_chars[:] = 0x5A
    assert raw(None, outputs()) == null and raw(inputs(), None) == null
    assert raw(inputs(read_chars=0), outputs()) == null and raw(inputs(read_offsets=0), outputs()) == null and raw(inputs(s=0), outputs()) == null
    assert raw(inputs(), outputs(read_chars=0)) == null and raw(inputs(), outputs(read_offsets=0)) == null
    # an output without its input and the reverse
    for name in st.SLOT_COLUMNS:
        assert raw(inputs(**{name: column.ctypes.data}), outputs()) == null and raw(inputs(), outputs(**{name: out_column.ctypes.data})) == null, name
    assert raw(inputs(qualities=case["qualities"].ctypes.data), outputs()) == null and raw(inputs(), outputs(qualities=out_chars.ctypes.data)) == null
    assert raw(inputs(), outputs(), slots=0) == bad and raw(inputs(), outputs(), slots=17) == bad and raw(inputs(), outputs(), reads=1 << 31) == bad
    # overlap as pointer ranges: the output begins on the input's last byte; the input begins on the output's last byte
    room = np.zeros(chars.size + 21, np.uint8)
    room[:chars.size] = chars
    assert raw(inputs(read_chars=room.ctypes.data), outputs(read_chars=room.ctypes.data + chars.size - 1)) == bad
    assert raw(inputs(read_chars=room.ctypes.data + 20, size=1), outputs(read_chars=room.ctypes.data)) == bad
    assert raw(inputs(read_chars=room.ctypes.data), outputs(read_chars=room.ctypes.data + chars.size)) == awfm.AwFmSuccess  # adjacent
    assert raw(None, None, reads=0) == awfm.AwFmSuccess  # numReads == 0 touches nothing
    assert (out_chars == 0x5A).all()


def test_end_to_end_on_a_one_strand_index_through_the_host_twins(awfm, tmp_path):
    """tests/strands_common.py EndToEnd: the loop of the header through the host twins -- reverse complement of every read into
    the second half, slot scores on the 2R rows, strand choice, window scores on the windows it names, slot scores, strand choice,
    orient, affine alignment, strings, SAM records.  Every plain pair is proper on its planted strand and position, every mate
    the seeds cannot place is rescued, every pair outside the insert interval stays improper; a proper pair from the reverse
    strand prints FLAG 83 / 163 and one from the forward strand 99 / 147 with the planted POS, PNEXT and signed TLEN.
    tests/test_gpu_strands.py holds the device to the same condition and to these bytes."""
    e = st.EndToEnd(awfm, tmp_path)
    try:
        e.check(e.host_loop(awfm))
    finally:
        e.close()
