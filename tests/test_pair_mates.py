"""awfmPairMates and awfmReverseComplementReads (include/awfm_gpu.h "pair mates", csrc/awfm_pair_mates.c), the host twins, against the
plain-Python restatement of tests/pair_mates_common.py and the hand-computed values of its edge list: every output and both
counters, on the edge list, on random slot tables for 1, 2, 4, 5 and 16 slots a read, with every output NULL in turn and alone,
with counters that hold a value before the call, with no pairs, with bad arguments, and on 1 and 16 threads; the reverse
complement on read lengths 0, 1, 2 and odd ones, mixed case, ambiguity letters, the three selections, malformed offsets and
overlapping buffers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_mates_common as pm  # noqa: E402


def test_restatement_gives_the_hand_computed_values_of_the_edge_list():
    for case, edges in pm.edge_cases():
        pm.check_edges(case.expected(), edges, what="restatement")


@pytest.mark.parametrize("slots", [4, 16])
def test_host_twin_on_the_edge_list(awfm, slots):
    for case, edges in pm.edge_cases(slots):
        got = case.host(awfm)
        pm.check_edges(got, edges, what="twin")
        pm.assert_equal(got, case.expected(), what=edges[0].name)


@pytest.mark.parametrize("slots", [1, 2, 4, 5, 16])
def test_host_twin_equals_the_restatement_on_random_tables(awfm, slots):
    for seed, params, qualities, big in ((1, {}, True, False), (2, dict(min_score=4, unpaired_penalty=3, window_pad=0, mapq_cap=254), True, False),
                                         (3, dict(min_insert=-400, max_insert=-150, unpaired_penalty=0), False, False),
                                         (4, dict(mapq_cap=254, unpaired_penalty=1 << 25), True, True)):
        case = pm.random_case(100 * slots + seed, 300, slots, params, qualities, big)
        want = case.expected(proper_before=5, windows_before=7)
        if seed == 1 and slots >= 2:  # the tables do collide
            assert want["numProper"] > 40 and want["numWindows"] > 10 and (want["pairSecondScores"] == want["pairScores"]).sum() > 10
        pm.assert_equal(case.host(awfm, proper_before=5, windows_before=7), want, what=f"C={slots} seed={seed}")


def test_threads_null_outputs_counters_and_no_pairs(awfm):
    case = pm.random_case(9, 257, 4)
    want = case.expected()
    pm.assert_equal(case.host(awfm, threads=1), want, what="1 thread")
    pm.assert_equal(case.host(awfm, threads=16), want, what="16 threads")
    for missing in pm.NAMES:  # every output NULL in turn, and alone
        for outputs in ([n for n in pm.NAMES if n != missing], [missing]):
            got = case.host(awfm, outputs=outputs, fill=0xA5)
            assert sorted(got) == sorted(outputs)
            pm.assert_equal(got, want, names=outputs, what=str(outputs))
    got = case.host(awfm, proper_before=1 << 40, windows_before=3)
    assert got["numProper"] == (1 << 40) + want["numProper"] and got["numWindows"] == 3 + want["numWindows"]
    # the output qualities may be the input array
    lib, given = awfm._lib.lib(), case.qualities.copy()
    pin = awfm.pair_inputs(case.offsets.ctypes.data, *(case.slots[name].ctypes.data for name in pm.SLOT_INPUTS), given.ctypes.data)
    params = awfm.pair_params(**case.params)
    in_place = awfm.pair_outputs(mappingQualities=given.ctypes.data)
    assert lib.awfmPairMates(C.byref(pin), case.num_pairs, 4, C.byref(params), C.byref(in_place), 3) == awfm.AwFmSuccess
    assert np.array_equal(given, want["mappingQualities"])
    # no pairs: nothing is touched, whatever else is wrong
    assert lib.awfmPairMates(None, 0, 99, None, None, 1) == awfm.AwFmSuccess
    empty = pm.Case(np.array([0], np.uint64), {name: np.zeros((0, 4), d) for name, d in pm.SLOT_INPUTS.items()}, None, {})
    got = empty.host(awfm, proper_before=4, windows_before=5)
    assert got["numProper"] == 4 and got["numWindows"] == 5 and got["pairSlots"].size == 0


def test_bad_arguments_return_their_codes(awfm):
    case = pm.random_case(5, 8, 4)
    bad, null = awfm.AwFmIllegalPositionError, -4  # AwFmNullPtrError
    for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(min_insert=501), dict(min_insert=-(1 << 40) - 1),
               dict(max_insert=(1 << 40) + 1), dict(mapq_cap=255)):
        with pytest.raises(awfm.AwFmError) as e:
            case.host(awfm, fill=0xA5, **kw)
        assert e.value.rc == bad, kw
    case.host(awfm, min_insert=-(1 << 40), max_insert=1 << 40, mapq_cap=254, min_score=0xFFFFFFFF, unpaired_penalty=0xFFFFFFFF, window_pad=0xFFFFFFFF)
    lib, params, out = awfm._lib.lib(), awfm.pair_params(**case.params), awfm.pair_outputs()
    pointers = [case.offsets.ctypes.data] + [case.slots[name].ctypes.data for name in pm.SLOT_INPUTS]
    good = awfm.pair_inputs(*pointers)
    assert lib.awfmPairMates(C.byref(good), 8, 4, C.byref(params), C.byref(out), 2) == awfm.AwFmSuccess
    assert lib.awfmPairMates(None, 8, 4, C.byref(params), C.byref(out), 2) == null
    assert lib.awfmPairMates(C.byref(good), 8, 4, None, C.byref(out), 2) == null
    assert lib.awfmPairMates(C.byref(good), 8, 4, C.byref(params), None, 2) == null
    for k in range(5):
        missing = awfm.pair_inputs(*[0 if j == k else v for j, v in enumerate(pointers)])
        assert lib.awfmPairMates(C.byref(missing), 8, 4, C.byref(params), C.byref(out), 2) == null, k
    assert lib.awfmPairMates(C.byref(good), 1 << 31, 4, C.byref(params), C.byref(out), 2) == bad  # 2 numPairs >= 2^32
    with pytest.raises(ValueError):
        awfm.pair_outputs(pairSlot=1)


LENGTHS = [0, 1, 2, 3, 5, 0, 7, 150, 151, 64, 33, 1, 0, 2, 99, 100]


@pytest.mark.parametrize("which", [pm.ALL, pm.ODD, pm.EVEN], ids=["all", "odd", "even"])
def test_reverse_complement_equals_python(awfm, which):
    chars, offsets = pm.reads_buffer(7, LENGTHS, lead=5)
    want, _ = pm.reverse_complement(chars, offsets, which, fill=0x5A)
    for threads in (1, 16):
        got, malformed = awfm.reverse_complement_reads_host(chars, offsets, which, threads=threads, fill=0x5A, malformed_before=3)
        assert malformed == 3 and np.array_equal(got, want)
    assert (want[:5] == 0x5A).all() and not np.array_equal(want[5:], chars[5:])
    # twice is the identity on the selected reads, and the case is kept
    again, _ = awfm.reverse_complement_reads_host(want, offsets, which, fill=0x5A)
    assert np.array_equal(again[5:], chars[5:])


def test_reverse_complement_by_hand_malformed_offsets_and_overlap(awfm):
    got, _ = awfm.reverse_complement_reads_host(b"AACGtNacgRyT", [0, 6, 12], pm.ALL)
    assert bytes(got) == b"NaCGTTAyRcgt"
    got, _ = awfm.reverse_complement_reads_host(b"AACGtNacgRyT", [0, 6, 12], pm.ODD)
    assert bytes(got) == b"AACGtNAyRcgt"
    got, _ = awfm.reverse_complement_reads_host(b"AACGtNacgRyT", [0, 6, 12], pm.EVEN)
    assert bytes(got) == b"NaCGTTacgRyT"
    # inverted offsets, and offsets beyond the buffer: neither read nor written, counted
    chars, offsets = pm.reads_buffer(8, [10, 20, 30])
    offsets = np.array([30, 40, 0, 30, 62], np.uint64)  # read 1 is inverted, read 3 ends beyond the 60 characters
    want, bad = pm.reverse_complement(chars, offsets, pm.ALL, fill=0x5A)
    got, malformed = awfm.reverse_complement_reads_host(chars, offsets, pm.ALL, fill=0x5A, malformed_before=1)
    assert bad == 2 and malformed == 3 and np.array_equal(got, want) and (got[:40] != 0x5A).any() and (got[40:] == 0x5A).all()
    want, bad = pm.reverse_complement(chars, offsets, pm.ALL, fill=0x5A, num_read_chars=35)  # a shorter buffer: read 0 leaves it too
    got, malformed = awfm.reverse_complement_reads_host(chars, offsets, pm.ALL, fill=0x5A, num_read_chars=35)
    assert bad == malformed == 3 and np.array_equal(got, want) and (got[30:] == 0x5A).all()
    # overlap is refused on the pointer ranges, a neighbour is not; an unknown selection and NULL arguments
    lib, buffer, o = awfm._lib.lib(), np.frombuffer(b"acgtacgtacgtacgtacgtacgt", np.uint8).copy(), np.array([0, 4, 8], np.uint64)
    base = buffer.ctypes.data

    def raw(source, target, which=pm.ALL, offsets=o.ctypes.data, reads=2):
        return lib.awfmReverseComplementReads(source, 8, offsets, reads, which, target, None, 1)

    for shift in (0, 1, 7):
        assert raw(base + 8, base + 8 + shift) == raw(base + 8, base + 8 - shift) == awfm.AwFmIllegalPositionError, shift
    assert bytes(buffer) == b"acgtacgtacgtacgtacgtacgt"
    assert raw(base + 8, base + 16) == awfm.AwFmSuccess and raw(base + 8, base) == awfm.AwFmSuccess
    assert bytes(buffer) == b"acgtacgtacgtacgtacgtacgt"  # (acgt is its own reverse complement)
    assert raw(base, base + 8, which=3) == awfm.AwFmIllegalPositionError
    assert raw(None, base + 8) == -4 and raw(base, base + 8, offsets=None) == -4
    assert raw(None, None, which=9, offsets=None, reads=0) == awfm.AwFmSuccess  # no reads: nothing is touched
    assert raw(base, None) == awfm.AwFmSuccess  # the output may be NULL


def test_end_to_end_through_the_host_twins(awfm, tmp_path):
    """the condition tests/test_gpu_pair_mates.py relies on, met by the HOST twins alone: every planted pair of the FASTA file held
    on both strands is found -- the plain pairs proper at the first pairing, the mates the seeds cannot place proper after the
    window call on the windows the first pairing names, the pairs outside the insert interval never, with windows for both reads
    -- and affine alignment on pairSlots returns the planted intervals"""
    e = pm.EndToEnd(awfm, tmp_path)
    try:
        e.check(*e.loop(pm.HostSide(awfm, e)))
    finally:
        e.close()
