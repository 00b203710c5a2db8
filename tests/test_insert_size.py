"""awfmInsertHistogram and awfmInsertInterval (include/awfm_gpu.h "insert size", csrc/awfm_insert.c), the host twins, against the
plain-Python restatement of tests/insert_size_common.py and the hand-computed values of its edge list: the histogram, both
counters and the eight fields of the estimate, on the edge list, on random slot tables for 1, 2, 4, 5 and 16 slots a read, on 1
and 16 threads, adding to a histogram and counters that hold values, with each counter NULL, with no pairs and with every bad
argument; estimate_insert_size_host against the two calls; and the end-to-end loop of pair_mates_common.EndToEnd with the
interval estimated after the first slot scores."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import insert_size_common as ic  # noqa: E402
import pair_mates_common as pm  # noqa: E402


def test_restatement_gives_the_hand_computed_values_of_the_edge_list():
    for e in ic.EDGES:
        h, samples, outside = ic.histogram_expected(e.case(), e.params)
        assert np.array_equal(h, e.dense()) and (samples, outside) == (e.samples, e.outside), e.name
        ic.check_estimate(ic.interval_expected(h, e.params), e.interval, what=e.name)


@pytest.mark.parametrize("slots", [4, 16])
def test_host_twins_on_the_edge_list(awfm, slots):
    for e in ic.EDGES:
        case, params = e.case(slots), awfm.insert_params(**e.params)
        h, samples, outside = awfm.insert_histogram_host(case.offsets, case.slots, params, mapping_qualities=case.qualities)
        assert np.array_equal(h, e.dense()) and (samples, outside) == (e.samples, e.outside), e.name
        ic.check_estimate(awfm.insert_interval_host(h, params), e.interval, what=e.name)


@pytest.mark.parametrize("slots", [1, 2, 4, 5, 16])
def test_host_twins_equal_the_restatement_on_random_tables(awfm, slots):
    for seed, pairs, extra in ((1, 300, {}), (2, 64, dict(spread=0, min_samples=5)), (3, 257, dict(spread=16)), (4, 100, dict(min_samples=1000))):
        case, ip = ic.random_table(100 * slots + seed, pairs, slots, **extra)
        samples, outside = ic.check_condition(case, ip)
        before = np.arange(ic.bins_of(ip), dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33)  # the histogram and both counters are added to
        want = ic.histogram_expected(case, ip, before, samples_before=5, outside_before=1 << 40)
        assert want[1] == 5 + samples and want[2] == (1 << 40) + outside
        params = awfm.insert_params(**ip)
        got = awfm.insert_histogram_host(case.offsets, case.slots, params, mapping_qualities=case.qualities, histogram=before, samples_before=5,
                                         outside_before=1 << 40)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (slots, seed)
        fresh, _, _ = awfm.insert_histogram_host(case.offsets, case.slots, params, mapping_qualities=case.qualities)
        assert np.array_equal(fresh, want[0] - before)
        for h in (fresh, want[0]):
            ic.check_estimate(awfm.insert_interval_host(h, params), ic.interval_expected(h, ip), what=f"C={slots} seed={seed}")
        if seed == 4:
            assert awfm.insert_interval_host(fresh, params)["valid"] == 0
        # the convenience call is the two calls
        both = awfm.estimate_insert_size_host(case.offsets, case.slots, params, mapping_qualities=case.qualities)
        assert np.array_equal(both.pop("histogram"), fresh) and both.pop("numOutside") == outside
        assert both == awfm.insert_interval_host(fresh, params)


def test_threads_null_counters_and_no_pairs(awfm):
    case, ip = ic.random_table(9, 5000, 4)  # (a loop of 4096 pairs and more is split over the threads)
    params = awfm.insert_params(**ip)
    want = ic.histogram_expected(case, ip)
    ic.check_condition(case, ip)
    for threads in (1, 16):
        got = awfm.insert_histogram_host(case.offsets, case.slots, params, mapping_qualities=case.qualities, threads=threads)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], threads
    for counters in (("numSamples",), ("numOutside",), ()):
        got = awfm.insert_histogram_host(case.offsets, case.slots, params, mapping_qualities=case.qualities, counters=counters, threads=16)
        assert np.array_equal(got[0], want[0])
        assert got[1] == (want[1] if "numSamples" in counters else None) and got[2] == (want[2] if "numOutside" in counters else None)
    # numPairs == 0 touches nothing, whatever else is passed
    lib = awfm._lib.lib()
    assert lib.awfmInsertHistogram(None, 0, 99, None, None, None, None, 4) == awfm.AwFmSuccess
    # counts above 2^32 in a bin
    big = np.zeros(ic.bins_of(ip), np.uint64)
    big[[3, 10, 11]] = [(1 << 40) + 1, 1 << 41, 5]
    ic.check_estimate(awfm.insert_interval_host(big, params), ic.interval_expected(big, ip))


def test_bad_arguments(awfm):
    lib, bad, null = awfm._lib.lib(), awfm.AwFmIllegalPositionError, -4
    case, ip = ic.random_table(5, 20, 4)
    pointers = [case.offsets.ctypes.data] + [case.slots[name].ctypes.data for name in pm.SLOT_INPUTS]
    good, params = awfm.pair_inputs(*pointers, case.qualities.ctypes.data), awfm.insert_params(**ip)
    h = np.zeros(ic.bins_of(ip), np.uint64)
    estimate = awfm._lib.AwFmInsertEstimate()

    def histogram(inputs=good, pairs=case.num_pairs, slots=4, settings=params, target=h.ctypes.data):
        return lib.awfmInsertHistogram(None if inputs is None else C.byref(inputs), pairs, slots, None if settings is None else C.byref(settings),
                                       target, None, None, 2)

    assert histogram() == awfm.AwFmSuccess and h.sum() == ic.histogram_expected(case, ip)[1]
    h[...] = 0
    assert histogram(inputs=None) == null and histogram(settings=None) == null and histogram(target=None) == null
    for k in range(5):
        assert histogram(inputs=awfm.pair_inputs(*[0 if j == k else v for j, v in enumerate(pointers)])) == null, k
    assert histogram(slots=0) == bad and histogram(slots=17) == bad and histogram(pairs=1 << 31) == bad
    M = ic.MAX_INSERT
    illegal = (dict(low_template=500, high_template=499), dict(low_template=0, high_template=ic.MAX_BINS), dict(low_template=-M - 1, high_template=-M),
               dict(low_template=M, high_template=M + 1), dict(spread=ic.MAX_SPREAD + 1), dict(fallback_min=901), dict(fallback_min=-M - 1),
               dict(fallback_max=M + 1))
    for kw in illegal:
        wrong = awfm.insert_params(**dict(ip, **kw))
        assert histogram(settings=wrong) == bad, kw
        assert lib.awfmInsertInterval(h.ctypes.data, C.byref(wrong), C.byref(estimate)) == bad, kw
    assert not h.any() and estimate.valid == 0 and estimate.maxInsert == 0  # nothing was touched
    for kw in (dict(low_template=0, high_template=ic.MAX_BINS - 1), dict(low_template=-M, high_template=-M), dict(low_template=M, high_template=M),
               dict(spread=ic.MAX_SPREAD), dict(fallback_min=-M, fallback_max=M), dict(fallback_min=7, fallback_max=7)):  # the last legal values
        edge = awfm.insert_params(**dict(ip, **kw))
        wide = np.zeros(ic.bins_of(dict(ip, **kw)), np.uint64)
        assert histogram(settings=edge, target=wide.ctypes.data) == awfm.AwFmSuccess, kw
        assert lib.awfmInsertInterval(wide.ctypes.data, C.byref(edge), C.byref(estimate)) == awfm.AwFmSuccess, kw
    assert lib.awfmInsertInterval(None, C.byref(params), C.byref(estimate)) == null
    assert lib.awfmInsertInterval(h.ctypes.data, None, C.byref(estimate)) == null
    assert lib.awfmInsertInterval(h.ctypes.data, C.byref(params), None) == null
    with pytest.raises(awfm.AwFmError) as e:
        awfm.insert_histogram_host(case.offsets, case.slots, awfm.insert_params(**dict(ip, spread=17)))
    assert e.value.rc == bad


def test_end_to_end_loop_with_the_interval_estimated_after_the_first_slot_scores(awfm, tmp_path):
    """pair_mates_common.EndToEnd through the host twins: slot scores, the estimate, pairing with it, window scores, slot scores,
    pairing with it, affine alignment.  The plain pairs plant T = 400: the three quartiles and the mean are 400, the interval
    [384, 416]; every planted plain and rescued pair comes out proper at its planted place."""
    e = pm.EndToEnd(awfm, tmp_path)
    try:
        side = ic.EstimatingHostSide(awfm, e)
        first, second, aligned = e.loop(side)
        kinds = [k for _, _, _, k in e.plan]
        assert first["numProper"] == kinds.count("plain")
        ic.check_end_to_end(e, side.estimate, second, aligned)
        assert side.estimate["numSamples"] + side.estimate["numOutside"] <= pm.E2E["pairs"] - kinds.count("rescued")
    finally:
        e.close()
