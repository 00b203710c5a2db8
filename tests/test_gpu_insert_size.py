"""awfmGpuInsertHistogram, awfmGpuInsertInterval and awfmGpuPairMatesEstimated (include/awfm_gpu.h "insert size",
csrc/awfm_insert_kernel.h, csrc/awfm_pair_mates_kernel.h) against the host twins, which tests/test_insert_size.py and
tests/test_pair_mates.py pin to the plain-Python restatements and to hand-computed values: bit for bit, every output between guard
words.  The histogram on the edge list, on batches whose last wave and workgroup end inside them for 1, 4, 5 and 16 slots a
read, on more pairs than the grid has threads, with 1, 2, kInsertLdsBins, kInsertLdsBins + 1 and 65536 bins, in both tiers, on
4097 pairs of one template length, called twice into one histogram, from two streams, with each counter NULL and with bad
arguments; the interval on every histogram of the edge list, on one full bin at either end of 65536, on counts above 2^32 and on
the fallback; the estimated pairing against awfmGpuPairMates with the same interval under both layouts, with every output NULL
in turn, with the three intervals that are not usable, and behind awfmGpuInsertInterval on one stream without a
synchronisation; and the loop end to end from a FASTA file."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import insert_size_common as ic  # noqa: E402
import pair_mates_common as pm  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, _upload  # noqa: E402
from test_gpu_pair_mates import DeviceCall, DeviceSide  # noqa: E402

pytestmark = pytest.mark.gpu

TIERS = pytest.mark.parametrize("tier", [None, "global"], ids=["natural", "global"])
LDS_BINS = 8192  # kInsertLdsBins (tests/test_insert_size_resources.py holds the header to it)


@pytest.fixture(scope="module")
def g(awfm, require_gpu):
    """an image: the calls take it for its device only"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtaacc", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    image = awfm.GpuIndex(ix)
    yield image
    image.destroy()
    ix.dealloc()


@functools.lru_cache(maxsize=None)
def table(seed, pairs, slots):
    case, ip = ic.random_table(seed, pairs, slots)
    ic.check_condition(case, ip)
    return case, ip


def guarded(torch, body):
    """the bytes of `body` between guard words on the device"""
    raw = np.ascontiguousarray(body).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate((np.full(GUARD, PATTERN, np.uint8), raw, np.full(GUARD, PATTERN, np.uint8)))).to("cuda")


def body_of(buffer, dtype, what):
    raw = buffer.cpu().numpy()
    assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), f"wrote outside {what}"
    return raw[GUARD:-GUARD].view(dtype)


class HistogramCall:
    """the arrays of one case on the device, and guarded histograms and counters for calls on them"""

    def __init__(self, awfm, torch, case):
        self.awfm, self.torch, self.case = awfm, torch, case
        self.arrays = [_upload(torch, case.offsets)] + [_upload(torch, case.slots[name]) for name in pm.SLOT_INPUTS]
        self.qualities = None if case.qualities is None else _upload(torch, case.qualities)
        self.inputs = awfm.pair_inputs(*(a.data_ptr() for a in self.arrays), 0 if self.qualities is None else self.qualities.data_ptr())

    def buffers(self, ip, before=None, samples_before=0, outside_before=0):
        start = np.zeros(ic.bins_of(ip), np.uint64) if before is None else before
        return [guarded(self.torch, start), guarded(self.torch, np.array([samples_before], np.uint64)),
                guarded(self.torch, np.array([outside_before], np.uint64))]

    def enqueue(self, g, ip, buffers, counters=(True, True), stream=0, **kw):
        g.insert_histogram(self.inputs, kw.pop("num_pairs", self.case.num_pairs), self.awfm.insert_params(**ip), buffers[0].data_ptr() + GUARD,
                           buffers[1].data_ptr() + GUARD if counters[0] else 0, buffers[2].data_ptr() + GUARD if counters[1] else 0,
                           max_candidates=kw.pop("max_candidates", self.case.C), stream=stream)

    @staticmethod
    def collect(buffers):
        return (body_of(buffers[0], np.uint64, "the histogram"), int(body_of(buffers[1], np.uint64, "numSamples")[0]),
                int(body_of(buffers[2], np.uint64, "numOutside")[0]))

    def __call__(self, g, ip, before=None, samples_before=0, outside_before=0, **kw):
        buffers = self.buffers(ip, before, samples_before, outside_before)
        self.enqueue(g, ip, buffers, **kw)
        self.torch.cuda.synchronize()
        return self.collect(buffers)

    def host(self, ip, before=None, samples_before=0, outside_before=0):
        return self.awfm.insert_histogram_host(self.case.offsets, self.case.slots, self.awfm.insert_params(**ip), mapping_qualities=self.case.qualities,
                                               histogram=before, samples_before=samples_before, outside_before=outside_before, threads=16)


def same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[1:] == want[1:], (what, got[1:], want[1:])
    if not np.array_equal(got[0], want[0]):
        at = int(np.argwhere(got[0] != want[0])[0][0])
        raise AssertionError(f"{what}: histogram[{at}] is {got[0][at]}, expected {want[0][at]} ({(got[0] != want[0]).sum()} differ)")


def device_interval(awfm, torch, g, histogram, ip, stream=0):
    """awfmGpuInsertInterval on an uploaded histogram -> the estimate's dict; the 64 bytes lie between guard words"""
    d_histogram = _upload(torch, np.ascontiguousarray(histogram, dtype=np.uint64))
    d_estimate = guarded(torch, np.full(ic.ESTIMATE_BYTES, PATTERN, np.uint8))
    g.insert_interval(d_histogram.data_ptr(), awfm.insert_params(**ip), d_estimate.data_ptr() + GUARD, stream=stream)
    torch.cuda.synchronize()
    return awfm.insert_estimate_dict(body_of(d_estimate, np.uint8, "the estimate"))


@TIERS
def test_edge_list_equals_the_host_twins_and_the_hand_computed_values(awfm, g, diag, tier):
    import torch
    diag(insert_tier=tier)
    for slots in (4, 16):
        for e in ic.EDGES:
            call = HistogramCall(awfm, torch, e.case(slots))
            before = np.full(ic.bins_of(e.params), 1 << 35, np.uint64)
            got = call(g, e.params, before, samples_before=9, outside_before=1 << 33)
            same(got, call.host(e.params, before, 9, 1 << 33), what=f"{e.name} C={slots}")
            assert np.array_equal(got[0] - before, e.dense()) and (got[1] - 9, got[2] - (1 << 33)) == (e.samples, e.outside), e.name
            if slots == 4:
                estimate = device_interval(awfm, torch, g, e.dense(), e.params)
                ic.check_estimate(estimate, e.interval, what=e.name)
                assert estimate == awfm.insert_interval_host(e.dense(), awfm.insert_params(**e.params)), e.name


@TIERS
@pytest.mark.parametrize("slots", [1, 4, 5, 16])
def test_batches_that_end_inside_a_wave_and_a_workgroup(awfm, g, diag, slots, tier):
    import torch
    diag(insert_tier=tier)
    for pairs in (1, 63, 64, 65, 255, 256, 257, 4097):
        case, ip = table(1000 * slots + pairs, pairs, slots)
        call = HistogramCall(awfm, torch, case)
        before = np.arange(ic.bins_of(ip), dtype=np.uint64) + np.uint64(1 << 32)
        want = call.host(ip, before, 1, 1 << 33)
        same(call(g, ip, before, samples_before=1, outside_before=1 << 33), want, what=f"{pairs} pairs C={slots}")
        estimate = device_interval(awfm, torch, g, want[0] - before, ip)
        assert estimate == awfm.insert_interval_host(want[0] - before, awfm.insert_params(**ip)), (pairs, slots)


def planted_case(seed, pairs, low, high, fixed=None):
    """one slot a mate in a table of two, template lengths spread over [low - 3, high + 3] with both ends of the range planted
    (fixed: every pair has that one), built without a Python loop"""
    rng = np.random.default_rng(seed)
    T = rng.integers(low - 3, high + 4, pairs) if fixed is None else np.full(pairs, fixed, np.int64)
    if fixed is None:
        T[0], T[pairs // 2], T[-1] = low, high, low
        T[1], T[2] = low - 1, high + 1  # (and one outside each end)
    n = 2 * pairs
    slots = {name: np.zeros((n, 2), dtype) for name, dtype in pm.SLOT_INPUTS.items()}
    slots["slotScores"][:, 0], slots["slotScores"][:, 1] = 50, pm.NONE
    slots["slotReadEnds"][:, 0] = 100
    starts = np.full(n, 1 << 20, np.int64)
    starts[1::2] += T - 100
    slots["slotTextEnds"][:, 0] = (starts + 100).astype(np.uint64)
    offsets = 7 + 100 * np.arange(n + 1, dtype=np.uint64)
    return pm.Case(offsets, slots, np.full(n, 40, np.uint8), {}), T


@TIERS
@pytest.mark.parametrize("bins", [1, 2, LDS_BINS, LDS_BINS + 1, 65536])
def test_bin_counts_around_the_private_histogram_and_at_the_limit(awfm, g, diag, bins, tier):
    import torch
    diag(insert_tier=tier)
    low = -700
    ip = dict(ic.PARAMS, low_template=low, high_template=low + bins - 1, min_quality=40)
    case, T = planted_case(bins, 3000, low, low + bins - 1)
    call = HistogramCall(awfm, torch, case)
    want = call.host(ip)
    inside = (T >= low) & (T <= low + bins - 1)
    assert want[0][0] >= 1 and want[0][-1] >= 1 and want[1] == inside.sum() and want[2] == 3000 - inside.sum() >= 1
    same(call(g, ip), want, what=f"{bins} bins")
    assert device_interval(awfm, torch, g, want[0], ip) == awfm.insert_interval_host(want[0], awfm.insert_params(**ip))


def _constant(name):
    import kernel_metadata_common as km
    return km.constant(name, "awfm_insert_kernel.h")


@TIERS
def test_more_pairs_than_the_grid_has_threads_and_the_most_contended_bin(awfm, g, diag, tier):
    import torch
    diag(insert_tier=tier)
    # 4097 pairs of one template length: two workgroups, every add into one bin
    case, _ = planted_case(1, 4097, 0, 999, fixed=300)
    got = HistogramCall(awfm, torch, case)(g, ic.PARAMS)
    assert got[0][300] == 4097 == got[0].sum() and got[1:] == (4097, 0)
    # several trips of every thread: the grid has a workgroup per kInsertPairsPerBlock pairs
    pairs = 5 * _constant("kInsertPairsPerBlock") + 77
    threads = (pairs // _constant("kInsertPairsPerBlock") + 1) * _constant("kInsertThreads")  # six workgroups
    assert pairs > 13 * threads
    case, _ = planted_case(2, pairs, 200, 700)
    ip = dict(ic.PARAMS, low_template=200, high_template=700)
    call = HistogramCall(awfm, torch, case)
    same(call(g, ip), call.host(ip), what="six workgroups")


def test_two_calls_two_streams_null_counters_and_bad_arguments(awfm, g, diag):
    import torch
    (a, ip_a), (b, ip_b) = table(31, 3000, 4), table(32, 2000, 16)
    calls = [HistogramCall(awfm, torch, a), HistogramCall(awfm, torch, b)]
    # two streams at once, one of them in the global tier of a range too wide for the private histogram
    ip_b = dict(ip_b, high_template=ip_b["low_template"] + LDS_BINS + 99)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    buffers = [call.buffers(ip) for call, ip in zip(calls, (ip_a, ip_b))]
    torch.cuda.synchronize()
    for call, ip, buffer, s in zip(calls, (ip_a, ip_b), buffers, streams):
        call.enqueue(g, ip, buffer, stream=s.cuda_stream)
    torch.cuda.synchronize()
    want = calls[0].host(ip_a)
    same(HistogramCall.collect(buffers[0]), want, what="first stream")
    same(HistogramCall.collect(buffers[1]), calls[1].host(ip_b), what="second stream")
    # two calls adding into one histogram, on one stream without a wait in between
    call = calls[0]
    for tier in (None, "global"):
        diag(insert_tier=tier)
        twice = call.buffers(ip_a)
        call.enqueue(g, ip_a, twice)
        call.enqueue(g, ip_a, twice)
        torch.cuda.synchronize()
        same(HistogramCall.collect(twice), (2 * want[0], 2 * want[1], 2 * want[2]), what="two calls")
        # each counter NULL in turn: the other and the histogram as before, the NULL one's buffer untouched
        for counters in ((False, True), (True, False), (False, False)):
            got = call(g, ip_a, samples_before=3, outside_before=4, counters=counters)
            same(got, (want[0], 3 + want[1] * counters[0], 4 + want[2] * counters[1]), what=str(counters))
    diag(insert_tier=None)
    # every bad argument: nothing is launched, the buffers keep what they held
    bad, M = awfm.AwFmIllegalPositionError, ic.MAX_INSERT
    illegal = (dict(low_template=500, high_template=499), dict(low_template=0, high_template=ic.MAX_BINS), dict(low_template=-M - 1, high_template=-M),
               dict(low_template=M, high_template=M + 1), dict(spread=ic.MAX_SPREAD + 1), dict(fallback_min=901), dict(fallback_min=-M - 1),
               dict(fallback_max=M + 1))
    untouched = call.buffers(ip_a, samples_before=5, outside_before=6)
    d_estimate = guarded(torch, np.full(ic.ESTIMATE_BYTES, PATTERN, np.uint8))
    for kw in illegal + (dict(max_candidates=0), dict(max_candidates=17), dict(num_pairs=1 << 31)):
        extra = {k: kw[k] for k in ("max_candidates", "num_pairs") if k in kw}
        wrong = dict(ip_a, **{k: v for k, v in kw.items() if k not in extra})
        with pytest.raises(awfm.AwFmError) as e:
            call.enqueue(g, wrong, untouched, **extra)
        assert e.value.rc == bad, kw
        if not extra:
            with pytest.raises(awfm.AwFmError) as e:
                g.insert_interval(untouched[0].data_ptr() + GUARD, awfm.insert_params(**wrong), d_estimate.data_ptr() + GUARD)
            assert e.value.rc == bad, kw
    lib, params = awfm._lib.lib(), awfm.insert_params(**ip_a)
    target, pointers = untouched[0].data_ptr() + GUARD, [t.data_ptr() for t in call.arrays]

    def raw(inputs, pairs, settings=params, histogram=target, image=g.handle):
        return lib.awfmGpuInsertHistogram(image, None if inputs is None else C.byref(inputs), pairs, 4, None if settings is None else C.byref(settings),
                                          histogram, None, None, None)

    good = awfm.pair_inputs(*pointers)
    assert raw(None, a.num_pairs) == -4 and raw(good, a.num_pairs, None) == -4 and raw(good, a.num_pairs, histogram=None) == -4
    assert raw(good, a.num_pairs, image=None) == -4
    for k in range(5):
        assert raw(awfm.pair_inputs(*[0 if j == k else v for j, v in enumerate(pointers)]), a.num_pairs) == -4, k
    assert raw(None, 0, None, None) == awfm.AwFmSuccess  # numPairs == 0 touches nothing
    assert lib.awfmGpuInsertInterval(None, target, C.byref(params), d_estimate.data_ptr() + GUARD, None) == -4
    assert lib.awfmGpuInsertInterval(g.handle, None, C.byref(params), d_estimate.data_ptr() + GUARD, None) == -4
    assert lib.awfmGpuInsertInterval(g.handle, target, None, d_estimate.data_ptr() + GUARD, None) == -4
    assert lib.awfmGpuInsertInterval(g.handle, target, C.byref(params), None, None) == -4
    torch.cuda.synchronize()
    got = HistogramCall.collect(untouched)
    assert not got[0].any() and got[1:] == (5, 6)
    assert (body_of(d_estimate, np.uint8, "the estimate") == PATTERN).all()


def test_interval_on_full_bins_at_either_end_counts_above_2_to_the_32_and_the_fallback(awfm, g):
    import torch
    ip = dict(ic.PARAMS, low_template=-100, high_template=-100 + ic.MAX_BINS - 1, spread=3, min_samples=10)
    for filled in ({0: 77}, {65535: 77}, {0: (1 << 33) + 5, 65535: 1 << 33}, {17: 1 << 46, 40000: (1 << 45) + 1, 40001: 3}, {5: 9}, {}):
        h = np.zeros(ic.MAX_BINS, np.uint64)
        for at, count in filled.items():
            h[at] = count
        want = ic.interval_expected(h, ip)
        assert want["valid"] == (sum(filled.values()) >= 10)
        got = device_interval(awfm, torch, g, h, ip)
        ic.check_estimate(got, want, what=str(filled))
        assert got == awfm.insert_interval_host(h, awfm.insert_params(**ip))
    # the quartiles where they fall into different chunks and different waves of the one workgroup, on a small and a large range
    rng = np.random.default_rng(3)
    for bins in (1, 5, 1023, 1024, 1025, 4096, 65536):
        ip = dict(ic.PARAMS, low_template=-40, high_template=bins - 41, spread=1)
        h = rng.integers(0, 1 << 28, bins).astype(np.uint64) * (rng.random(bins) < 0.3)
        h[rng.integers(0, bins)] += np.uint64(1)
        assert device_interval(awfm, torch, g, h, ip) == awfm.insert_interval_host(h, awfm.insert_params(**ip)), bins


class Estimated:
    """stands where DeviceCall expects the image: pair_mates through awfmGpuPairMatesEstimated, the interval in a struct on the
    device (interval None: the one the call would have passed from the host); the other six words hold anything"""

    def __init__(self, g, torch, interval=None):
        self.g, self.torch, self.interval, self.kept = g, torch, interval, []

    def pair_mates(self, inputs, num_pairs, outputs, min_insert, max_insert, **kw):
        lo, hi = (min_insert, max_insert) if self.interval is None else self.interval
        self.kept.append(_upload(self.torch, np.array([lo, hi, -1, 7, 1 << 62, 0, 0, 0], np.int64)))
        self.g.pair_mates_estimated(inputs, num_pairs, outputs, self.kept[-1].data_ptr(), **kw)


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_estimated_pairing_equals_pairing_with_the_same_interval(awfm, g, diag, group):
    import torch
    diag(pair_group=group)
    proxy = Estimated(g, torch)
    cases = [case for slots in (4, 16) for case, _ in pm.edge_cases(slots)]
    cases += [pm.random_case(40 + k, pairs, slots, params) for k, (pairs, slots, params) in enumerate((
        (300, 4, {}), (257, 1, dict(min_insert=-400, max_insert=-150, unpaired_penalty=0)), (65, 5, dict(min_score=4, mapq_cap=254)),
        (129, 16, dict(min_insert=-ic.MAX_INSERT, max_insert=ic.MAX_INSERT))))]
    for case in cases:
        call = DeviceCall(awfm, torch, case)
        want = call(g, proper_before=3, windows_before=1 << 33)
        pm.assert_equal(call(proxy, proper_before=3, windows_before=1 << 33), want, what=f"{case.num_pairs} pairs C={case.C}")
    call = DeviceCall(awfm, torch, cases[-4])
    want = call(g)
    assert want["numProper"] > 40 and want["numWindows"] > 10
    for missing in pm.NAMES:  # every output NULL in turn, and alone
        for outputs in ([n for n in pm.NAMES if n != missing], [missing]):
            got = call(proxy, outputs=outputs)
            assert sorted(got) == sorted(outputs)
            pm.assert_equal(got, want, names=outputs, what=str(outputs))


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_an_interval_that_is_not_usable_makes_no_pair_proper_and_names_no_window(awfm, g, diag, group):
    import torch
    diag(pair_group=group)
    case = pm.random_case(61, 300, 4)
    # the restatement with an interval no T lies in, and no window: what the rules leave of a pairing without concordant pairs
    want = pm.expected(pm.Case(case.offsets, case.slots, case.qualities, dict(case.params, min_insert=1, max_insert=0)), 5, 7)
    assert want["numProper"] == 5 and (want["windowSequences"] != pm.NO_WINDOW).sum() > 100 and (want["pairScores"] > 0).sum() > 100
    want["windowSequences"][...], want["windowBegins"][...], want["windowEnds"][...], want["numWindows"] = pm.NO_WINDOW, 0, 0, 7
    call = DeviceCall(awfm, torch, case)
    M = ic.MAX_INSERT
    for interval in ((501, 500), (-M - 1, 500), (200, M + 1), (1 << 62, -(1 << 62))):
        got = call(Estimated(g, torch, interval), proper_before=5, windows_before=7)
        pm.assert_equal(got, want, what=str(interval))
    # the limits themselves are usable
    for interval in ((-M, M), (300, 300)):
        got = call(Estimated(g, torch, interval))
        pm.assert_equal(got, case.host(awfm, threads=16, min_insert=interval[0], max_insert=interval[1]), what=str(interval))
    # what the host can see it still refuses, and an estimate it needs
    with pytest.raises(awfm.AwFmError) as e:
        call(Estimated(g, torch, (200, 500)), mapq_cap=255)
    assert e.value.rc == awfm.AwFmIllegalPositionError
    pout = awfm.pair_outputs()
    with pytest.raises(awfm.AwFmError) as e:
        g.pair_mates_estimated(call.inputs, case.num_pairs, pout, 0)
    assert e.value.rc == -4


def test_an_estimate_written_on_the_stream_is_consumed_without_a_synchronisation(awfm, g):
    import torch
    case, ip = table(77, 3000, 4)
    ip = dict(ip, spread=1)
    hist = HistogramCall(awfm, torch, case)
    pairing = DeviceCall(awfm, torch, case)
    stream = torch.cuda.Stream()
    buffers = hist.buffers(ip)
    d_estimate = guarded(torch, np.array([501, 500, 0, 0, 0, 0, 0, 0], np.int64))  # (what lies there before is not usable)
    collected = {}

    class Behind:
        """pair_mates as DeviceCall calls it: histogram, interval and estimated pairing on the stream, nothing in between"""

        @staticmethod
        def pair_mates(inputs, num_pairs, outputs, min_insert, max_insert, stream=0, **kw):
            hist.enqueue(g, ip, buffers, stream=stream)
            g.insert_interval(buffers[0].data_ptr() + GUARD, awfm.insert_params(**ip), d_estimate.data_ptr() + GUARD, stream=stream)
            g.pair_mates_estimated(inputs, num_pairs, outputs, d_estimate.data_ptr() + GUARD, stream=stream, **kw)

    _, collect = pairing.run(Behind, stream=stream.cuda_stream)
    torch.cuda.synchronize()
    collected = collect()
    want_histogram = hist.host(ip)
    same(HistogramCall.collect(buffers), want_histogram, what="histogram")
    estimate = awfm.insert_estimate_dict(body_of(d_estimate, np.uint8, "the estimate"))
    assert estimate == awfm.insert_interval_host(want_histogram[0], awfm.insert_params(**ip)) and estimate["valid"] == 1
    want = case.host(awfm, threads=16, min_insert=estimate["minInsert"], max_insert=estimate["maxInsert"])
    assert want["numProper"] > 300
    pm.assert_equal(collected, want, what="behind the interval")


class EstimatingDeviceSide(DeviceSide):
    """the loop's calls on the device, the interval estimated there after the first slot scores: histogram, interval and every
    pairing read and write device memory only"""

    def pair(self, slots, scored):
        torch, awfm = self.torch, self.awfm
        fields = {name: (dtype, self.n // 2) for name, dtype in pm.PAIR_OUTPUTS.items()}
        fields.update({name: (dtype, self.n) for name, dtype in pm.READ_OUTPUTS.items()})
        fields.update(numProper=(np.uint64, 1), numWindows=(np.uint64, 1))
        out = self.buffers(fields)
        pin = awfm.pair_inputs(self.offsets.data_ptr(), self.slots["sequences"].data_ptr(), scored["slotScores"].data_ptr(),
                               scored["slotReadEnds"].data_ptr(), scored["slotTextEnds"].data_ptr(), scored["mappingQualities"].data_ptr())
        if not hasattr(self, "estimate"):
            params = awfm.insert_params(**ic.E2E_INSERT)
            self.histogram = torch.zeros(ic.bins_of(ic.E2E_INSERT), dtype=torch.int64, device="cuda")
            self.counters = torch.zeros(2, dtype=torch.int64, device="cuda")
            self.estimate = torch.zeros(8, dtype=torch.int64, device="cuda")
            self.g.insert_histogram(pin, self.n // 2, params, self.histogram.data_ptr(), self.counters.data_ptr(), self.counters.data_ptr() + 8,
                                    max_candidates=self.C)
            self.g.insert_interval(self.histogram.data_ptr(), params, self.estimate.data_ptr())
        E = pm.E2E
        self.g.pair_mates_estimated(pin, self.n // 2, awfm.pair_outputs(**{name: t.data_ptr() for name, t in out.items()}), self.estimate.data_ptr(),
                                    max_candidates=self.C, min_score=E["min_score"], unpaired_penalty=E["unpaired_penalty"], window_pad=E["window_pad"],
                                    mapq_cap=E["mapq_cap"])
        self.pairings = getattr(self, "pairings", []) + [(out, fields)]
        return out


def test_end_to_end_from_a_fasta_file_with_the_interval_estimated_on_the_device(awfm, require_gpu, tmp_path):
    """tests/pair_mates_common.py EndToEnd with no insert interval given: slot scores, histogram, interval, estimated pairing,
    window scores, slot scores, estimated pairing, affine alignment on the device, nothing downloaded before the final comparison;
    equal to the host loop of tests/test_insert_size.py and held to the same conditions"""
    import torch
    e = pm.EndToEnd(awfm, tmp_path)
    image = awfm.GpuIndex(e.ix)
    try:
        image.set_text(e.text)
        side = EstimatingDeviceSide(awfm, torch, image, e)
        _, _, aligned = e.loop(side)
        first, second = (side.home(out, fields) for out, fields in side.pairings)
        for pairing in (first, second):
            pairing["numProper"], pairing["numWindows"] = int(pairing["numProper"][0]), int(pairing["numWindows"][0])
        estimate = awfm.insert_estimate_dict(side.estimate.cpu().numpy())
        ic.check_end_to_end(e, estimate, second, aligned)
        host = ic.EstimatingHostSide(awfm, e)
        want_first, want_second, want_aligned = e.loop(host)
        assert np.array_equal(side.histogram.cpu().numpy().view(np.uint64), host.estimate.pop("histogram"))
        assert int(side.counters[1]) == host.estimate.pop("numOutside") and int(side.counters[0]) == estimate["numSamples"]
        assert estimate == host.estimate
        pm.assert_equal(first, want_first, what="first pairing")
        pm.assert_equal(second, want_second, what="second pairing")
        for name, _ in awfm.AFFINE_READ_OUTPUTS:
            assert np.array_equal(aligned[name], want_aligned[name]), name
    finally:
        image.destroy()
        e.close()
