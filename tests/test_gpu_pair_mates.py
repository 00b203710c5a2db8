"""awfmGpuPairMates and awfmGpuReverseComplementReads (include/awfm_gpu.h "pair mates", csrc/awfm_pair_mates_kernel.h) against their
host twins, which tests/test_pair_mates.py pins to the plain-Python restatement and to hand-computed values: every output and both
counters, bit for bit -- on the edge list with sixteen lanes a pair and with a wave a pair, on batches whose last group, wave and
workgroup end inside them for 1, 4, 5 and 16 slots a read, on more pairs than the grid has groups, from two streams at once, with
every output NULL in turn, with the qualities updated in place and with bad arguments; the reverse complement on read lengths
around every edge of the layout at every alignment of input and output, under the three selections, with malformed reads and up
to the last byte of an allocation; and end to end from a FASTA file held on both strands.  Every output lies between guard
words."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_mates_common as pm  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, _upload  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = dict(pm.PAIR_OUTPUTS, **pm.READ_OUTPUTS)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avxwindowfmindex_amd", "csrc")


@pytest.fixture(scope="module")
def g(awfm, require_gpu):
    """an image: the calls take it for its device only"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtaacc", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    image = awfm.GpuIndex(ix)
    yield image
    image.destroy()
    ix.dealloc()


def size_of(name, case):
    if name in pm.COUNTERS:
        return 8
    return np.dtype(DTYPES[name]).itemsize * (case.num_pairs if name in pm.PAIR_OUTPUTS else case.num_reads)


class DeviceCall:
    """the arrays of one case on the device and guarded outputs for calls on them"""

    def __init__(self, awfm, torch, case):
        self.awfm, self.torch, self.case = awfm, torch, case
        self.arrays = [_upload(torch, case.offsets)] + [_upload(torch, case.slots[name]) for name in pm.SLOT_INPUTS]
        self.qualities = None if case.qualities is None else _upload(torch, case.qualities)
        self.inputs = awfm.pair_inputs(*(a.data_ptr() for a in self.arrays), 0 if self.qualities is None else self.qualities.data_ptr())

    def run(self, g, outputs=None, stream=0, proper_before=0, windows_before=0, launch=True, **kw):
        torch, case = self.torch, self.case
        outputs = pm.NAMES if outputs is None else list(outputs)
        buffers = {name: torch.full((size_of(name, case) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        for name, before in (("numProper", proper_before), ("numWindows", windows_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        pout = self.awfm.pair_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        params = dict(case.params, **kw)
        torch.cuda.synchronize()

        def enqueue():
            g.pair_mates(self.inputs, case.num_pairs, pout, max_candidates=params.pop("max_candidates", case.C), stream=stream, **params)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), size_of(name, case)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                result[name] = int(body.view(np.uint64)[0]) if name in pm.COUNTERS else body.view(DTYPES[name])
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, **kw):
        _, collect = self.run(g, **kw)
        self.torch.cuda.synchronize()
        return collect()


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_edge_list_equals_the_host_twin_and_the_hand_computed_values(awfm, g, diag, group):
    import torch
    diag(pair_group=group)
    for slots in (4, 16):
        for case, edges in pm.edge_cases(slots):
            got = DeviceCall(awfm, torch, case)(g, proper_before=9, windows_before=2)
            pm.assert_equal(got, case.host(awfm, threads=16, proper_before=9, windows_before=2), what=f"{edges[0].name} C={slots}")
            got["numProper"] -= 9
            got["numWindows"] -= 2
            pm.check_edges(got, edges, what=f"C={slots}")


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
@pytest.mark.parametrize("slots", [1, 4, 5, 16])
def test_batches_that_end_inside_a_group_a_wave_and_a_workgroup(awfm, g, diag, slots, group):
    import torch
    if group == 64 and slots > 4:
        return  # (a wave per pair is the natural layout there)
    diag(pair_group=group)
    settings = ({}, dict(min_score=4, unpaired_penalty=3, window_pad=0, mapq_cap=254), dict(min_insert=-400, max_insert=-150, unpaired_penalty=0))
    for k, pairs in enumerate((1, 3, 4, 5, 63, 64, 65, 4097)):
        case = pm.random_case(1000 * slots + pairs, pairs, slots, settings[k % 3], qualities=k % 4 != 3, big=k % 2 == 1)
        want = case.host(awfm, threads=16, proper_before=1, windows_before=1 << 33)
        pm.assert_equal(DeviceCall(awfm, torch, case)(g, proper_before=1, windows_before=1 << 33), want, what=f"{pairs} pairs")


def _constant(name):
    text = open(os.path.join(CSRC, "awfm_pair_mates_kernel.h")).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", text).group(1))


def test_more_pairs_than_the_grid_has_groups(awfm, g):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = cus * _constant("kPairBlocksPerCU") * (_constant("kPairThreads") // 16)  # the grid's groups of sixteen lanes
    case = pm.random_case(77, groups + groups // 2 + 3, 4)
    want = case.host(awfm, threads=16)
    assert want["numProper"] > groups // 4 and want["numWindows"] > groups // 16
    pm.assert_equal(DeviceCall(awfm, torch, case)(g), want)


def test_two_streams_null_outputs_in_place_and_bad_arguments(awfm, g, diag):
    import ctypes as C
    import torch
    a, b = pm.random_case(31, 3000, 4), pm.random_case(32, 2000, 16, dict(mapq_cap=254))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
    collects = [call.run(g, stream=s.cuda_stream)[1] for call, s in zip(calls, streams)]
    torch.cuda.synchronize()
    want = a.host(awfm, threads=16)
    pm.assert_equal(collects[0](), want, what="first stream")
    pm.assert_equal(collects[1](), b.host(awfm, threads=16), what="second stream")
    call = calls[0]
    for layout in (None, 64):
        diag(pair_group=layout)
        for missing in pm.NAMES:  # every output NULL in turn, and alone
            for outputs in ([n for n in pm.NAMES if n != missing], [missing]):
                got = call(g, outputs=outputs)
                assert sorted(got) == sorted(outputs)
                pm.assert_equal(got, want, names=outputs, what=str(outputs))
    # the output qualities may be the input array
    in_place = awfm.pair_outputs(mappingQualities=call.qualities.data_ptr())
    g.pair_mates(call.inputs, a.num_pairs, in_place, max_candidates=4, **a.params)
    torch.cuda.synchronize()
    assert np.array_equal(call.qualities.cpu().numpy(), want["mappingQualities"])
    # every bad argument: nothing is launched, the outputs keep the pattern
    call = DeviceCall(awfm, torch, a)
    bad = awfm.AwFmIllegalPositionError
    for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(min_insert=501), dict(min_insert=-(1 << 40) - 1),
               dict(max_insert=(1 << 40) + 1), dict(mapq_cap=255)):
        enqueue, collect = call.run(g, launch=False, **kw)
        with pytest.raises(awfm.AwFmError) as e:
            enqueue()
        assert e.value.rc == bad, kw
        torch.cuda.synchronize()
        got = collect()
        assert all((np.asarray(got[name]).view(np.uint8) == PATTERN).all() for name in DTYPES), kw
    lib, params = awfm._lib.lib(), awfm.pair_params(**a.params)
    d_slots = torch.full((4 * a.num_reads,), PATTERN, dtype=torch.uint8, device="cuda")
    guarded = awfm.pair_outputs(pairSlots=d_slots.data_ptr())
    pointers = [t.data_ptr() for t in call.arrays]

    def raw(inputs, pairs, outputs, settings=params, image=g.handle):
        return lib.awfmGpuPairMates(image, None if inputs is None else C.byref(inputs), pairs, 4, None if settings is None else C.byref(settings),
                                    None if outputs is None else C.byref(outputs), None)

    good = awfm.pair_inputs(*pointers)
    assert raw(None, a.num_pairs, guarded) == -4 and raw(good, a.num_pairs, None) == -4 and raw(good, a.num_pairs, guarded, None) == -4
    assert raw(good, a.num_pairs, guarded, image=None) == -4
    for k in range(5):
        missing = awfm.pair_inputs(*[0 if j == k else v for j, v in enumerate(pointers)])
        assert raw(missing, a.num_pairs, guarded) == -4, k
    assert raw(good, 1 << 31, guarded) == bad
    assert raw(None, 0, None, None) == awfm.AwFmSuccess  # numPairs == 0 touches nothing
    torch.cuda.synchronize()
    assert (d_slots.cpu().numpy() == PATTERN).all()  # nothing was launched
    assert raw(good, a.num_pairs, guarded) == awfm.AwFmSuccess  # (the arguments the refused calls differ from)
    torch.cuda.synchronize()
    assert np.array_equal(d_slots.cpu().numpy().view(np.uint32), want["pairSlots"])


LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("which", [pm.ALL, pm.ODD, pm.EVEN], ids=["all", "odd", "even"])
def test_reverse_complement_at_every_alignment(awfm, g, which):
    """every length of the list several times over, forwards and backwards behind a lead of 7 bytes, so that each begins off the
    multiples of 16 at least once; input and output 0 to 3 bytes into their allocations, independently"""
    import torch
    order = LENGTHS + [3] + LENGTHS[::-1] + [5] + LENGTHS[3:] + [7, 64, 9, 16]
    chars, offsets = pm.reads_buffer(11 + which, order, lead=7)
    for n in LENGTHS:  # every length begins off the multiples of 16, and the reads begin at every offset mod 4
        assert any(int(offsets[r]) % 16 for r, length in enumerate(order) if length == n), n
    assert {int(o) % 4 for o in offsets} == {0, 1, 2, 3}
    want, _ = awfm.reverse_complement_reads_host(chars, offsets, which, threads=16, fill=PATTERN)
    assert np.array_equal(want, pm.reverse_complement(chars, offsets, which, fill=PATTERN)[0])
    d_offsets = _upload(torch, offsets)
    for skew_in in range(4):
        for skew_out in range(4):
            d_chars = torch.from_numpy(np.concatenate((np.full(GUARD + skew_in, PATTERN, np.uint8), chars, np.full(GUARD, PATTERN, np.uint8)))).to("cuda")
            d_out = torch.full((chars.size + 2 * GUARD + skew_out,), PATTERN, dtype=torch.uint8, device="cuda")
            d_malformed = _upload(torch, np.array([5], np.uint64))
            g.reverse_complement_reads(d_chars.data_ptr() + GUARD + skew_in, chars.size, d_offsets.data_ptr(), len(order),
                                       d_out.data_ptr() + GUARD + skew_out, which, d_malformed.data_ptr())
            torch.cuda.synchronize()
            raw = d_out.cpu().numpy()
            assert (raw[:GUARD + skew_out] == PATTERN).all() and (raw[GUARD + skew_out + chars.size:] == PATTERN).all(), (skew_in, skew_out)
            assert np.array_equal(raw[GUARD + skew_out:GUARD + skew_out + chars.size], want), (skew_in, skew_out)
            assert int(d_malformed.cpu().numpy().view(np.uint64)[0]) == 5


def test_reverse_complement_to_the_last_byte_malformed_reads_and_bad_arguments(awfm, g):
    import torch
    # allocations of exactly the buffer's size: the last read ends at the last byte of both
    chars, offsets = pm.reads_buffer(21, [150] * 37 + [149], lead=0)
    d_chars, d_offsets = torch.from_numpy(chars).to("cuda"), _upload(torch, offsets)
    d_out = torch.zeros(chars.size, dtype=torch.uint8, device="cuda")
    g.reverse_complement_reads(d_chars.data_ptr(), chars.size, d_offsets.data_ptr(), 38, d_out.data_ptr(), pm.ODD)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), awfm.reverse_complement_reads_host(chars, offsets, pm.ODD)[0])
    # inverted offsets and offsets beyond the buffer: neither read nor written, counted
    bad = np.array([30, 40, 0, 30, 62, 62, 1 << 40], np.uint64)
    for limit in (60, 35):
        want, malformed = awfm.reverse_complement_reads_host(chars[:60], bad, pm.ALL, fill=PATTERN, num_read_chars=limit, malformed_before=2)
        d_out = torch.full((60 + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        d_malformed = _upload(torch, np.array([2], np.uint64))
        g.reverse_complement_reads(d_chars.data_ptr(), limit, _upload(torch, bad).data_ptr(), 6, d_out.data_ptr() + GUARD, pm.ALL,
                                   d_malformed.data_ptr())
        torch.cuda.synchronize()
        raw = d_out.cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + 60:] == PATTERN).all() and np.array_equal(raw[GUARD:GUARD + 60], want), limit
        assert int(d_malformed.cpu().numpy().view(np.uint64)[0]) == malformed == (6 if limit == 60 else 7)
    # overlap, an unknown selection, NULL arguments, no reads, no output
    base = d_chars.data_ptr()
    for source, target, which, d_off, reads, rc in ((base, base, pm.ALL, d_offsets.data_ptr(), 38, awfm.AwFmIllegalPositionError),
                                                    (base, base + chars.size - 1, pm.ALL, d_offsets.data_ptr(), 38, awfm.AwFmIllegalPositionError),
                                                    (base, d_out.data_ptr(), 3, d_offsets.data_ptr(), 38, awfm.AwFmIllegalPositionError),
                                                    (0, d_out.data_ptr(), pm.ALL, d_offsets.data_ptr(), 38, -4),
                                                    (base, d_out.data_ptr(), pm.ALL, 0, 38, -4)):
        with pytest.raises(awfm.AwFmError) as e:
            g.reverse_complement_reads(source, chars.size, d_off, reads, target, which)
        assert e.value.rc == rc
    g.reverse_complement_reads(0, chars.size, 0, 0, 0, 9)  # numReads == 0 touches nothing
    d_malformed = _upload(torch, np.array([0], np.uint64))
    g.reverse_complement_reads(base, 60, _upload(torch, bad).data_ptr(), 6, 0, pm.ALL, d_malformed.data_ptr())  # counts only
    torch.cuda.synchronize()
    assert int(d_malformed.cpu().numpy().view(np.uint64)[0]) == 4
    assert np.array_equal(d_chars.cpu().numpy(), chars)


class DeviceSide:
    """the loop's four calls on the device, every array resident there: nothing comes home between the calls"""

    def __init__(self, awfm, torch, g, e):
        import verify_chains_common as vc
        self.awfm, self.torch, self.g, self.e, self.vc = awfm, torch, g, e, vc
        self.n, self.C = e.offsets.size - 1, pm.E2E["slots"]
        # call 1 on the device: mate 2 as sequenced -> one strand
        d_sequenced = _upload(torch, e.sequenced)
        self.chars = torch.zeros(e.sequenced.size, dtype=torch.uint8, device="cuda")
        self.offsets = _upload(torch, e.offsets)
        g.reverse_complement_reads(d_sequenced.data_ptr(), e.sequenced.size, self.offsets.data_ptr(), self.n, self.chars.data_ptr(), pm.ODD)
        self.slots = {name: _upload(torch, e.slots[name]) for name in vc.SLOT_FIELDS}  # ONE table: the window call writes into it
        self.vin = awfm.verify_inputs(self.chars.data_ptr(), e.sequenced.size, self.offsets.data_ptr(), **{name: t.data_ptr() for name, t in self.slots.items()})
        self.common = dict(band_pad=8, max_drift=15, scoring=pm.E2E["scoring"])
        self.kept = []

    def buffers(self, fields):
        out = {name: self.torch.zeros(count * np.dtype(dtype).itemsize, dtype=self.torch.uint8, device="cuda") for name, (dtype, count) in fields.items()}
        self.kept.append(out)
        return out

    def home(self, buffers, fields):
        self.torch.cuda.synchronize()
        return {name: buffers[name].cpu().numpy().view(fields[name][0]) for name in fields}

    def score(self, slots):
        fields = {"slotScores": (np.uint32, self.n * self.C), "slotReadEnds": (np.uint32, self.n * self.C), "slotTextEnds": (np.uint64, self.n * self.C),
                  "mappingQualities": (np.uint8, self.n)}
        out = self.buffers(fields)
        self.g.score_chains_affine(self.vin, self.n, self.awfm.slot_score_outputs(**{name: t.data_ptr() for name, t in out.items()}),
                                   max_candidates=self.C, min_score=pm.E2E["min_score"], mapq_cap=pm.E2E["mapq_cap"], **self.common)
        return out

    def pair(self, slots, scored):
        fields = {name: (dtype, self.n // 2) for name, dtype in pm.PAIR_OUTPUTS.items()}
        fields.update({name: (dtype, self.n) for name, dtype in pm.READ_OUTPUTS.items()})
        fields.update(numProper=(np.uint64, 1), numWindows=(np.uint64, 1))
        out = self.buffers(fields)
        pin = self.awfm.pair_inputs(self.offsets.data_ptr(), self.slots["sequences"].data_ptr(), scored["slotScores"].data_ptr(),
                                    scored["slotReadEnds"].data_ptr(), scored["slotTextEnds"].data_ptr(), scored["mappingQualities"].data_ptr())
        self.g.pair_mates(pin, self.n // 2, self.awfm.pair_outputs(**{name: t.data_ptr() for name, t in out.items()}), pm.E2E["min_insert"],
                          pm.E2E["max_insert"], max_candidates=self.C, min_score=pm.E2E["min_score"], unpaired_penalty=pm.E2E["unpaired_penalty"],
                          window_pad=pm.E2E["window_pad"], mapq_cap=pm.E2E["mapq_cap"])
        self.pairings = getattr(self, "pairings", []) + [(out, fields)]
        return out

    def windows(self, pairing, slots):
        win = self.awfm.window_inputs(self.chars.data_ptr(), self.e.sequenced.size, self.offsets.data_ptr(), pairing["windowSequences"].data_ptr(),
                                      pairing["windowBegins"].data_ptr(), pairing["windowEnds"].data_ptr())
        scratch = self.torch.zeros(self.g.score_windows_affine_scratch_bytes(pm.E2E["length"]), dtype=self.torch.uint8, device="cuda")
        self.kept.append(scratch)
        self.g.score_windows_affine(win, self.n, self.awfm.window_score_outputs(**{name: t.data_ptr() for name, t in self.slots.items()}),
                                    scratch.data_ptr(), pm.E2E["length"], scoring=pm.E2E["scoring"], min_score=pm.E2E["min_score"],
                                    slot_stride=self.C, slot_column=self.C - 1)
        return self.slots

    def align(self, slots, chosen):
        fields = {name: (dtype, self.n) for name, dtype in self.awfm.AFFINE_READ_OUTPUTS}
        out = self.buffers(fields)
        scratch = self.torch.zeros(self.g.align_chains_affine_scratch_bytes(pm.E2E["length"]), dtype=self.torch.uint8, device="cuda")
        self.kept.append(scratch)
        self.g.align_chains_affine(self.vin, chosen.data_ptr(), self.n, self.awfm.affine_outputs(**{name: t.data_ptr() for name, t in out.items()}),
                                   scratch.data_ptr(), max_candidates=self.C, max_ops=pm.E2E["max_ops"], max_rows=pm.E2E["length"], **self.common)
        return self.home(out, fields)


def test_end_to_end_from_a_fasta_file_held_on_both_strands(awfm, require_gpu, tmp_path):
    """tests/pair_mates_common.py EndToEnd: 96 pairs as sequenced, planted on either strand of three records; call 1, then the
    loop of the header on the device without a download in between -- slot scores, pairing, window scores on the windows the
    pairing names (into the free column of the one slot table), slot scores, pairing, affine alignment with pairSlots.  Every
    plain pair is proper at once, every mate the seeds cannot place is rescued and its pair proper at the planted place, every
    pair outside the insert interval stays improper with windows for both reads, the alignments are the planted intervals; and
    both pairings and the alignments equal the host twins' (tests/test_pair_mates.py holds those to the same conditions)."""
    import torch
    e = pm.EndToEnd(awfm, tmp_path)
    g = awfm.GpuIndex(e.ix)
    try:
        g.set_text(e.text)
        assert g.num_records == len(e.records)
        side = DeviceSide(awfm, torch, g, e)
        _, _, aligned = e.loop(side)
        assert np.array_equal(side.chars.cpu().numpy(), e.chars)  # call 1
        first, second = (side.home(out, fields) for out, fields in side.pairings)
        for pairing in (first, second):
            pairing["numProper"], pairing["numWindows"] = int(pairing["numProper"][0]), int(pairing["numWindows"][0])
        e.check(first, second, aligned)
        want_first, want_second, want_aligned = e.loop(pm.HostSide(awfm, e))
        pm.assert_equal(first, want_first, what="first pairing")
        pm.assert_equal(second, want_second, what="second pairing")
        for name, _ in awfm.AFFINE_READ_OUTPUTS:
            assert np.array_equal(aligned[name], want_aligned[name]), name
    finally:
        g.destroy()
        e.close()
