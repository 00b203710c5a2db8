"""awfmGpuChooseStrands and awfmGpuOrientReads (include/awfm_gpu.h "strands", csrc/awfm_strands_kernel.h) against their host twins,
which tests/test_strands.py pins to the plain-Python restatement and to hand-computed values: every output and all four counters,
bit for bit -- on the edge list with the natural group and with a wave a pair or read, on batches whose last group, wave and
workgroup end inside them for 1, 4, 5 and 16 slots a row, on more pairs than the grid has groups, from two streams at once, with
every output NULL in turn, with counters that start nonzero and with every refusal; the orienting gather on every read length
around the edges of its layout at every alignment of source and destination, in tensors of exactly the buffers' sizes, with
malformed reads and its refusals; and end to end from a FASTA file indexed on one strand.  Every output lies between guard
words."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strands_common as st  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, _upload  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = st.dtypes()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "avxwindowfmindex_amd", "csrc")
BEFORE = dict(numReverse=5, numProper=9, numWindows=1 << 33, numMalformed=2)
SETTINGS = ({}, dict(min_score=4, unpaired_penalty=3, window_pad=0, mapq_cap=254), dict(min_insert=-400, max_insert=-150, unpaired_penalty=0))
SIZES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 65, 257)


@pytest.fixture(scope="module")
def g(awfm, require_gpu):
    """an image: the calls take it for its device only"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtaacc", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    image = awfm.GpuIndex(ix)
    yield image
    image.destroy()
    ix.dealloc()


def size_of(name, case):
    if name in st.COUNTERS:
        return 8
    count = case.num_reads if name in st.READ_OUTPUTS else case.num_rows if name in st.ROW_OUTPUTS else case.num_reads // 2
    return np.dtype(DTYPES[name]).itemsize * count


class DeviceCall:
    """the arrays of one case on the device and guarded outputs for calls on them"""

    def __init__(self, awfm, torch, case):
        self.awfm, self.torch, self.case = awfm, torch, case
        self.arrays = [_upload(torch, case.offsets)] + [_upload(torch, case.slots[name]) for name in st.SLOT_INPUTS]
        self.inputs = awfm.strand_inputs(*(a.data_ptr() for a in self.arrays))

    def run(self, g, paired, outputs=None, stream=0, before=None, launch=True, **kw):
        torch, case = self.torch, self.case
        outputs = st.names(paired) if outputs is None else list(outputs)
        buffers = {name: torch.full((size_of(name, case) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        for name in st.COUNTERS:
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([(before or {}).get(name, 0)], np.uint64).view(np.uint8)).to("cuda")
        sout = self.awfm.strand_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        params = dict(case.params, **kw)
        torch.cuda.synchronize()

        def enqueue():
            g.choose_strands(self.inputs, params.pop("num_reads", case.num_reads), sout, paired=paired, max_candidates=params.pop("max_candidates", case.C),
                             stream=stream, **params)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), size_of(name, case)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                result[name] = int(body.view(np.uint64)[0]) if name in st.COUNTERS else body.view(DTYPES[name])
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, paired, **kw):
        _, collect = self.run(g, paired, **kw)
        self.torch.cuda.synchronize()
        return collect()


@pytest.mark.parametrize("paired", [False, True], ids=["unpaired", "paired"])
@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_edge_list_equals_the_host_twin_and_the_hand_computed_values(awfm, g, diag, group, paired):
    import torch
    diag(strand_group=group)
    for slots in (4, 16):
        for case, edges in st.edge_cases(slots):
            got = DeviceCall(awfm, torch, case)(g, paired, before=BEFORE)
            st.assert_equal(got, case.host(awfm, paired, threads=16, before=BEFORE), st.names(paired), what=f"{edges[0].name} C={slots}")
            for name, value in BEFORE.items():
                got[name] -= value
            st.check_edges(got, edges, paired, what=f"C={slots}")


# (paired with more than four slots a row, a wave per pair is the natural layout: those cases are not run twice)
BATCH_LAYOUTS = [(slots, group, paired) for slots in (1, 4, 5, 16) for group in (None, 64) for paired in (False, True)
                 if not (group == 64 and paired and slots > 4)]


@pytest.mark.parametrize("slots,group,paired", BATCH_LAYOUTS, ids=[f"{s}-{g or 'natural'}-{'paired' if p else 'unpaired'}" for s, g, p in BATCH_LAYOUTS])
def test_batches_that_end_inside_a_group_a_wave_and_a_workgroup(awfm, g, diag, slots, group, paired):
    import torch
    diag(strand_group=group)
    for k, size in enumerate(SIZES):
        reads = 2 * size if paired else size
        case = st.random_case(1000 * slots + size, reads, slots, SETTINGS[k % 3], big=k % 2 == 1)
        want = case.host(awfm, paired, threads=16, before=BEFORE)
        st.assert_equal(DeviceCall(awfm, torch, case)(g, paired, before=BEFORE), want, st.names(paired), what=f"{reads} reads")


def _constant(name):
    text = open(os.path.join(CSRC, "awfm_strands_kernel.h")).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", text).group(1))


@pytest.mark.parametrize("slots", [4, 16])
def test_five_more_pairs_than_the_grid_has_groups(awfm, g, slots):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_cu, lanes = (_constant("kStrandBlocksPerCU"), 32) if slots == 4 else (_constant("kStrandWaveBlocksPerCU"), 64)
    groups = cus * per_cu * (_constant("kStrandThreads") // lanes)
    case = st.random_case(77 + slots, 2 * (groups + 5), slots)
    want = case.host(awfm, True, threads=16)
    assert want["numProper"] > groups // 8 and want["numWindows"] > groups // 32
    st.assert_equal(DeviceCall(awfm, torch, case)(g, True), want, st.names(True))


def test_more_reads_than_the_grid_has_groups_unpaired(awfm, g):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    groups = cus * _constant("kStrandBlocksPerCU") * (_constant("kStrandThreads") // 16)
    case = st.random_case(78, groups + 5, 4)
    st.assert_equal(DeviceCall(awfm, torch, case)(g, False), case.host(awfm, False, threads=16), st.names(False))


def test_two_streams_null_outputs_and_bad_arguments(awfm, g, diag):
    import torch
    a, b = st.random_case(31, 3000, 4), st.random_case(32, 2000, 16, dict(mapq_cap=254))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
    collects = [call.run(g, True, stream=s.cuda_stream)[1] for call, s in zip(calls, streams)]
    torch.cuda.synchronize()
    want = a.host(awfm, True, threads=16)
    st.assert_equal(collects[0](), want, st.names(True), what="first stream")
    st.assert_equal(collects[1](), b.host(awfm, True, threads=16), st.names(True), what="second stream")
    call = calls[0]
    for paired in (True, False):
        want = a.host(awfm, paired, threads=16)
        for layout in (None, 64):
            diag(strand_group=layout)
            for missing in st.names(paired):  # every output NULL in turn, and alone
                for outputs in ([n for n in st.names(paired) if n != missing], [missing]):
                    got = call(g, paired, outputs=outputs)
                    assert sorted(got) == sorted(outputs)
                    st.assert_equal(got, want, outputs, what=str(outputs))
    diag(strand_group=None)
    # unpaired, the pair arrays are not written
    got = call(g, False, outputs=st.names(True))
    assert all((got[name].view(np.uint8) == PATTERN).all() for name in st.PAIR_OUTPUTS) and got["numProper"] == 0
    # every bad argument: nothing is launched, the outputs keep the pattern
    bad = awfm.AwFmIllegalPositionError
    for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(min_insert=501), dict(min_insert=-(1 << 40) - 1),
               dict(max_insert=(1 << 40) + 1), dict(mapq_cap=255), dict(flags=2), dict(flags=3), dict(num_reads=2999), dict(num_reads=1 << 31)):
        enqueue, collect = call.run(g, True, launch=False, **kw)
        with pytest.raises(awfm.AwFmError) as e:
            enqueue()
        assert e.value.rc == bad, kw
        torch.cuda.synchronize()
        got = collect()
        assert all((np.asarray(got[name]).view(np.uint8) == PATTERN).all() for name in DTYPES), kw
    lib, params = awfm._lib.lib(), awfm.pair_params(**a.params)
    d_slots = torch.full((4 * a.num_reads,), PATTERN, dtype=torch.uint8, device="cuda")
    guarded = awfm.strand_outputs(strandSlots=d_slots.data_ptr())
    pointers = [t.data_ptr() for t in call.arrays]

    def raw(inputs, reads, outputs, settings=params, image=g.handle, flags=1):
        return lib.awfmGpuChooseStrands(image, None if inputs is None else C.byref(inputs), reads, 4, flags, None if settings is None else C.byref(settings),
                                        None if outputs is None else C.byref(outputs), None)

    good = awfm.strand_inputs(*pointers)
    assert raw(None, a.num_reads, guarded) == -4 and raw(good, a.num_reads, None) == -4 and raw(good, a.num_reads, guarded, None) == -4
    assert raw(good, a.num_reads, guarded, image=None) == -4
    for k in range(5):
        missing = awfm.strand_inputs(*[0 if j == k else v for j, v in enumerate(pointers)])
        assert raw(missing, a.num_reads, guarded) == -4, k
    assert raw(good, a.num_reads, guarded, awfm.pair_params(200, 500, mapq_cap=255), flags=0) == bad  # unpaired reads mapqCap
    assert raw(None, 0, None, None) == awfm.AwFmSuccess  # numReads == 0 touches nothing
    torch.cuda.synchronize()
    assert (d_slots.cpu().numpy() == PATTERN).all()  # nothing was launched
    assert raw(good, a.num_reads, guarded, awfm.pair_params(501, 200), flags=0) == awfm.AwFmSuccess  # unpaired does not read the interval
    torch.cuda.synchronize()
    assert np.array_equal(d_slots.cpu().numpy().view(np.uint32), want["strandSlots"])


# ---- orient ---------------------------------------------------------------------------------------------------------------------
class OrientCall:
    """one orient case on the device: inputs `skew_in` bytes and outputs `skew_out` bytes into allocations with guard words"""

    def __init__(self, awfm, torch, case, skew_in=0, skew_out=0, capacity=None, exact=False, num_read_chars=None):
        self.awfm, self.torch, self.case = awfm, torch, case
        R = len(case["strands"])
        o = case["offsets"].astype(np.int64)
        self.R, self.C = R, next(iter(case["columns"].values())).shape[1]
        self.capacity = max(int(o[R] - o[0]), 0) if capacity is None else capacity
        pad = 0 if exact else GUARD
        self.pad, self.skew_out = pad, 0 if exact else skew_out

        def guarded(body, skew):
            return torch.from_numpy(np.concatenate((np.full(pad + skew, PATTERN, np.uint8), body, np.full(pad, PATTERN, np.uint8)))).to("cuda")

        skew_in = 0 if exact else skew_in
        self.chars, self.quals = guarded(case["chars"], skew_in), guarded(case["qualities"], skew_in)
        self.offsets, self.strands = _upload(torch, case["offsets"]), _upload(torch, case["strands"])
        self.columns = {name: _upload(torch, a) for name, a in case["columns"].items()}
        self.out = {name: torch.full((2 * pad + self.skew_out + max(self.capacity, 1 if exact else 0),), PATTERN, dtype=torch.uint8, device="cuda")
                    for name in ("readChars", "qualities")}
        self.out["readOffsets"] = torch.full((2 * GUARD + 8 * (R + 1),), PATTERN, dtype=torch.uint8, device="cuda")
        self.out["numMalformed"] = _upload(torch, np.array([3], np.uint64))
        for name, a in case["columns"].items():
            self.out[name] = torch.full((2 * GUARD + R * self.C * a.dtype.itemsize,), PATTERN, dtype=torch.uint8, device="cuda")
        size = case["chars"].size if num_read_chars is None else num_read_chars
        rows = awfm.verify_inputs(self.chars.data_ptr() + pad + skew_in, size, self.offsets.data_ptr(),
                                  **{n: t.data_ptr() for n, t in self.columns.items() if n in dict(awfm.VERIFY_SLOT_INPUTS)})
        self.inputs = awfm.orient_inputs(rows, self.strands.data_ptr(), self.quals.data_ptr() + pad + skew_in,
                                         **{n: t.data_ptr() for n, t in self.columns.items() if n not in dict(awfm.VERIFY_SLOT_INPUTS)})
        self.outputs = awfm.orient_outputs(self.out["readChars"].data_ptr() + pad + self.skew_out, self.capacity, self.out["readOffsets"].data_ptr() + GUARD,
                                           qualities=self.out["qualities"].data_ptr() + pad + self.skew_out, numMalformed=self.out["numMalformed"].data_ptr(),
                                           **{n: self.out[n].data_ptr() + GUARD for n in case["columns"]})

    def __call__(self, g):
        self.g = g
        g.orient_reads(self.inputs, self.R, self.outputs, max_candidates=self.C)
        self.torch.cuda.synchronize()
        result = {}
        for name in ("readChars", "qualities"):
            raw, lead = self.out[name].cpu().numpy(), self.pad + self.skew_out
            assert (raw[:lead] == PATTERN).all() and (raw[lead + self.capacity:][:self.pad] == PATTERN).all(), f"wrote outside {name}"
            result[name] = raw[lead:lead + self.capacity]
        raw = self.out["readOffsets"].cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all()
        result["readOffsets"] = raw[GUARD:-GUARD].view(np.uint64)
        for name, a in self.case["columns"].items():
            raw = self.out[name].cpu().numpy()
            assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), f"wrote outside {name}"
            result[name] = raw[GUARD:-GUARD].view(a.dtype).reshape(self.R, self.C)
        result["numMalformed"] = int(self.out["numMalformed"].cpu().numpy().view(np.uint64)[0])
        return result


def _host(awfm, case, **kw):
    return awfm.orient_reads_host(case["chars"], case["offsets"], case["strands"], slots=case["columns"], qualities=case["qualities"], fill=PATTERN,
                                  malformed_before=3, threads=16, **kw)


@pytest.mark.parametrize("slots", [1, 16])
def test_orient_every_length_at_every_alignment(awfm, g, slots):
    """the matrix of tests/test_strands.py -- every length at every destination offset mod 4, leads 0 to 3, strands and their
    opposites -- with input and output 0 to 3 bytes into their allocations on top (the lead moves the source, the output's skew
    the destination words)"""
    import torch
    order = st.orient_order()
    seen = set()
    for lead in range(4):
        case = st.orient_case(lead, order, lead=lead, C=slots)
        for flip in (0, 1):
            case["strands"] ^= np.uint8(flip)
            seen |= st.orient_alignments(case, order)
            want = _host(awfm, case)
            for skew_out in ((0, 1, 2, 3) if flip == 0 else ((lead + 1) % 4,)):
                st.assert_orient_equal(OrientCall(awfm, torch, case, skew_in=(lead + skew_out) % 3, skew_out=skew_out)(g), want, what=f"{lead} {flip} {skew_out}")
    assert seen == {(n, s, a, b) for n in st.ORIENT_LENGTHS for s in range(2) for a in range(4) for b in range(4)}


def test_orient_to_the_last_byte_malformed_reads_and_bad_arguments(awfm, g):
    import torch
    # tensors of exactly the buffers' sizes, no guard words: the last reverse row ends at the last byte of the input tensor, the
    # last read at the last byte of the output tensor (the allocator rounds a tensor up, so this is not the end of a device
    # allocation; the kernel loads only aligned dwords that hold a byte of the buffer, whatever lies behind)
    case = st.orient_case(21, [150] * 37 + [149], C=4)
    case["strands"][-1] = 1
    st.assert_orient_equal(OrientCall(awfm, torch, case, exact=True)(g), _host(awfm, case), what="exact")
    case["strands"][-1] = 0
    st.assert_orient_equal(OrientCall(awfm, torch, case, exact=True)(g), _host(awfm, case), what="exact, forward")
    # each kind of malformed read (tests/test_strands.py test_orient_malformed_reads)
    base = st.orient_case(5, [20, 21, 22, 23, 24, 25, 26, 27], lead=2, tail=4)
    R = 8
    for kind in range(7):
        case = {k: (v.copy() if isinstance(v, np.ndarray) else {n: a.copy() for n, a in v.items()}) for k, v in base.items()}
        kw, o = {}, case["offsets"]
        if kind == 0:
            o[3], o[4] = o[4], o[3]
        elif kind == 1:
            o[R + 3], o[R + 4] = o[R + 4], o[R + 3]
        elif kind == 2:
            kw["num_read_chars"] = int(o[2 * R - 1])
        elif kind == 3:
            o[R + 5] += 1
        elif kind == 4:
            case["strands"][[1, 6]] = (2, 255)
        elif kind == 5:
            kw["capacity"] = int(o[R - 1] - o[0]) + 3
        else:
            o[0] = o[1] + 1
        want = _host(awfm, case, **kw)
        assert 3 < want["numMalformed"] < 3 + R, kind
        st.assert_orient_equal(OrientCall(awfm, torch, case, skew_in=1, skew_out=2, **kw)(g), want, what=f"kind {kind}")
    # refusals: nothing is launched
    call = OrientCall(awfm, torch, base)
    lib, bad = awfm._lib.lib(), awfm.AwFmIllegalPositionError

    def raw(inputs, outputs, reads=R, slots=4, image=g.handle):
        return lib.awfmGpuOrientReads(image, None if inputs is None else C.byref(inputs), reads, slots, None if outputs is None else C.byref(outputs), None)

    def changed(struct, **fields):
        copy = type(struct)()
        C.memmove(C.byref(copy), C.byref(struct), C.sizeof(struct))
        for name, value in fields.items():
            target = copy.rows if name.startswith("rows_") else copy
            setattr(target, name[5:] if name.startswith("rows_") else name, value)
        return copy

    assert raw(None, call.outputs) == -4 and raw(call.inputs, None) == -4 and raw(call.inputs, call.outputs, image=None) == -4
    for fields in (dict(rows_readChars=None), dict(rows_readOffsets=None), dict(strands=None), dict(qualities=None), dict(rows_sequences=None),
                   dict(slotTextEnds=None)):
        assert raw(changed(call.inputs, **fields), call.outputs) == -4, fields
    for fields in (dict(readChars=None), dict(readOffsets=None), dict(qualities=None), dict(chainEndDiagonals=None), dict(slotScores=None)):
        assert raw(call.inputs, changed(call.outputs, **fields)) == -4, fields
    assert raw(call.inputs, call.outputs, slots=0) == bad and raw(call.inputs, call.outputs, slots=17) == bad
    assert raw(call.inputs, call.outputs, reads=1 << 31) == bad
    source = call.chars.data_ptr() + GUARD
    assert raw(call.inputs, changed(call.outputs, readChars=source + base["chars"].size - 1)) == bad  # overlap by one byte
    assert raw(call.inputs, changed(call.outputs, qualities=call.quals.data_ptr() + GUARD)) == bad
    assert raw(None, None, reads=0) == awfm.AwFmSuccess  # numReads == 0 touches nothing
    torch.cuda.synchronize()
    for name in ("readChars", "qualities", "readOffsets", "sequences"):
        assert (call.out[name].cpu().numpy() == PATTERN).all(), name
    assert np.array_equal(call.chars.cpu().numpy()[GUARD:-GUARD], base["chars"])


def test_end_to_end_on_a_one_strand_index(awfm, require_gpu, tmp_path):
    """tests/strands_common.py EndToEnd: a FASTA file of three records indexed on ONE strand, 96 FR pairs planted on both strands.
    The loop of the header on the device without a download in between: reverse complement of every read into the second half
    of the buffer, slot scores on the 2R rows, strand choice, window scores on the windows it names (into the free column of the
    one slot table), slot scores, strand choice, orient, affine alignment with strandSlots, strings, SAM records with baseFlags.
    The results meet the condition the host loop meets (tests/test_strands.py), and both strand choices, the oriented batch, the
    alignments and the SAM lines equal the host's byte for byte."""
    import torch
    import verify_chains_common as vc
    e = st.EndToEnd(awfm, tmp_path)
    image = awfm.GpuIndex(e.ix)
    try:
        image.set_text(e.text)
        E, R, C, n = st.E2E, e.R, st.E2E["slots"], st.E2E["length"]
        rows, size, max_ops = 2 * R, e.size, E["max_ops"]
        kept = []

        def buffers(fields):
            out = {name: torch.zeros(max(count * np.dtype(dtype).itemsize, 8), dtype=torch.uint8, device="cuda") for name, (dtype, count) in fields.items()}
            kept.append(out)
            return out

        def home(out, fields):
            torch.cuda.synchronize()
            return {name: out[name].cpu().numpy()[:count * np.dtype(dtype).itemsize].view(dtype) for name, (dtype, count) in fields.items()}

        # the reads as sequenced in the first half of ONE buffer, their reverse complements into the second half
        d_chars = torch.zeros(2 * size, dtype=torch.uint8, device="cuda")
        d_chars[:size] = torch.from_numpy(e.sequenced.copy()).to("cuda")
        d_offsets, d_qualities = _upload(torch, e.offsets), _upload(torch, e.qualities)
        image.reverse_complement_reads(d_chars.data_ptr(), size, d_offsets.data_ptr(), R, d_chars.data_ptr() + size, 0)
        slots = {name: _upload(torch, e.slots[name]) for name in vc.SLOT_FIELDS}  # ONE table: the window call writes into it
        vin = awfm.verify_inputs(d_chars.data_ptr(), 2 * size, d_offsets.data_ptr(), **{name: t.data_ptr() for name, t in slots.items()})
        score_fields = {"slotScores": (np.uint32, rows * C), "slotReadEnds": (np.uint32, rows * C), "slotTextEnds": (np.uint64, rows * C)}
        strand_fields = {name: (dtype, R) for name, dtype in st.READ_OUTPUTS.items()}
        strand_fields.update({name: (dtype, rows) for name, dtype in st.ROW_OUTPUTS.items()})
        strand_fields.update({name: (dtype, R // 2) for name, dtype in st.PAIR_OUTPUTS.items()})
        strand_fields.update({name: (np.uint64, 1) for name in st.COUNTERS})

        def choose():
            scored, out = buffers(score_fields), buffers(strand_fields)
            image.score_chains_affine(vin, rows, awfm.slot_score_outputs(**{name: t.data_ptr() for name, t in scored.items()}), max_candidates=C,
                                      min_score=E["min_score"], mapq_cap=E["mapq_cap"], **st.E2E_COMMON)
            sin = awfm.strand_inputs(d_offsets.data_ptr(), slots["sequences"].data_ptr(), scored["slotScores"].data_ptr(),
                                     scored["slotReadEnds"].data_ptr(), scored["slotTextEnds"].data_ptr())
            image.choose_strands(sin, R, awfm.strand_outputs(**{name: t.data_ptr() for name, t in out.items()}), paired=True, min_insert=E["min_insert"],
                                 max_insert=E["max_insert"], max_candidates=C, min_score=E["min_score"], unpaired_penalty=E["unpaired_penalty"],
                                 window_pad=E["window_pad"], mapq_cap=E["mapq_cap"])
            return scored, out

        _, first = choose()
        win = awfm.window_inputs(d_chars.data_ptr(), 2 * size, d_offsets.data_ptr(), first["windowSequences"].data_ptr(), first["windowBegins"].data_ptr(),
                                 first["windowEnds"].data_ptr())
        scratch = torch.zeros(image.score_windows_affine_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        image.score_windows_affine(win, rows, awfm.window_score_outputs(**{name: t.data_ptr() for name, t in slots.items()}), scratch.data_ptr(), n,
                                   scoring=E["scoring"], min_score=E["min_score"], slot_stride=C, slot_column=C - 1)
        scored, second = choose()
        # orient: the R-row batch
        column_dtypes = dict(st.SLOT_COLUMNS)
        oriented_fields = {"readChars": (np.uint8, size), "qualities": (np.uint8, size), "readOffsets": (np.uint64, R + 1), "numMalformed": (np.uint64, 1)}
        oriented_fields.update({name: (dtype, R * C) for name, dtype in column_dtypes.items()})
        oriented = buffers(oriented_fields)
        oin = awfm.orient_inputs(vin, second["strands"].data_ptr(), d_qualities.data_ptr(), **{name: t.data_ptr() for name, t in scored.items()})
        image.orient_reads(oin, R, awfm.orient_outputs(oriented["readChars"].data_ptr(), size, oriented["readOffsets"].data_ptr(),
                                                       **{name: t.data_ptr() for name, t in oriented.items() if name not in ("readChars", "readOffsets")}),
                           max_candidates=C)
        narrow = awfm.verify_inputs(oriented["readChars"].data_ptr(), size, oriented["readOffsets"].data_ptr(),
                                    **{name: oriented[name].data_ptr() for name in vc.SLOT_FIELDS})
        aligned_fields = {name: (dtype, R) for name, dtype in awfm.AFFINE_READ_OUTPUTS}
        aligned_fields["ops"] = (np.uint32, R * max_ops)
        aligned = buffers(aligned_fields)
        align_scratch = torch.zeros(image.align_chains_affine_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        image.align_chains_affine(narrow, second["strandSlots"].data_ptr(), R, awfm.affine_outputs(**{name: t.data_ptr() for name, t in aligned.items()}),
                                  align_scratch.data_ptr(), max_candidates=C, max_ops=max_ops, max_rows=n, **st.E2E_COMMON)
        capacity = 128 * R
        string_fields = {"cigarOffsets": (np.uint64, R + 1), "cigarChars": (np.uint8, capacity), "mdOffsets": (np.uint64, R + 1), "mdChars": (np.uint8, capacity)}
        strings = buffers(string_fields)
        string_scratch = torch.zeros(image.alignment_strings_scratch_bytes(R), dtype=torch.uint8, device="cuda")
        image.alignment_strings(awfm.string_inputs(oriented["sequences"].data_ptr(), second["strandSlots"].data_ptr(), aligned["textBegins"].data_ptr(),
                                                   aligned["numOps"].data_ptr(), aligned["ops"].data_ptr()),
                                R, awfm.string_outputs(cigarCapacity=capacity, mdCapacity=capacity, **{k: v.data_ptr() for k, v in strings.items()}),
                                string_scratch.data_ptr(), max_candidates=C, max_ops=max_ops, classic=True)
        d_names = [torch.from_numpy(a.copy()).to("cuda") for a in (e.record_names[0].view(np.uint8), e.record_names[1])]
        addresses = e.sam_arrays(oriented, second, aligned, strings)
        addresses.update(recordNameOffsets=d_names[0], recordNameChars=d_names[1])
        line_capacity = 1024 * R
        sam_fields = {"lineOffsets": (np.uint64, R + 1), "lineChars": (np.uint8, line_capacity), "numUnaligned": (np.uint64, 1), "numOverflow": (np.uint64, 1)}
        sam = buffers(sam_fields)
        sam_scratch = torch.zeros(image.sam_records_scratch_bytes(R) + 16, dtype=torch.uint8, device="cuda")
        image.sam_records(awfm.sam_inputs(size, len(e.records), **{name: t.data_ptr() for name, t in addresses.items()}), R,
                          awfm.sam_outputs(lineOffsets=sam["lineOffsets"].data_ptr(), lineChars=sam["lineChars"].data_ptr(), lineCapacity=line_capacity,
                                           numUnaligned=sam["numUnaligned"].data_ptr(), numOverflow=sam["numOverflow"].data_ptr()),
                          (sam_scratch.data_ptr() + 15) & ~15, max_candidates=C, paired=True)
        torch.cuda.synchronize()
        # everything comes home only now
        got = dict(first=home(first, strand_fields), second=home(second, strand_fields), oriented=home(oriented, oriented_fields),
                   aligned=home(aligned, aligned_fields), strings=home(strings, string_fields), sam=home(sam, sam_fields))
        for choice in (got["first"], got["second"]):
            for name in st.COUNTERS:
                choice[name] = int(choice[name][0])
        got["oriented"]["numMalformed"] = int(got["oriented"]["numMalformed"][0])
        for name in ("numUnaligned", "numOverflow"):
            got["sam"][name] = int(got["sam"][name][0])
        total = int(got["sam"]["lineOffsets"][-1])
        got["sam"]["lineChars"] = got["sam"]["lineChars"][:total]
        assert np.array_equal(d_chars.cpu().numpy(), e.chars)  # the reverse complements in the second half
        e.check(got)
        want = e.host_loop(awfm)
        st.assert_equal(got["first"], want["first"], st.names(True), what="first choice")
        st.assert_equal(got["second"], want["second"], st.names(True), what="second choice")
        for name in vc.SLOT_FIELDS:
            assert np.array_equal(slots[name].cpu().numpy().view(vc.SLOT_DTYPES[name]).reshape(rows, C), want["slots"][name]), name
        for name, (dtype, _) in oriented_fields.items():
            if name != "numMalformed":
                assert np.array_equal(got["oriented"][name], np.asarray(want["oriented"][name]).reshape(-1)), name
        for name, _ in awfm.AFFINE_READ_OUTPUTS:
            assert np.array_equal(got["aligned"][name], want["aligned"][name]), name
        assert total == int(want["sam"]["lineOffsets"][-1]) and np.array_equal(got["sam"]["lineOffsets"], want["sam"]["lineOffsets"])
        assert bytes(got["sam"]["lineChars"]) == bytes(want["sam"]["lineChars"][:total])
        assert got["sam"]["numUnaligned"] == want["sam"]["numUnaligned"] == 0 and got["sam"]["numOverflow"] == 0
    finally:
        image.destroy()
        e.close()
