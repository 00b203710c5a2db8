"""awfmGpuSamRecords (include/awfm_gpu.h "SAM records", csrc/awfm_sam_kernel.h) against its host twin awfmSamRecords, which
tests/test_sam_records.py pins to the plain-Python restatement of the definition and to lines written out by hand -- and against
that restatement itself, so that the twin is not the only witness: lineOffsets, lineChars and both counters, byte for byte, on the
hand-made batches with every optional array NULL in turn, paired and unpaired, at the natural tier and with sam_tier=direct, on
0 to 200 reads of lengths 0 to 151, beside one read of 20000 characters, with line starts at every residue mod 4 and the arena
itself at every skew, at capacities that cut the output, from two streams at once, with bad arguments, and end to end behind the
device pipeline of tests/test_gpu_pair_mates.py.  Inputs, outputs and the scratch (exactly its declared size) lie between guard
words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_records_common as sm  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5


def _guarded(torch, array):
    """the array's bytes on the device between guard words -> (buffer, address)"""
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    host = np.concatenate((np.full(GUARD, PATTERN, np.uint8), raw, np.full(GUARD, PATTERN, np.uint8)))
    buffer = torch.from_numpy(host).to("cuda")
    return buffer, buffer.data_ptr() + GUARD


@pytest.fixture(scope="module")
def g(awfm, require_gpu):
    """the call takes the image for its device only: any image does"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtacgtacgtacgtacgtacgt", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    image = awfm.GpuIndex(ix)
    yield image
    image.destroy()
    ix.dealloc()


class Scratch:
    """exactly awfmGpuSamRecordsScratchBytes bytes between guard words"""

    def __init__(self, torch, g, num_reads):
        self.size = g.sam_records_scratch_bytes(num_reads)
        assert self.size > 4 * num_reads
        self.buffer = torch.full((self.size + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.address = self.buffer.data_ptr() + GUARD
        assert self.address % 16 == 0

    def check(self):
        raw = self.buffer.cpu().numpy()
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.size:] == PATTERN).all(), "wrote outside the scratch"


class DeviceCall:
    """the arrays of one batch on the device between guard words, and guarded outputs for calls on them"""

    def __init__(self, awfm, torch, batch):
        self.awfm, self.torch, self.batch = awfm, torch, batch
        held = {name: a for name, a in batch.arrays.items() if a is not None}
        self.buffers = {name: _guarded(torch, a) for name, a in held.items()}
        self.inputs = awfm.sam_inputs(held["readChars"].size, held["recordNameOffsets"].size - 1, **{name: b[1] for name, b in self.buffers.items()})

    def run(self, g, scratch, capacity, outputs=None, skew=0, stream=0, unaligned_before=0, overflow_before=0, launch=True):
        torch, n = self.torch, self.batch.n
        outputs = list(sm.NAMES) if outputs is None else list(outputs)
        sizes = dict(lineOffsets=8 * (n + 1), lineChars=capacity, numUnaligned=8, numOverflow=8)
        buffers = {name: torch.full((sizes[name] + 2 * GUARD + 4,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        at = {name: GUARD + (skew if name == "lineChars" else 0) for name in outputs}
        for name, before in (("numUnaligned", unaligned_before), ("numOverflow", overflow_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        sout = self.awfm.sam_outputs(lineCapacity=capacity, **{name: b.data_ptr() + at[name] for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.sam_records(self.inputs, n, sout, scratch.address, max_candidates=self.batch.C, paired=self.batch.paired, stream=stream)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), sizes[name]
                assert (raw[:at[name]] == PATTERN).all() and (raw[at[name] + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[at[name]:at[name] + size].copy()
                result[name] = int(body.view(np.uint64)[0]) if name.startswith("num") else body.view(np.uint64) if name.endswith("Offsets") else body
            for name, (buffer, address) in self.buffers.items():
                raw = buffer.cpu().numpy()
                assert (raw[:GUARD] == PATTERN).all() and (raw[-GUARD:] == PATTERN).all(), f"wrote beside the input {name}"
            scratch.check()
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, *args, **kwargs):
        _, collect = self.run(*args, **kwargs)
        self.torch.cuda.synchronize()
        return collect()


def check(awfm, torch, g, batch, what="", capacity=None, want=None, **arguments):
    """one device call against the twin and the restatement, every output -> the device's result"""
    names = arguments.get("outputs")
    before = dict(unaligned_before=arguments.get("unaligned_before", 0), overflow_before=arguments.get("overflow_before", 0))
    full = sm.expected(batch) if want is None else want
    capacity = int(full["lineOffsets"][-1]) if capacity is None else capacity
    arena = names is None or "lineChars" in names
    restated = sm.expected(batch, capacity, arena=arena, fill=PATTERN, **before)
    twin = awfm.sam_records_host(batch.arrays, max_candidates=batch.C, paired=batch.paired, fill=PATTERN, line_capacity=capacity, outputs=names, **before)
    got = DeviceCall(awfm, torch, batch)(g, Scratch(torch, g, batch.n), capacity, **arguments)
    compare = sm.NAMES if names is None else names
    assert sorted(got) == sorted(compare)
    sm.assert_same(got, twin, names=compare, what=(what, "twin"))
    sm.assert_same(got, restated, names=compare, what=(what, "restatement"))
    return got


@pytest.mark.parametrize("tier", [None, "direct"], ids=["natural", "direct"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_hand_made_batches_equal_the_host_twin_and_the_restatement(awfm, g, diag, tier, paired):
    import torch
    diag(sam_tier=tier)
    for without in [()] + [(w,) for w in sm.OPTIONAL] + [sm.OPTIONAL]:
        batch = sm.hand_batch(paired, without)
        got = check(awfm, torch, g, batch, what=("hand", paired, without), unaligned_before=5, overflow_before=2)
        assert got["numOverflow"] == 2 and got["numUnaligned"] > 5 + sm.UNALIGNED_COUNT
    unaligned = sm.Batch(sm.unaligned_reads(), paired=paired, inverted=sm.UNALIGNED_INVERTED)
    assert check(awfm, torch, g, unaligned, what="unaligned")["numUnaligned"] == sm.UNALIGNED_COUNT


@pytest.mark.parametrize("tier", [None, "direct"], ids=["natural", "direct"])
def test_read_counts_read_lengths_skews_and_capacities(awfm, g, diag, tier):
    import torch
    diag(sam_tier=tier)
    base = sm.mixed_batch(11, 200)
    offsets = sm.expected(base)["lineOffsets"]
    assert {int(v) % 4 for v in offsets[:-1]} == {0, 1, 2, 3}  # line starts at every residue mod 4
    lengths = {int(b) - int(a) for a, b in zip(base.arrays["readOffsets"][:-1], base.arrays["readOffsets"][1:])}
    assert lengths == {0, 1, 3, 4, 5, 150, 151}
    for n in (1, 2, 63, 64, 65, 200):
        check(awfm, torch, g, base.cut(n), what=("reads", n))
    for n in (2, 64, 200):
        check(awfm, torch, g, sm.mixed_batch(12 + n, n, paired=True), what=("pairs", n))
    for skew in (1, 2, 3):  # the arena itself off a dword boundary
        check(awfm, torch, g, base, what=("skew", skew), skew=skew)
    total = int(offsets[-1])
    for capacity in (total - 1, (int(offsets[100]) + int(offsets[101])) // 2, int(offsets[100]), 0):
        got = check(awfm, torch, g, base, what=("capacity", capacity), capacity=capacity, overflow_before=3, skew=capacity % 4)
        assert got["numOverflow"] == 3 + sum(int(v) > capacity for v in offsets[1:])
    for names in (("lineOffsets",), ("lineOffsets", "numOverflow"), ("numUnaligned",), ("lineOffsets", "lineChars")):
        check(awfm, torch, g, base, what=names, outputs=names)
    # no reads: nothing is touched, not even with a scratch of nothing
    call = DeviceCall(awfm, torch, base)
    call.batch = base.cut(0)
    got = call(g, Scratch(torch, g, 1), 32, unaligned_before=3, overflow_before=4)
    assert (got["lineOffsets"].view(np.uint8) == PATTERN).all() and (got["lineChars"] == PATTERN).all() and got["numUnaligned"] == 3 and got["numOverflow"] == 4


@pytest.mark.parametrize("tier", [None, "direct"], ids=["natural", "direct"])
def test_a_read_of_20000_characters_and_lines_around_the_tile(awfm, g, diag, tier):
    import torch
    diag(sam_tier=tier)
    check(awfm, torch, g, sm.mixed_batch(21, 9, long_read=(4, 20000)), what="long")
    check(awfm, torch, g, sm.mixed_batch(22, 8, paired=True, long_read=(3, 20000), without=("qualities",)), what="long, paired")
    # lines of every length from a little below the tile (kSamTileBytes = 2048) to a little above, at every skew
    reads = [sm.read(b"A" * length, name=b"t", md=b"") for length in range(1000, 1016)]
    batch = sm.Batch(reads, without=("secondScores",))
    lengths = np.diff(sm.expected(batch)["lineOffsets"].astype(np.int64))
    assert lengths.min() < 2048 - 3 and lengths.max() > 2048 + 3
    for skew in range(4):
        check(awfm, torch, g, batch, what=("tile", skew), skew=skew)


def test_bad_arguments_and_two_streams_with_a_scratch_each(awfm, g):
    import torch
    first, second = sm.mixed_batch(31, 200, paired=True), sm.hand_batch(False)
    scratch = Scratch(torch, g, 200)
    call = DeviceCall(awfm, torch, first)
    null, illegal = -4, awfm.AwFmIllegalPositionError
    out = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")
    sout = awfm.sam_outputs(lineOffsets=out.data_ptr(), lineChars=out.data_ptr() + 8 * 256, lineCapacity=(1 << 17) - 8 * 256)

    def refused(rc, **arguments):
        with pytest.raises(awfm.AwFmError) as error:
            g.sam_records(arguments.pop("inputs", call.inputs), arguments.pop("n", 200), arguments.pop("outputs", sout),
                          arguments.pop("scratch", scratch.address), **arguments)
        assert error.value.rc == rc, (error.value.rc, rc)

    refused(null, inputs=None)
    refused(null, outputs=None)
    refused(null, scratch=0)
    for name in ("readChars", "readOffsets", "sequences", "slots", "scores", "editDistances", "textBegins", "textEnds", "cigarOffsets", "cigarChars",
                 "recordNameOffsets", "recordNameChars", "nameOffsets", "nameChars", "mdOffsets", "mdChars"):
        lacking = awfm.sam_inputs(1, len(sm.RECORD_NAMES), **{k: b[1] for k, b in call.buffers.items() if k != name})
        refused(null, inputs=lacking, max_candidates=3)
    refused(null, outputs=awfm.sam_outputs(lineChars=out.data_ptr(), lineCapacity=64), max_candidates=3)
    refused(illegal, max_candidates=0)
    refused(illegal, max_candidates=17)
    refused(illegal, max_candidates=3, flags=2)
    refused(illegal, max_candidates=3, n=199, paired=True)
    refused(illegal, max_candidates=3, n=1 << 32)
    refused(illegal, max_candidates=3, scratch=scratch.address + 8)
    assert g.sam_records_scratch_bytes(0) == 0 and g.sam_records_scratch_bytes(1 << 32) == 0
    torch.cuda.synchronize()
    scratch.check()
    # two streams at once, each with its own scratch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    runs = []
    for batch, stream in ((first, streams[0]), (second, streams[1])):
        want = sm.expected(batch, fill=PATTERN)
        enqueue, collect = DeviceCall(awfm, torch, batch).run(g, Scratch(torch, g, batch.n), int(want["lineOffsets"][-1]), stream=stream.cuda_stream, launch=False)
        runs.append((enqueue, collect, want))
    for _ in range(3):
        for enqueue, _, _ in runs:
            enqueue()
    torch.cuda.synchronize()
    for _, collect, want in runs:
        got = collect()
        sm.assert_same(got, want, names=("lineOffsets", "lineChars"), what="streams")
        assert got["numUnaligned"] == 3 * want["numUnaligned"] and got["numOverflow"] == 0  # the counters are added to
    for stream in streams:
        g.stream_retire(stream.cuda_stream)


def test_end_to_end_through_the_device_pipeline(awfm, require_gpu, tmp_path):
    """tests/pair_mates_common.py EndToEnd behind tests/test_gpu_pair_mates.py DeviceSide: the loop of the pairing header, then
    affine alignment with its scripts kept on the device, the classic strings, and the records -- every array passed on as it
    lies on the device.  The arena equals the host twin's on the downloaded arrays byte for byte, and every line passes the parser of
    tests/sam_records_common.py."""
    import torch
    import pair_mates_common as pm
    from test_gpu_pair_mates import DeviceSide
    e = pm.EndToEnd(awfm, tmp_path)
    image = awfm.GpuIndex(e.ix)
    try:
        image.set_text(e.text)
        n, C, max_ops = e.offsets.size - 1, pm.E2E["slots"], pm.E2E["max_ops"]
        fields = {name: (dtype, n) for name, dtype in awfm.AFFINE_READ_OUTPUTS}
        fields["ops"] = (np.uint32, n * max_ops)

        class ScriptsKept(DeviceSide):
            """the loop's device side, its last call with the scripts among the outputs and everything left on the device"""

            def align(self, slots, chosen):
                out = self.buffers(fields)
                scratch = torch.zeros(image.align_chains_affine_scratch_bytes(pm.E2E["length"]), dtype=torch.uint8, device="cuda")
                self.kept.append(scratch)
                image.align_chains_affine(self.vin, chosen.data_ptr(), n, awfm.affine_outputs(**{name: t.data_ptr() for name, t in out.items()}),
                                          scratch.data_ptr(), max_candidates=C, max_ops=max_ops, max_rows=pm.E2E["length"], **self.common)
                return out

        side = ScriptsKept(awfm, torch, image, e)
        _, second, aligned = e.loop(side)
        score_fields = {"secondScores": (np.uint32, n)}
        scored = side.buffers(score_fields)
        image.score_chains_affine(side.vin, n, awfm.slot_score_outputs(secondScores=scored["secondScores"].data_ptr()), max_candidates=C,
                                  min_score=pm.E2E["min_score"], mapq_cap=pm.E2E["mapq_cap"], **side.common)
        capacity = 128 * n
        strings = {name: torch.zeros(size, dtype=torch.uint8, device="cuda")
                   for name, size in (("cigarOffsets", 8 * (n + 1)), ("cigarChars", capacity), ("mdOffsets", 8 * (n + 1)), ("mdChars", capacity))}
        string_scratch = torch.zeros(image.alignment_strings_scratch_bytes(n), dtype=torch.uint8, device="cuda")
        sin = awfm.string_inputs(side.slots["sequences"].data_ptr(), second["pairSlots"].data_ptr(), aligned["textBegins"].data_ptr(),
                                 aligned["numOps"].data_ptr(), aligned["ops"].data_ptr())
        image.alignment_strings(sin, n, awfm.string_outputs(cigarCapacity=capacity, mdCapacity=capacity, **{k: v.data_ptr() for k, v in strings.items()}),
                                string_scratch.data_ptr(), max_candidates=C, max_ops=max_ops, classic=True)
        name_offsets, name_chars = awfm.record_names(e.ix)
        d_names = [torch.from_numpy(a.copy()).to("cuda") for a in (name_offsets.view(np.uint8), name_chars)]
        addresses = dict(readChars=side.chars, readOffsets=side.offsets, recordNameOffsets=d_names[0], recordNameChars=d_names[1],
                         sequences=side.slots["sequences"], slots=second["pairSlots"], scores=aligned["scores"], editDistances=aligned["editDistances"],
                         textBegins=aligned["textBegins"], textEnds=aligned["textEnds"], cigarOffsets=strings["cigarOffsets"],
                         cigarChars=strings["cigarChars"], mdOffsets=strings["mdOffsets"], mdChars=strings["mdChars"],
                         mappingQualities=second["mappingQualities"], secondScores=scored["secondScores"], properPairs=second["properPairs"])
        sam_in = awfm.sam_inputs(e.sequenced.size, len(e.records), **{name: t.data_ptr() for name, t in addresses.items()})
        line_capacity = 1024 * n
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_lines = torch.full((line_capacity,), PATTERN, dtype=torch.uint8, device="cuda")
        d_counters = torch.zeros(2, dtype=torch.int64, device="cuda")
        scratch = Scratch(torch, image, n)
        image.sam_records(sam_in, n, awfm.sam_outputs(lineOffsets=d_offsets.data_ptr(), lineChars=d_lines.data_ptr(), lineCapacity=line_capacity,
                                                      numUnaligned=d_counters.data_ptr(), numOverflow=d_counters.data_ptr() + 8),
                          scratch.address, max_candidates=C, paired=True)
        torch.cuda.synchronize()
        scratch.check()
        offsets, lines = d_offsets.cpu().numpy().view(np.uint64), d_lines.cpu().numpy()
        assert [int(v) for v in d_counters.cpu().numpy()] == [0, 0]
        dtypes = {name: dtype for name, dtype, _ in awfm.SAM_INPUTS}
        arrays = {name: t.cpu().numpy().view(dtypes[name]) for name, t in addresses.items()}
        arrays["sequences"] = arrays["sequences"].reshape(n, C)
        twin = awfm.sam_records_host(arrays, paired=True, line_capacity=line_capacity, fill=PATTERN, threads=16)
        sm.assert_same(dict(lineOffsets=offsets, lineChars=lines, numUnaligned=0, numOverflow=0), twin, what="end to end")
        home = {name: aligned[name].cpu().numpy().view(fields[name][0]) for name in ("scores", "textBegins", "textEnds")}
        sm.check_end_to_end(e, awfm.strings_of(offsets, lines), home, awfm.sam_header(e.ix))
    finally:
        image.destroy()
        e.close()
