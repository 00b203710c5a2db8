"""awfmGpuReadChains (include/awfm_gpu.h "read chains", csrc/awfm_chains_kernel.h) against its host twin awfmReadChains, which
tests/test_read_chains.py pins to the plain-Python restatement of the definition and to brute force: every output, bit for bit,
on the edge list, the hand-made and the malformed slots and around the tiers' limits by default and with the workgroup tier
forced, on a batch of every size, on the longest recurrence a read can hold, end to end from a FASTA file, and from two streams
at once.  Every output and the scratch lie between guard words."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes before and behind every output, behind the scratch
PATTERN = 0xA5


def _constant(name):
    header = open(os.path.join(ROOT, "avxwindowfmindex_amd", "csrc", "awfm_chains_kernel.h")).read()
    return int(re.search(r"constexpr unsigned " + name + r" = (\d+);", header).group(1))


@pytest.fixture(scope="module")
def image(awfm, require_gpu):
    """the call reads nothing of the index: any small image serves"""
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtacgt" * 8, np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    g = awfm.GpuIndex(ix)
    yield g
    g.destroy()
    ix.dealloc()


def _upload(torch, array):
    """an array of exactly its size on the device (one element for an empty one, which no well-formed read reaches)"""
    if array is None:
        return None
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(8, np.uint8)).to("cuda")


class DeviceCall:
    """the arrays of one case on the device, and guarded outputs and scratch for calls on them"""

    def __init__(self, awfm, torch, case, inputs=None, slots=None):
        self.awfm, self.torch, self.case = awfm, torch, case
        inst = case.inst
        if inputs is None:
            self.arrays = [_upload(torch, a) for a in (inst.offsets, inst.seed_ends, inst.seed_lengths, inst.hit_offsets, inst.positions, inst.sequences)]
            o, ends, lengths, ho, pos, sn = [a.data_ptr() if a is not None else 0 for a in self.arrays]
            inputs = awfm.candidate_inputs(o, inst.num_seeds, ends, lengths, inst.fixed_length, ho, inst.num_hits, pos, sn)
        self.inputs = inputs
        self.slot_arrays = [_upload(torch, a) for a in (case.sequences, case.diagonals, case.spans)] if slots is None else slots

    def run(self, g, outputs=None, stream=0, overflowed_before=0, launch=True, **params):
        """enqueues the call (launch=False: prepares it) -> (launch or None, collect)"""
        torch, n, slots = self.torch, self.case.inst.num_reads, self.case.slots
        outputs = list(ch.FIELDS) if outputs is None else list(outputs)
        sizes = {name: n * slots * np.dtype(ch.DTYPES[name]).itemsize for name in ch.SLOT_FIELDS}
        sizes.update({name: n * 4 for name in ch.READ_FIELDS}, numOverflowed=8)
        buffers = {name: torch.full((sizes[name] + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        if "numOverflowed" in outputs:
            buffers["numOverflowed"][GUARD:GUARD + 8] = torch.from_numpy(np.array([overflowed_before], np.uint64).view(np.uint8)).to("cuda")
        scratch_bytes = self.awfm.read_chains_scratch_bytes(n)
        scratch = torch.full((scratch_bytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        cout = self.awfm.chain_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        d_sequences, d_diagonals, d_spans = [a.data_ptr() for a in self.slot_arrays]
        torch.cuda.synchronize()

        def enqueue():
            g.read_chains(self.inputs, n, d_sequences, d_diagonals, d_spans, cout, scratch.data_ptr(), max_candidates=slots, stream=stream, **params)

        def collect():
            assert (scratch[scratch_bytes:] == PATTERN).all(), "wrote behind the scratch"
            result = {}
            for name, b in buffers.items():
                raw = b.cpu().numpy()
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + sizes[name]:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + sizes[name]]
                if name == "numOverflowed":
                    result[name] = int(body.view(np.uint64)[0])
                else:
                    result[name] = body.view(ch.DTYPES[name]).reshape((n, slots) if name in ch.SLOT_FIELDS else (n,))
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, **kw):
        _, collect = self.run(g, **kw)
        self.torch.cuda.synchronize()
        return collect()


EDGE_PARAMS = [(ch.EDGE_BAND, 4, 64, 0), (ch.EDGE_BAND, 1, 1, 0), (ch.EDGE_BAND, 16, 64, 1), (0, 16, 7, 2), (0xFFFFFFFF, 3, 64, 0),
               (ch.EDGE_BAND, 16, 64, 0xFFFFFFFF), (0xFFFFFFFF, 2, 2, 0xFFFFFFFF)]


@pytest.mark.parametrize("tier", [None, "group"], ids=["default", "group"])
def test_edge_list_and_malformed_reads_equal_the_host_twin(awfm, image, diag, tier):
    import torch
    diag(chains_tier=tier)
    edge = ch.edge_instance()
    for band, slots, lookback, gap_penalty in EDGE_PARAMS:
        case = ch.candidate_case(awfm, edge, band, slots, max_hits_per_seed=ch.EDGE_MAX_HITS)
        params = dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=band, lookback=lookback, gap_penalty=gap_penalty)
        want = case.host(awfm, overflowed_before=3, **params)
        assert want["keptHits"][ch.EDGE_READS["4096 kept hits"]] == 4096 and want["numOverflowed"] == 4
        ch.assert_equal(DeviceCall(awfm, torch, case)(image, overflowed_before=3, **params), want, what=str(params))
    case = ch.candidate_case(awfm, edge, ch.EDGE_BAND, 3, max_hits_per_seed=ch.EDGE_MAX_HITS)
    call = DeviceCall(awfm, torch, case)
    params = dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=ch.EDGE_BAND, gap_penalty=1)
    want = case.host(awfm, **params)
    for missing in ch.FIELDS:  # every output NULL in turn, and alone
        for outputs in ([f for f in ch.FIELDS if f != missing], [missing]):
            got = call(image, outputs=outputs, **params)
            assert sorted(got) == sorted(outputs)
            ch.assert_equal(got, want, names=outputs, what=str(outputs))
    for shape in ("lengths", "fixed", "one-sequence"):
        inst = rc.random_instance(7, with_sequences=shape != "one-sequence", fixed_length=0 if shape == "lengths" else 20)
        case = ch.candidate_case(awfm, inst, 4, 5, max_hits_per_seed=4)
        params = dict(band=4, max_hits_per_seed=4, lookback=3, gap_penalty=1)
        ch.assert_equal(DeviceCall(awfm, torch, case)(image, **params), case.host(awfm, **params), what=shape)
    case = ch.lookback_case()
    for lookback in (64, 63, 1):
        want = case.host(awfm, band=5, lookback=lookback)
        assert int(want["chainScores"][0, 0]) == (25 if lookback == 64 else 20)
        ch.assert_equal(DeviceCall(awfm, torch, case)(image, band=5, lookback=lookback), want, what=f"lookback {lookback}")
    bad = rc.malformed_instance()
    slots = np.tile(np.array([[0, 1]], np.uint32), (bad.num_reads, 1))
    case = ch.Case(bad, slots, np.full(slots.shape, 100), np.full(slots.shape, 300))
    want = case.host(awfm, band=4, overflowed_before=7)
    assert [r for r in range(bad.num_reads) if want["keptHits"][r] == ch.MALFORMED] == list(rc.MALFORMED_READS)
    ch.assert_equal(DeviceCall(awfm, torch, case)(image, band=4, overflowed_before=7), want, what="malformed")  # the counter is added to
    case = ch.intersecting_case()
    want = case.host(awfm, band=20, overflowed_before=1)
    assert [r for r in range(5) if want["keptHits"][r] == ch.MALFORMED] == list(ch.INTERSECTING_READS)
    ch.assert_equal(DeviceCall(awfm, torch, case)(image, band=20, overflowed_before=1), want, what="intersecting slots")


@pytest.mark.parametrize("tier", [None, "group"], ids=["default", "group"])
def test_reads_at_the_tiers_limits(awfm, image, diag, tier):
    """reads of exactly the wave tier's limit and one more, of the workgroup tier's limit and one more, and around the powers of
    two the sort pads to and the 64 anchors a wave loads at a time; every kept hit is an anchor, so the sizes are the tiers' own
    measure; the same batch with the workgroup tier forced (chains_tier=wave is the default)"""
    import torch
    diag(chains_tier=tier)
    wave, group = _constant("kChainsWaveLimit"), _constant("kChainsGroupLimit")
    assert group == ch.MAX_HITS and wave < group
    sizes = [wave, wave + 1, wave - 1, 0, 1, 2, 3, group, group + 1, group - 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 5 * group, 1]
    for loci, params in ((4, dict(band=3, gap_penalty=1)), (1, dict(band=2, lookback=20)), (16, dict(band=0, gap_penalty=0))):
        case = ch.sized_case(sizes, loci=loci, seed=3 + loci)
        want = case.host(awfm, **params)
        assert want["keptHits"].tolist() == sizes and want["numOverflowed"] == 2
        assert want["chainAnchors"].max() > 8
        ch.assert_equal(DeviceCall(awfm, torch, case)(image, **params), want, what=str(params))
    inst = rc.dropped_seeds_instance()  # seeds above maxHitsPerSeed that hold whole rounds of a wave: the gather jumps over them
    case = ch.candidate_case(awfm, inst, 7, 8, max_hits_per_seed=16)
    params = dict(band=7, max_hits_per_seed=16, gap_penalty=1)
    ch.assert_equal(DeviceCall(awfm, torch, case)(image, **params), case.host(awfm, **params), what="dropped seeds")


def test_batch_of_every_size_goes_through_the_worklist(awfm, image):
    """every number of kept hits from 0 to 4097 once (2^12 + 2 reads), in random order: the worklist, its length read on the
    device, both grids trimmed"""
    import torch
    rng = np.random.default_rng(12)
    sizes = rng.permutation(ch.MAX_HITS + 2)
    case = ch.sized_case(sizes, loci=5, slots=6, seed=8)
    params = dict(band=3, gap_penalty=1, lookback=32)
    want = case.host(awfm, threads=16, **params)
    assert np.array_equal(want["keptHits"], sizes) and want["numOverflowed"] == 1
    assert (want["bestSlots"] == ch.NO_SLOT).sum() == 2 and want["chainAnchors"].max() > 30
    ch.assert_equal(DeviceCall(awfm, torch, case)(image, **params), want)


def test_the_longest_recurrence_and_the_widest_spread(awfm, image):
    """4096 hits in ONE slot: 4096 sequential steps of one wave, the most a read can ask for (microseconds per step would still
    be milliseconds: the suite's time limit is not near); and 4096 hits spread evenly over 16 slots, two per wave"""
    import torch
    for loci, slots in ((1, 1), (16, 16), (1, 16)):
        case = ch.sized_case([ch.MAX_HITS, 7, ch.MAX_HITS], loci=loci, slots=slots, seed=40 + loci, span=6)
        for params in (dict(band=6, gap_penalty=1), dict(band=2, gap_penalty=0, lookback=1)):
            want = case.host(awfm, **params)
            assert want["keptHits"].tolist() == [ch.MAX_HITS, 7, ch.MAX_HITS]
            assert "lookback" in params or want["chainAnchors"].max() > 100  # (lookback 1 sees the hit before, often of the same seed)
            ch.assert_equal(DeviceCall(awfm, torch, case)(image, **params), want, what=f"{loci} loci {params}")


def test_two_streams_on_one_image_at_once(awfm, image):
    import torch
    a, b = ch.sized_case([300, 5, 4000, 0, 256, 257] * 40, loci=3, seed=5), ch.candidate_case(awfm, rc.random_instance(9, reads=400), 3, 2)
    calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
    params = [dict(band=3, gap_penalty=1), dict(band=3, lookback=4)]
    want = [a.host(awfm, **params[0]), b.host(awfm, **params[1])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = [call.run(image, stream=s.cuda_stream, launch=False, **p) for _ in range(3) for call, p, s in zip(calls, params, streams)]
    for enqueue, _ in pending:  # interleaved, nothing waited for in between: each call has its own scratch and outputs
        enqueue()
    torch.cuda.synchronize()
    for k, (_, collect) in enumerate(pending):
        ch.assert_equal(collect(), want[k % 2], what=f"call {k}")


def test_error_codes_and_an_empty_batch(awfm, image):
    import torch
    case = ch.candidate_case(awfm, rc.random_instance(5, reads=4), 3, 4)
    call = DeviceCall(awfm, torch, case)
    scratch = torch.zeros(awfm.read_chains_scratch_bytes(4), dtype=torch.uint8, device="cuda")
    assert awfm.read_chains_scratch_bytes(1 << 20) <= 16 + 4 * (1 << 20) + 16
    out = awfm.chain_outputs()
    d_slots = [a.data_ptr() for a in call.slot_arrays]
    image.read_chains(call.inputs, 0, 0, 0, 0, out, 0)  # no reads: succeeds, touches nothing
    image.read_chains(call.inputs, 4, *d_slots, out, scratch.data_ptr(), band=3)  # every output NULL
    for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(lookback=0), dict(lookback=65)):
        with pytest.raises(awfm.AwFmError) as err:
            image.read_chains(call.inputs, 4, *d_slots, out, scratch.data_ptr(), **kw)
        assert err.value.rc == awfm.AwFmIllegalPositionError
    with pytest.raises(awfm.AwFmError) as err:
        image.read_chains(call.inputs, 1 << 32, *d_slots, out, scratch.data_ptr())
    assert err.value.rc == awfm.AwFmIllegalPositionError
    for k in range(4):  # a missing slot array, no scratch
        arrays = [0 if i == k else a for i, a in enumerate(d_slots + [scratch.data_ptr()])]
        with pytest.raises(awfm.AwFmError) as err:
            image.read_chains(call.inputs, 4, arrays[0], arrays[1], arrays[2], out, arrays[3])
        assert err.value.rc == -4
    inst = case.inst
    broken = awfm.candidate_inputs(call.arrays[0].data_ptr(), inst.num_seeds, call.arrays[1].data_ptr(), 0, 0, call.arrays[3].data_ptr(),
                                   inst.num_hits, call.arrays[4].data_ptr(), 0)
    with pytest.raises(awfm.AwFmError) as err:  # neither lengths nor a fixed length
        image.read_chains(broken, 4, *d_slots, out, scratch.data_ptr())
    assert err.value.rc == -4
    torch.cuda.synchronize()


def test_end_to_end_on_the_device_equals_the_host_and_chains_every_planted_read(awfm, require_gpu, tmp_path, wide):
    """reads -> awfmGpuLongestSuffixMatches -> hit offsets -> locate -> awfmGpuLocalPositions -> awfmGpuReadCandidates ->
    awfmGpuReadChains with the candidate call's slot arrays passed straight in, on one stream; equal to the host's pipeline and
    twins"""
    import torch
    lengths = lp.record_lengths(43, count=200, longest=1500)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    assert g.is_wide == wide
    reads, planted = rc.planted_reads(records)
    host = rc.host_pipeline(awfm, ix, reads)
    chars, starts, ends, offsets, seed_ends = rc.windows_of(reads)
    n, num_reads, slots = len(starts), len(reads), 4
    stream_obj = torch.cuda.Stream()
    s = stream_obj.cuda_stream
    d_chars, d_starts, d_ends, d_offsets, d_seed_ends = [_upload(torch, a) for a in (chars, starts, ends, offsets, seed_ends)]
    d_lengths = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ranges = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    d_hit_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_scan = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g.longest_suffix_matches(d_chars.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, n, rc.E2E_MIN_LENGTH, d_lengths.data_ptr(),
                             d_ranges.data_ptr(), d_counts.data_ptr(), s)
    total = g.hit_offsets_from_counts(d_counts.data_ptr(), n, d_hit_offsets.data_ptr(), d_scan.data_ptr(), s)
    assert total == host.num_hits
    d_positions = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_sequences = torch.zeros(total, dtype=torch.int32, device="cuda")
    d_slot_sequences = torch.zeros(num_reads * slots, dtype=torch.int32, device="cuda")
    d_slot_diagonals = torch.zeros(num_reads * slots, dtype=torch.int64, device="cuda")
    d_slot_spans = torch.zeros(num_reads * slots, dtype=torch.int32, device="cuda")
    d_candidates_scratch = torch.zeros(awfm.read_candidates_scratch_bytes(num_reads), dtype=torch.uint8, device="cuda")
    stream_obj.wait_stream(torch.cuda.current_stream())
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), n, total, d_positions.data_ptr(), s)
    g.local_positions(d_positions.data_ptr(), total, d_sequences.data_ptr(), d_positions.data_ptr(), stream=s)
    inputs = awfm.candidate_inputs(d_offsets.data_ptr(), n, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), total,
                                   d_positions.data_ptr(), d_sequences.data_ptr())
    cand = awfm.candidate_outputs(sequences=d_slot_sequences.data_ptr(), diagonals=d_slot_diagonals.data_ptr(), diagonalSpans=d_slot_spans.data_ptr())
    g.read_candidates(inputs, num_reads, cand, d_candidates_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=2, min_votes=2,
                      max_candidates=slots, stream=s)
    case = ch.candidate_case(awfm, host, 2, slots, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=2)
    call = DeviceCall(awfm, torch, case, inputs=inputs, slots=[d_slot_sequences, d_slot_diagonals, d_slot_spans])
    params = dict(max_hits_per_seed=rc.E2E_MAX_HITS, band=2, gap_penalty=1)
    _, collect = call.run(g, stream=s, **params)
    stream_obj.synchronize()
    got = collect()
    assert np.array_equal(d_slot_sequences.cpu().numpy().view(np.uint32).reshape(num_reads, slots), case.sequences)
    ch.assert_equal(got, case.host(awfm, **params))
    ch.assert_planted_reads_chained(got, case, planted, rc.E2E_CAP)
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
