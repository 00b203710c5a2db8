"""awfmGpuReadCandidates (include/awfm_gpu.h "candidate loci", csrc/awfm_candidates_kernel.h) against its host twin
awfmReadCandidates, which tests/test_read_candidates.py pins to the NumPy restatement of the definition: every output, bit for
bit, on the edge list and around the tiers' limits by default and with the workgroup tier forced, on a batch of 2^14 reads of every size, end to end
from a FASTA file, and from two streams at once.  Every output and the scratch lie between guard words."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64  # bytes before and behind every output, behind the scratch
PATTERN = 0xA5


def _constant(name):
    header = open(os.path.join(ROOT, "avxwindowfmindex_amd", "csrc", "awfm_candidates_kernel.h")).read()
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
    raw = np.ascontiguousarray(array).view(np.uint8)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(8, np.uint8)).to("cuda")


class DeviceCall:
    """the arrays of one instance on the device, and guarded outputs and scratch for calls on them"""

    def __init__(self, awfm, torch, inst):
        self.awfm, self.torch, self.inst = awfm, torch, inst
        self.arrays = [_upload(torch, a) for a in (inst.offsets, inst.seed_ends, inst.seed_lengths, inst.hit_offsets, inst.positions, inst.sequences)]
        o, ends, lengths, ho, pos, sn = [a.data_ptr() if a is not None else 0 for a in self.arrays]
        self.inputs = awfm.candidate_inputs(o, inst.num_seeds, ends, lengths, inst.fixed_length, ho, inst.num_hits, pos, sn)

    def run(self, g, outputs=None, stream=0, overflowed_before=0, max_candidates=4, launch=True, **params):
        """enqueues the call (launch=False: prepares it) -> (launch or None, collect)"""
        torch, n = self.torch, self.inst.num_reads
        outputs = list(rc.FIELDS) if outputs is None else list(outputs)
        sizes = {name: n * max_candidates * np.dtype(rc.DTYPES[name]).itemsize for name in rc.SLOT_FIELDS}
        sizes.update({name: n * 4 for name in rc.READ_FIELDS}, numOverflowed=8)
        buffers = {name: torch.full((sizes[name] + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        if "numOverflowed" in outputs:
            buffers["numOverflowed"][GUARD:GUARD + 8] = torch.from_numpy(np.array([overflowed_before], np.uint64).view(np.uint8)).to("cuda")
        scratch_bytes = self.awfm.read_candidates_scratch_bytes(n)
        scratch = torch.full((scratch_bytes + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        cout = self.awfm.candidate_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.read_candidates(self.inputs, n, cout, scratch.data_ptr(), max_candidates=max_candidates, stream=stream, **params)

        def collect():
            return self._collect(buffers, scratch, scratch_bytes, sizes, n, max_candidates)

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def _collect(self, buffers, scratch, scratch_bytes, sizes, n, slots):
        """after the stream was waited for: the outputs as the host call returns them, the guards checked"""
        assert (scratch[scratch_bytes:] == PATTERN).all(), "wrote behind the scratch"
        result = {}
        for name, b in buffers.items():
            raw = b.cpu().numpy()
            assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + sizes[name]:] == PATTERN).all(), f"wrote outside {name}"
            body = raw[GUARD:GUARD + sizes[name]]
            if name == "numOverflowed":
                result[name] = int(body.view(np.uint64)[0])
            else:
                result[name] = body.view(rc.DTYPES[name]).reshape((n, slots) if name in rc.SLOT_FIELDS else (n,))
        return result

    def __call__(self, g, **kw):
        _, collect = self.run(g, **kw)
        self.torch.cuda.synchronize()
        return collect()


NULL_COMBINATIONS = [["numCandidates"], ["sequences", "diagonals", "votes", "diagonalSpans", "numOverflowed"], ["readBegins"], ["readEnds", "keptHits"],
                     [f for f in rc.FIELDS if f != "numOverflowed"]]


@pytest.mark.parametrize("tier", [None, "group"], ids=["default", "group"])
def test_edge_list_and_malformed_reads_equal_the_host_twin(awfm, image, diag, tier):
    import torch
    diag(candidates_tier=tier)
    edge = rc.edge_instance()
    call = DeviceCall(awfm, torch, edge)
    for band, min_votes, slots in [(rc.EDGE_BAND, 1, 4), (rc.EDGE_BAND, 0, 1), (rc.EDGE_BAND, 2, 16), (0, 1, 16), (0xFFFFFFFF, 1, 3), (rc.EDGE_BAND, 5000, 4)]:
        params = dict(max_hits_per_seed=rc.EDGE_MAX_HITS, band=band, min_votes=min_votes, max_candidates=slots)
        want = edge.host(awfm, **params)
        assert want["keptHits"][rc.EDGE_READS["4096 kept hits"]] == 4096 and want["numOverflowed"] == 1
        rc.assert_equal(call(image, **params), want, what=str(params))
    params = dict(max_hits_per_seed=rc.EDGE_MAX_HITS, band=rc.EDGE_BAND, max_candidates=3)
    want = edge.host(awfm, **params)
    for outputs in NULL_COMBINATIONS:  # every output may be NULL; without readBegins and readEnds the second pass is skipped
        got = call(image, outputs=outputs, **params)
        assert sorted(got) == sorted(outputs)
        rc.assert_equal(got, want, names=outputs, what=str(outputs))
    for shape in ("fixed", "one-sequence"):
        inst = rc.random_instance(7, with_sequences=shape != "one-sequence", fixed_length=20)
        params = dict(band=4, min_votes=2, max_candidates=5, max_hits_per_seed=4)
        rc.assert_equal(DeviceCall(awfm, torch, inst)(image, **params), inst.host(awfm, **params), what=shape)
    bad = rc.malformed_instance()
    want = bad.host(awfm, band=4, overflowed_before=7)
    assert [r for r in range(bad.num_reads) if want["keptHits"][r] == rc.MALFORMED] == list(rc.MALFORMED_READS)
    rc.assert_equal(DeviceCall(awfm, torch, bad)(image, band=4, overflowed_before=7), want, what="malformed")  # the counter is added to


@pytest.mark.parametrize("tier", [None, "group"], ids=["default", "group"])
def test_reads_at_the_tiers_limits(awfm, image, diag, tier):
    """reads of exactly the wave tier's limit and one more, of the workgroup tier's limit and one more, and around the powers of
    two the sort pads to; the same batch with the workgroup tier forced (candidates_tier=wave is the default)"""
    import torch
    diag(candidates_tier=tier)
    wave, group = _constant("kCandidatesWaveLimit"), _constant("kCandidatesGroupLimit")
    assert group == rc.MAX_HITS and wave < group
    sizes = [wave, wave + 1, wave - 1, 0, 1, 2, 3, group, group + 1, group - 1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, wave, 5 * group, 1]
    inst = rc.sized_instance(sizes, seed=3)
    call = DeviceCall(awfm, torch, inst)
    for params in (dict(band=7, max_candidates=16), dict(band=0, min_votes=2, max_candidates=4), dict(band=1 << 30, max_candidates=1, max_hits_per_seed=7)):
        want = inst.host(awfm, **params)
        if not params.get("max_hits_per_seed"):
            assert want["keptHits"].tolist() == sizes and want["numOverflowed"] == 2
        rc.assert_equal(call(image, **params), want, what=str(params))
    inst = rc.dropped_seeds_instance()  # seeds above maxHitsPerSeed that hold whole rounds of a wave: the gather jumps over them
    params = dict(band=7, max_candidates=8, max_hits_per_seed=16)
    rc.assert_equal(DeviceCall(awfm, torch, inst)(image, **params), inst.host(awfm, **params), what="dropped seeds")


def test_batch_of_every_size_goes_through_the_worklist(awfm, image):
    """2^14 reads: every number of kept hits from 0 to 4097 once, the rest small, in random order -- the worklist, its length
    read on the device, both grids trimmed"""
    import torch
    rng = np.random.default_rng(14)
    sizes = np.concatenate([np.arange(rc.MAX_HITS + 2), rng.integers(0, 300, (1 << 14) - rc.MAX_HITS - 2)])
    sizes = sizes[rng.permutation(len(sizes))]
    inst = rc.sized_instance(sizes, seed=8)
    params = dict(band=7, min_votes=2, max_candidates=8)
    want = inst.host(awfm, threads=16, **params)
    assert np.array_equal(want["keptHits"], np.where(sizes > rc.MAX_HITS, rc.MAX_HITS + 1, sizes)) and want["numOverflowed"] == 1
    assert (want["numCandidates"] > 8).any() and (want["numCandidates"] == 0).any()
    rc.assert_equal(DeviceCall(awfm, torch, inst)(image, **params), want)


def test_two_streams_on_one_image_at_once(awfm, image):
    import torch
    a, b = rc.sized_instance([300, 5, 4000, 0, 256, 257] * 40, seed=5), rc.random_instance(9, reads=400)
    calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
    params = [dict(band=7, max_candidates=6), dict(band=3, min_votes=2, max_candidates=2)]
    want = [a.host(awfm, **params[0]), b.host(awfm, **params[1])]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pending = [call.run(image, stream=s.cuda_stream, launch=False, **p) for _ in range(3) for call, p, s in zip(calls, params, streams)]
    for enqueue, _ in pending:  # interleaved, nothing waited for in between: each call has its own scratch and outputs
        enqueue()
    torch.cuda.synchronize()
    for k, (_, collect) in enumerate(pending):
        rc.assert_equal(collect(), want[k % 2], what=f"call {k}")


def test_error_codes_and_an_empty_batch(awfm, image):
    import torch
    inst = rc.random_instance(5, reads=4)
    call = DeviceCall(awfm, torch, inst)
    scratch = torch.zeros(awfm.read_candidates_scratch_bytes(4), dtype=torch.uint8, device="cuda")
    assert awfm.read_candidates_scratch_bytes(1 << 20) <= 16 + 4 * (1 << 20) + 16
    out = awfm.candidate_outputs()
    image.read_candidates(call.inputs, 0, out, 0)  # no reads: succeeds, touches nothing
    for kw, code in ((dict(max_candidates=0), awfm.AwFmIllegalPositionError), (dict(max_candidates=17), awfm.AwFmIllegalPositionError)):
        with pytest.raises(awfm.AwFmError) as err:
            image.read_candidates(call.inputs, 4, out, scratch.data_ptr(), **kw)
        assert err.value.rc == code
    with pytest.raises(awfm.AwFmError) as err:
        image.read_candidates(call.inputs, 1 << 32, out, scratch.data_ptr())
    assert err.value.rc == awfm.AwFmIllegalPositionError
    with pytest.raises(awfm.AwFmError) as err:  # no scratch
        image.read_candidates(call.inputs, 4, out, 0)
    assert err.value.rc == -4
    broken = awfm.candidate_inputs(call.arrays[0].data_ptr(), inst.num_seeds, call.arrays[1].data_ptr(), 0, 0, call.arrays[3].data_ptr(),
                                   inst.num_hits, call.arrays[4].data_ptr(), 0)
    with pytest.raises(awfm.AwFmError) as err:  # neither lengths nor a fixed length
        image.read_candidates(broken, 4, out, scratch.data_ptr())
    assert err.value.rc == -4
    torch.cuda.synchronize()


def test_end_to_end_on_the_device_equals_the_host_and_finds_every_planted_read(awfm, require_gpu, tmp_path, wide):
    """reads -> awfmGpuLongestSuffixMatches -> hit offsets -> locate -> awfmGpuLocalPositions -> awfmGpuReadCandidates with the
    kernel's match lengths passed straight in, on one stream; equal to the host's pipeline and twin"""
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
    n = len(starts)
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
    stream_obj.wait_stream(torch.cuda.current_stream())
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), n, total, d_positions.data_ptr(), s)
    g.local_positions(d_positions.data_ptr(), total, d_sequences.data_ptr(), d_positions.data_ptr(), stream=s)
    call = DeviceCall.__new__(DeviceCall)
    call.awfm, call.torch, call.inst = awfm, torch, host
    call.inputs = awfm.candidate_inputs(d_offsets.data_ptr(), n, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), total,
                                        d_positions.data_ptr(), d_sequences.data_ptr())
    for band in (2, 0):
        params = dict(max_hits_per_seed=rc.E2E_MAX_HITS, band=band, min_votes=2, max_candidates=4)
        _, collect = call.run(g, stream=s, **params)
        stream_obj.synchronize()
        got = collect()
        rc.assert_equal(got, host.host(awfm, **params), what=f"band {band}")
        if band == 2:
            rc.assert_planted_reads_found(got, planted, 2)
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
