"""awfmGpuVerifyChains (include/awfm_gpu.h "chain verification", csrc/awfm_verify_kernel.h) against its host twin
awfmVerifyChains, which tests/test_verify_chains.py pins to the plain-Python restatement of the definition and to hand-computed
values: every output, bit for bit, on the edge list at the natural number of lanes per slot and with 32 and 64 forced, with the
read buffer skewed by 1, 2 and 3 bytes, on texts of every length mod 16 whose verified interval ends at the last byte, on a
batch of 2^12 reads x 4 slots in both alphabets, on one slot of 2^20 characters, from two streams at once, without a text, with
the text replaced between two calls, and end to end from a FASTA file.  Every output and the read buffer lie between guard
words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_candidates_common as rc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
from test_verify_chains import long_case  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 64, 0xA5
SIZES = {"editDistances": lambda n, C: 4 * n * C, "bestSlots": lambda n, C: 4 * n, "numUnverified": lambda n, C: 8}


class Image:
    """an index of the case's text with the text and the record table installed"""

    def __init__(self, awfm, case, records=True):
        self.ix = awfm.create_index(case.text, awfm.AwFmAlphabetAmino if case.alphabet == vc.AMINO else awfm.AwFmAlphabetDna, 2, 2)
        self.g = awfm.GpuIndex(self.ix)
        self.g.set_text(case.text)
        if records and case.ends is not None:
            self.g.set_record_table(case.ends)

    def close(self):
        self.g.destroy()
        self.ix.dealloc()


def _upload(torch, array):
    raw = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
    return torch.from_numpy(raw.copy() if raw.size else np.zeros(8, np.uint8)).to("cuda")


class DeviceCall:
    """the arrays of one case on the device -- the read buffer `skew` bytes into its allocation, between guard words -- and
    guarded outputs for calls on them"""

    def __init__(self, awfm, torch, case, skew=0):
        self.awfm, self.torch, self.case = awfm, torch, case
        chars = np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), case.read_chars, np.full(GUARD, PATTERN, np.uint8)))
        self.chars = torch.from_numpy(chars).to("cuda")
        self.offsets = _upload(torch, case.offsets)
        self.slots = {name: _upload(torch, case.slots[name]) for name in vc.SLOT_FIELDS}
        self.inputs = awfm.verify_inputs(self.chars.data_ptr() + GUARD + skew, case.num_read_chars, self.offsets.data_ptr(),
                                         **{name: a.data_ptr() for name, a in self.slots.items()})

    def run(self, g, w, x, outputs=None, stream=0, unverified_before=0, launch=True):
        torch, n, C = self.torch, self.case.num_reads, self.case.C
        outputs = list(SIZES) if outputs is None else list(outputs)
        buffers = {name: torch.full((SIZES[name](n, C) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        if "numUnverified" in outputs:
            buffers["numUnverified"][GUARD:GUARD + 8] = torch.from_numpy(np.array([unverified_before], np.uint64).view(np.uint8)).to("cuda")
        vout = self.awfm.verify_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.verify_chains(self.inputs, n, vout, max_candidates=C, band_pad=w, max_drift=x, stream=stream)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), SIZES[name](n, C)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                result[name] = int(body.view(np.uint64)[0]) if name == "numUnverified" else body.view(np.uint32).reshape((n, C) if name == "editDistances" else (n,))
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, w, x, **kw):
        _, collect = self.run(g, w, x, **kw)
        self.torch.cuda.synchronize()
        return collect()


@pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
def test_edge_list_equals_the_host_twin_and_the_hand_computed_values(awfm, require_gpu, diag, group):
    import torch
    diag(verify_group=group)
    builders = {(w, x): vc.edge_builder(w, x) for w, x in ((2, 3), (8, 15), (3, 4), (24, 15))}  # 8, 32, 11 and 64 diagonals
    image = Image(awfm, builders[2, 3].case())
    try:
        for (w, x), b in builders.items():
            case = b.case()
            want = case.host(awfm, w, x, unverified_before=9)
            assert np.array_equal(want["editDistances"], b.want())
            vc.assert_equal(DeviceCall(awfm, torch, case)(image.g, w, x, unverified_before=9), want, what=f"w={w} x={x}")
        b = builders[2, 3]
        want = b.case().host(awfm, 2, 3)
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            vc.assert_equal(DeviceCall(awfm, torch, b.case(), skew=skew)(image.g, 2, 3), want, what=f"buffer skewed by {skew}")
            vc.assert_equal(DeviceCall(awfm, torch, b.case(skew))(image.g, 2, 3), want, what=f"reads skewed by {skew}")
        call = DeviceCall(awfm, torch, b.case())
        names = list(SIZES)
        for missing in names:  # every output NULL in turn, and alone
            for outputs in ([n for n in names if n != missing], [missing]):
                got = call(image.g, 2, 3, outputs=outputs)
                assert sorted(got) == sorted(outputs)
                vc.assert_equal(got, want, names=outputs, what=str(outputs))
    finally:
        image.close()


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_band_widths_indel_runs_and_inverted_offsets(awfm, require_gpu, diag, group):
    import torch
    diag(verify_group=group)
    for width, (w, x) in sorted(vc.BAND_SHAPES.items()):
        b = vc.band_shape_case(w, x)
        image = Image(awfm, b.case())
        try:
            got = DeviceCall(awfm, torch, b.case())(image.g, w, x)
            assert np.array_equal(got["editDistances"], b.want()), (width, got["editDistances"].tolist(), b.values)
            if width == 64:
                with pytest.raises(awfm.AwFmError) as e:  # 65 diagonals
                    DeviceCall(awfm, torch, b.case())(image.g, 32, 0)
                assert e.value.rc == awfm.AwFmIllegalPositionError
        finally:
            image.close()
    read, text = b"acgtacgtacttgcagcagcag", b"acgtacgtacgcagcagcagtt"
    b = vc.Builder([text])
    b.add("run", read, 0, 22, 0, 0, 22, 4)
    image = Image(awfm, b.case())
    try:
        for w in (2, 1, 0):  # an indel run of exactly w, of w + 1, and pure Hamming
            got = DeviceCall(awfm, torch, b.case())(image.g, w, 0)
            assert int(got["editDistances"][0, 0]) == vc.banded(read, text, w) == int(b.case().host(awfm, w, 0)["editDistances"][0, 0])
    finally:
        image.close()
    b = vc.Builder([b"acgtacgtacgtacgt"])
    for k in range(4):
        b.add(f"read {k}", b"acgt", 0, 4, 0, 4 * k, 4 * k + 4, 0)
    case = b.case()
    case.offsets = np.array([0, 4, 3, 12, 17], np.uint64)
    image = Image(awfm, case, records=False)  # no record table: one sequence (the terminator belongs to it)
    try:
        case.ends = None
        for limit in (16, 11):
            case.num_read_chars = limit
            vc.assert_equal(DeviceCall(awfm, torch, case)(image.g, 2, 3), case.host(awfm, 2, 3), what=f"offsets, {limit} characters")
    finally:
        image.close()


def test_texts_of_every_length_mod_16_verified_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        b = vc.tail_case(length)
        image = Image(awfm, b.case())
        try:
            got = DeviceCall(awfm, torch, b.case())(image.g, 2, 3)
            assert np.array_equal(got["editDistances"], b.want()), (length, got["editDistances"].tolist())
        finally:
            image.close()


@pytest.mark.parametrize("alphabet", [vc.DNA, vc.AMINO], ids=["dna", "amino"])
def test_batch_of_4096_reads_by_4_slots(awfm, require_gpu, alphabet):
    """lengths 1..300 with 63, 64, 65, 127, 128, 129 among them, edits of 0..12 %, a tenth of the slots unused and a few
    malformed, a text of 2^16 positions in 37 records (two empty, one of one residue); and 16 slots a read"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    lengths[:12] = [63, 64, 65, 127, 128, 129, 1, 300, 63, 64, 65, 2]
    case = vc.random_case(17, 1 << 12, 4, alphabet, text_length=1 << 16, num_records=37, lengths=lengths)
    sizes = np.diff(np.concatenate(([-1], case.ends.astype(np.int64)))) - 1
    assert (sizes == 0).sum() >= 2 and (sizes == 1).sum() >= 1 and len(sizes) >= 36
    want = case.host(awfm, 8, 15, threads=16, unverified_before=3)
    distances = want["editDistances"]
    assert 0.05 < (distances == vc.NONE).mean() < 0.2 and (distances == vc.MALFORMED).sum() > 50 and (distances == vc.TOO_WIDE).sum() > 0
    image = Image(awfm, case)
    try:
        vc.assert_equal(DeviceCall(awfm, torch, case)(image.g, 8, 15, unverified_before=3), want)
        small = vc.random_case(23, 300, 16, alphabet, text_length=1 << 16, num_records=37, max_length=150)
        small.text, small.ends = case.text, case.ends  # the same image: slots that leave a record there are malformed on both sides
        for w, x in ((3, 4), (8, 15), (20, 23)):  # 16, 32 and 64 lanes
            vc.assert_equal(DeviceCall(awfm, torch, small)(image.g, w, x), small.host(awfm, w, x, threads=8), what=f"16 slots, w={w} x={x}")
        one = vc.random_case(29, 500, 1, alphabet, text_length=1 << 16, num_records=37, max_length=90)
        one.text, one.ends = case.text, case.ends
        vc.assert_equal(DeviceCall(awfm, torch, one)(image.g, 2, 3), one.host(awfm, 2, 3, threads=8), what="one slot")
    finally:
        image.close()


def test_one_slot_of_two_to_the_twenty_characters(awfm, require_gpu):
    """the too-long boundary: 2^20 characters are verified (one wave's work: 2^20 rows), one more is refused"""
    import torch
    case = long_case()
    want = case.host(awfm, 8, 15)
    assert want["editDistances"].tolist() == [[5, vc.TOO_LONG]]
    image = Image(awfm, case)
    try:
        vc.assert_equal(DeviceCall(awfm, torch, case)(image.g, 8, 15), want)
    finally:
        image.close()


def test_without_a_text_with_the_text_replaced_and_from_two_streams(awfm, require_gpu):
    import torch
    a, b = vc.random_case(5, 600, 4, max_length=200), vc.random_case(6, 500, 3, max_length=120)
    b.text, b.ends = a.text, a.ends
    image = Image(awfm, a)
    try:
        g = image.g
        calls, params = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)], [(8, 15), (2, 3)]
        want = [a.host(awfm, 8, 15), b.host(awfm, 2, 3)]
        g.set_text(None)
        with pytest.raises(awfm.AwFmError) as e:
            g.verify_chains(calls[0].inputs, a.num_reads, awfm.verify_outputs(), max_candidates=4)
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
        g.set_text(a.text)
        g.verify_chains(calls[0].inputs, 0, awfm.verify_outputs())  # no reads: succeeds, touches nothing
        g.verify_chains(calls[0].inputs, a.num_reads, awfm.verify_outputs(), max_candidates=4)  # every output NULL
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(band_pad=32, max_drift=0), dict(band_pad=0, max_drift=64)):
            with pytest.raises(awfm.AwFmError) as e:
                g.verify_chains(calls[0].inputs, a.num_reads, awfm.verify_outputs(), **kw)
            assert e.value.rc == awfm.AwFmIllegalPositionError
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = [call.run(g, *p, stream=s.cuda_stream, launch=False) for _ in range(3) for call, p, s in zip(calls, params, streams)]
        for enqueue, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, (_, collect) in enumerate(pending):
            vc.assert_equal(collect(), want[k % 2], what=f"call {k}")
        # the text replaced between two calls: the same slots against a text whose every fifth character is another one
        other = a.text.copy()
        other[::5] = np.where(other[::5] == 0, 0, ord("n"))
        g.set_text(other)
        changed = vc.Case(a.read_chars.tobytes(), a.offsets, a.slots, other.tobytes(), a.ends)
        got = calls[0](g, 8, 15)
        vc.assert_equal(got, changed.host(awfm, 8, 15), what="replaced text")
        assert not np.array_equal(got["editDistances"], want[0]["editDistances"])
    finally:
        image.close()


def test_end_to_end_from_a_fasta_file(awfm, require_gpu, tmp_path, wide):
    """reads -> longest suffix matches -> hit offsets -> locate -> local positions -> candidates -> chains -> verification, on one
    stream, the chain call's arrays passed straight in.  Reads are planted with a substitution at every 30th character, a third
    of them with one deletion; decoy records carry a copy of a planted read's locus with 8 more substitutions.  The best verified
    slot of every planted read is its record, its distance is at most the edits planted inside the chain's interval and equals the
    unbanded distance of the two intervals, and the decoy's slot gets a strictly larger distance whatever its votes."""
    import torch
    fa, records, reads, planted, decoy_of = vc.planted_with_decoys(str(tmp_path))
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    assert g.is_wide == wide
    text, record_ends = vc.text_of(records)
    g.set_text(text)
    assert g.num_records == len(records)
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
    d_positions = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_sequences = torch.zeros(total, dtype=torch.int32, device="cuda")
    slot32 = {name: torch.zeros(num_reads * slots, dtype=torch.int32, device="cuda") for name in ("sequences", "diagonalSpans", "chainAnchors", "chainReadBegins", "chainReadEnds", "votes")}
    slot64 = {name: torch.zeros(num_reads * slots, dtype=torch.int64, device="cuda") for name in ("diagonals", "chainBeginDiagonals", "chainEndDiagonals")}
    d_scratch = torch.zeros(max(awfm.read_candidates_scratch_bytes(num_reads), awfm.read_chains_scratch_bytes(num_reads)), dtype=torch.uint8, device="cuda")
    d_read_offsets = _upload(torch, np.arange(num_reads + 1, dtype=np.uint64) * rc.E2E_READ_LENGTH)
    stream_obj.wait_stream(torch.cuda.current_stream())
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), n, total, d_positions.data_ptr(), s)
    g.local_positions(d_positions.data_ptr(), total, d_sequences.data_ptr(), d_positions.data_ptr(), stream=s)
    inputs = awfm.candidate_inputs(d_offsets.data_ptr(), n, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), total,
                                   d_positions.data_ptr(), d_sequences.data_ptr())
    cand = awfm.candidate_outputs(sequences=slot32["sequences"].data_ptr(), diagonals=slot64["diagonals"].data_ptr(),
                                  diagonalSpans=slot32["diagonalSpans"].data_ptr(), votes=slot32["votes"].data_ptr())
    g.read_candidates(inputs, num_reads, cand, d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=2, min_votes=2, max_candidates=slots, stream=s)
    chain_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    chains = awfm.chain_outputs(**{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    g.read_chains(inputs, num_reads, slot32["sequences"].data_ptr(), slot64["diagonals"].data_ptr(), slot32["diagonalSpans"].data_ptr(), chains,
                  d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=2, max_candidates=slots, gap_penalty=1, stream=s)
    d_distances = torch.full((num_reads * slots,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_best = torch.full((num_reads,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_unverified = torch.zeros(1, dtype=torch.int64, device="cuda")
    vin = awfm.verify_inputs(d_chars.data_ptr(), len(chars), d_read_offsets.data_ptr(), sequences=slot32["sequences"].data_ptr(),
                             **{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    vout = awfm.verify_outputs(editDistances=d_distances.data_ptr(), bestSlots=d_best.data_ptr(), numUnverified=d_unverified.data_ptr())
    g.verify_chains(vin, num_reads, vout, max_candidates=slots, band_pad=8, max_drift=15, stream=s)
    stream_obj.synchronize()
    slot_arrays = {name: (slot32.get(name) if name in slot32 else slot64[name]).cpu().numpy().view(vc.SLOT_DTYPES[name]).reshape(num_reads, slots)
                   for name in vc.SLOT_FIELDS}
    case = vc.Case(chars.tobytes(), np.arange(num_reads + 1) * rc.E2E_READ_LENGTH, slot_arrays, text.tobytes(), record_ends)
    got = dict(editDistances=d_distances.cpu().numpy().view(np.uint32).reshape(num_reads, slots), bestSlots=d_best.cpu().numpy().view(np.uint32),
               numUnverified=int(d_unverified.cpu().numpy()[0]))
    vc.assert_equal(got, case.host(awfm, 8, 15))
    assert got["numUnverified"] == 0  # chains made from located hits are never malformed
    vc.assert_planted_reads_verified(case, got, planted, decoy_of)
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
