"""awfmGpuAlignChainsAffine (include/awfm_gpu.h "affine alignment", csrc/awfm_align_affine_kernel.h) against its host twin
awfmAlignChainsAffine, which tests/test_align_affine.py pins to the plain-Python restatement of the definition and to hand-computed
values: every output, bit for bit, except the rows of ops of truncated reads -- on the edge lists at the natural number of lanes
per read and with 32 and 64 forced, with the read buffer skewed by 1, 2 and 3 bytes, on reads of every length around the chunk
edges at every band width and two scorings, on texts of every length mod 16, on a batch of 2^12 reads in both alphabets, on
more reads than the grid has waves, on one read of maxRows characters and one more, from two streams at once, without a text,
and end to end from a FASTA file.  Inputs, outputs and the scratch (exactly its declared size) lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import test_gpu_align_chains as gac  # noqa: E402
from test_align_affine import long_affine_case, long_expected  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, Image, _upload  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = {name: (lambda n, m, size=np.dtype(dtype).itemsize: size * n) for name, dtype in af.READ_OUTPUTS.items()}
SIZES.update(ops=lambda n, m: 4 * n * m, numUnaligned=lambda n, m: 8, numTruncated=lambda n, m: 8)
DTYPES = dict(af.READ_OUTPUTS, ops=np.uint32)
longest_read = gac.longest_read


class Scratch(gac.Scratch):
    """exactly awfmGpuAlignChainsAffineScratchBytes bytes between guard words"""

    def __init__(self, torch, g, max_rows):
        self.max_rows, self.size = max_rows, g.align_chains_affine_scratch_bytes(max_rows)
        assert self.size > 0 and self.size % 16 == 0
        self.buffer = torch.full((self.size + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        self.address = self.buffer.data_ptr() + GUARD


class DeviceCall(gac.DeviceCall):
    """gac.DeviceCall's arrays on the device and guarded outputs for the affine call on them"""

    def run(self, g, w, x, scratch, scoring=af.DEFAULT, max_ops=32, outputs=None, stream=0, unaligned_before=0, truncated_before=0, launch=True):
        torch, n = self.torch, self.case.num_reads
        outputs = list(SIZES) if outputs is None else list(outputs)
        buffers = {name: torch.full((SIZES[name](n, max_ops) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        for name, before in (("numUnaligned", unaligned_before), ("numTruncated", truncated_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        aout = self.awfm.affine_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.align_chains_affine(self.inputs, self.chosen.data_ptr(), n, aout, scratch.address, max_candidates=self.case.C, band_pad=w,
                                  max_drift=x, scoring=scoring, max_ops=max_ops, max_rows=scratch.max_rows, stream=stream)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), SIZES[name](n, max_ops)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                if name in af.COUNTERS:
                    result[name] = int(body.view(np.uint64)[0])
                else:
                    result[name] = body.view(DTYPES[name]).reshape((n, max_ops) if name == "ops" else (n,))
            scratch.check()
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect


@pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
def test_edge_lists_equal_the_host_twin_and_the_hand_computed_values(awfm, require_gpu, diag, group):
    import torch
    diag(affine_group=group)
    builders = {(w, x): af.edge_builder(w, x) for w, x in ((2, 3), (8, 15), (3, 4), (24, 15))}  # 8, 32, 11 and 64 diagonals
    image = Image(awfm, builders[2, 3].case())
    try:
        scratch = Scratch(torch, image.g, 64)
        for (w, x), b in builders.items():
            case = b.case()
            want = case.host(awfm, w, x, max_ops=8, unaligned_before=9, truncated_before=2)
            got = DeviceCall(awfm, torch, case)(image.g, w, x, scratch, max_ops=8, unaligned_before=9, truncated_before=2)
            af.assert_equal(got, want, what=f"w={w} x={x}", fill=PATTERN)
            b.check(got, 8)
        for b, w, x, scoring in ((af.outside_builder(), 0, 0, af.DEFAULT), (af.unit_builder(), 2, 3, (1, 1, 0, 1))):
            got = DeviceCall(awfm, torch, b.case())(image.g, w, x, scratch, scoring=scoring, max_ops=8)
            af.assert_equal(got, b.case().host(awfm, w, x, scoring, max_ops=8), what=f"w={w} {scoring}", fill=PATTERN)
            b.check(got, 8)
        b = builders[2, 3]
        case = b.case()
        want = case.host(awfm, 2, 3, max_ops=8)
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            af.assert_equal(DeviceCall(awfm, torch, case, skew=skew)(image.g, 2, 3, scratch, max_ops=8), want, what=f"buffer skewed by {skew}")
            af.assert_equal(DeviceCall(awfm, torch, b.case(skew))(image.g, 2, 3, scratch, max_ops=8), want, what=f"reads skewed by {skew}")
        call = DeviceCall(awfm, torch, case)
        for max_ops in (4, 3):  # exactly the most runs of a read, and one less: the rows lie in one guarded array, each behind the other
            af.assert_equal(call(image.g, 2, 3, scratch, max_ops=max_ops), case.host(awfm, 2, 3, max_ops=max_ops), what=f"{max_ops} runs", fill=PATTERN)
        names = list(SIZES)
        for missing in names:  # every output NULL in turn, and alone
            for outputs in ([n for n in names if n != missing], [missing]):
                got = call(image.g, 2, 3, scratch, max_ops=8, outputs=outputs)
                assert sorted(got) == sorted(outputs)
                af.assert_equal(got, want, names=outputs, what=str(outputs))
        # maxRows at the longest read's length and one less: the rule of the device side, restated
        longest = int(np.diff(case.offsets.astype(np.int64)).max())
        for max_rows in (longest, longest - 1):
            want_rows = case.expected(2, 3, max_ops=8, max_rows=max_rows)
            assert ((want_rows["scores"] == af.TOO_LONG).sum() > 0) == (max_rows < longest)
            af.assert_equal(call(image.g, 2, 3, Scratch(torch, image.g, max_rows), max_ops=8), want_rows, what=f"maxRows {max_rows}", fill=PATTERN)
    finally:
        image.close()


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_read_lengths_around_the_chunk_edges_at_every_band_width(awfm, require_gpu, diag, group):
    import torch
    diag(affine_group=group)
    b = af.shapes_builder()
    image = Image(awfm, b.case())
    try:
        scratch = Scratch(torch, image.g, 300)
        for width, (w, x) in sorted(af.BAND_SHAPES.items()):
            scoring = af.DEFAULT if width % 2 else (2, 4, 4, 2)
            for skew in (0, 1, 2, 3):
                case = b.case(skew)
                want = case.host(awfm, w, x, scoring, max_ops=16)
                assert want["numUnaligned"] == 0 and (want["scores"][3:] > 0).all()
                got = DeviceCall(awfm, torch, case, skew=(4 - skew) % 4 if width % 2 else skew)(image.g, w, x, scratch, scoring=scoring, max_ops=16)
                af.assert_equal(got, want, what=f"width {width} skew {skew}", fill=PATTERN)
            other = (2, 4, 4, 2) if width % 2 else af.DEFAULT  # both scorings at every width
            af.assert_equal(DeviceCall(awfm, torch, case)(image.g, w, x, scratch, scoring=other, max_ops=16), case.host(awfm, w, x, other, max_ops=16),
                            what=f"width {width} {other}", fill=PATTERN)
            if width == 64:
                with pytest.raises(awfm.AwFmError) as e:  # 65 diagonals
                    DeviceCall(awfm, torch, case)(image.g, 32, 0, scratch)
                assert e.value.rc == awfm.AwFmIllegalPositionError
    finally:
        image.close()


def test_texts_of_every_length_mod_16_aligned_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        b = af.tail_case(length)
        image = Image(awfm, b.case())
        try:
            got = DeviceCall(awfm, torch, b.case())(image.g, 2, 3, Scratch(torch, image.g, 32))
            b.check(got, 32)
        finally:
            image.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_batch_of_4096_reads(awfm, require_gpu, alphabet):
    """lengths 1..300 with the chunk edges among them, edits of 0..12 %, a tenth of the slots unused, some malformed, a tenth
    hanging over a record end, a text of 2^16 positions in 37 records (two empty, one of one residue); then sixteen slots a read"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    lengths[:12] = [63, 64, 65, 127, 128, 129, 1, 300, 63, 64, 65, 2]
    case = af.random_case(20, 1 << 12, 4, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, hanging=0.1, other=0.005)
    want = case.host(awfm, 8, 15, max_ops=64, threads=16, unaligned_before=3, truncated_before=1)
    s = want["scores"]
    hanging = sum(ac.Case.status(case, r, 8, 15) == ac.OVERHANG for r in range(case.num_reads))
    assert 0.05 < (s == af.NONE).mean() < 0.3 and (s == af.MALFORMED).sum() > 50 and hanging > 50
    assert want["numTruncated"] - 1 < 0.01 * (s < af.TOO_LONG).sum()
    image = Image(awfm, case)
    try:
        small = af.random_case(23, 300, 16, alphabet, text_length=1 << 16, num_records=37, max_length=150, hanging=0.1)
        scratch = Scratch(torch, image.g, longest_read(case, small))
        got = DeviceCall(awfm, torch, case)(image.g, 8, 15, scratch, max_ops=64, unaligned_before=3, truncated_before=1)
        af.assert_equal(got, want, fill=PATTERN)
        small.text, small.ends = case.text, case.ends  # the same image: slots that leave a record there are malformed on both sides
        for (w, x), scoring in zip(((3, 4), (8, 15), (20, 23)), ((2, 4, 4, 2), (1, 1, 0, 1), (1, 0, 0, 1))):  # 16, 32 and 64 lanes
            got = DeviceCall(awfm, torch, small)(image.g, w, x, scratch, scoring=scoring, max_ops=24)
            af.assert_equal(got, small.host(awfm, w, x, scoring, max_ops=24, threads=8), what=f"16 slots, w={w} x={x}", fill=PATTERN)
    finally:
        image.close()


def test_more_reads_than_the_grid_has_waves_and_a_read_of_max_rows(awfm, require_gpu, diag):
    """4100 reads of 200..600 characters with 64 lanes each: more than the 4096 waves of the largest grid; and with maxRows = 4096
    one read of 4096 characters and one of 4097, which is too long, under (1, 4, 6, 1) and (255, 255, 255, 255)"""
    import torch
    diag(affine_group=64)
    rng = np.random.default_rng(43)
    case = af.random_case(19, 4100, 1, text_length=1 << 16, num_records=37, lengths=rng.integers(200, 601, 4100), max_rate=0.06)
    want = case.host(awfm, 8, 15, max_ops=64, threads=16)
    image = Image(awfm, case)
    try:
        af.assert_equal(DeviceCall(awfm, torch, case)(image.g, 8, 15, Scratch(torch, image.g, longest_read(case)), max_ops=64), want, fill=PATTERN)
    finally:
        image.close()
    diag(affine_group=None)
    long = long_affine_case(4096)
    image = Image(awfm, long)
    try:
        scratch = Scratch(torch, image.g, 4096)
        for scoring in (af.DEFAULT, (255, 255, 255, 255)):
            want = long.host(awfm, 8, 15, scoring)
            assert (int(want["scores"][1]) > 0) and af.cigar(af.runs_of(want["ops"][0], int(want["numOps"][0]))) == long_expected(4096)[5]
            for name in af.READ_OUTPUTS:  # (the host's limit is 2^16)
                want[name][1] = af.TOO_LONG if name == "scores" else 0
            want["numUnaligned"] = 1
            got = DeviceCall(awfm, torch, long)(image.g, 8, 15, scratch, scoring=scoring)
            af.assert_equal(dict(got, ops=got["ops"][:1]), dict(want, ops=want["ops"][:1], numOps=want["numOps"][:1]), names=["ops"])
            af.assert_equal(got, want, names=[n for n in want if n != "ops"])
            assert (got["ops"][1] == PATTERN * 0x01010101).all()
    finally:
        image.close()


def test_without_a_text_bad_arguments_and_two_streams_with_a_scratch_each(awfm, require_gpu):
    import torch
    a, b = af.random_case(5, 600, 4, max_length=200, hanging=0.1), af.random_case(6, 500, 3, max_length=120, hanging=0.1)
    b.text, b.ends = a.text, a.ends
    image = Image(awfm, a)
    try:
        g = image.g
        calls, params = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)], [(8, 15, af.DEFAULT), (2, 3, (2, 4, 4, 2))]
        want = [a.host(awfm, 8, 15), b.host(awfm, 2, 3, (2, 4, 4, 2))]
        scratches = [Scratch(torch, g, longest_read(a)), Scratch(torch, g, longest_read(b))]
        args = (calls[0].inputs, calls[0].chosen.data_ptr(), a.num_reads, awfm.affine_outputs(), scratches[0].address)
        g.set_text(None)
        with pytest.raises(awfm.AwFmError) as e:
            g.align_chains_affine(*args, max_candidates=4, max_rows=scratches[0].max_rows)
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
        g.set_text(a.text)
        g.align_chains_affine(calls[0].inputs, 0, 0, awfm.affine_outputs(), 0)  # no reads: succeeds, touches nothing
        g.align_chains_affine(*args, max_candidates=4, max_rows=scratches[0].max_rows)  # every output NULL
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(band_pad=32, max_drift=0), dict(band_pad=0, max_drift=64), dict(max_ops=0),
                   dict(max_ops=af.MAX_OPS + 1), dict(max_rows=0), dict(max_rows=af.MAX_LENGTH + 1), dict(scoring=(0, 4, 6, 1)),
                   dict(scoring=(256, 4, 6, 1)), dict(scoring=(1, 256, 6, 1)), dict(scoring=(1, 4, 256, 1)), dict(scoring=(1, 4, 6, 0)),
                   dict(scoring=(1, 4, 6, 256))):
            with pytest.raises(awfm.AwFmError) as e:
                g.align_chains_affine(*args, **dict(dict(max_candidates=4, max_rows=scratches[0].max_rows), **kw))
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        for scoring in ((1, 0, 0, 1), (255, 255, 255, 255)):  # the bounds themselves
            g.align_chains_affine(*args, max_candidates=4, max_rows=scratches[0].max_rows, scoring=scoring)
        for bad, kw in (((args[0], 0) + args[2:], {}), (args[:4] + (0,), {}), (args, dict(scoring=None))):  # no slots, no scratch, no scoring
            with pytest.raises(awfm.AwFmError) as e:
                g.align_chains_affine(*bad, max_candidates=4, max_rows=scratches[0].max_rows, **kw)
            assert e.value.rc == -4  # AwFmNullPtrError
        with pytest.raises(awfm.AwFmError) as e:  # a scratch that is not aligned to 16 bytes
            g.align_chains_affine(*(args[:4] + (scratches[0].address + 4,)), max_candidates=4, max_rows=100)
        assert e.value.rc == awfm.AwFmIllegalPositionError
        assert g.align_chains_affine_scratch_bytes(0) == 0 and g.align_chains_affine_scratch_bytes(af.MAX_LENGTH + 1) == 0
        assert g.align_chains_affine_scratch_bytes(300) == 300 * g.align_chains_affine_scratch_bytes(1)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = []
        for _ in range(3):  # a call's scratch is its own until it has finished: the calls of a stream follow each other
            for call, (w, x, scoring), s, scratch in zip(calls, params, streams, scratches):
                pending.append(call.run(g, w, x, scratch, scoring=scoring, stream=s.cuda_stream, launch=False))
        for enqueue, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, (_, collect) in enumerate(pending):
            af.assert_equal(collect(), want[k % 2], what=f"call {k}", fill=PATTERN)
        for s in streams:
            g.stream_retire(s.cuda_stream)
    finally:
        image.close()


def test_end_to_end_from_a_fasta_file(awfm, require_gpu, tmp_path):
    """reads -> longest suffix matches -> hit offsets -> locate -> local positions -> candidates -> chains -> verification ->
    affine alignment of verification's best slots, on one stream, every call's arrays passed straight to the next.  Every output
    equals the host twin's on the same slots; every planted read (a substitution at every 30th character, a third of them with
    one deletion) is aligned to its record within bandPad of the planted interval, and its script replays to its score."""
    import torch
    fa, records, reads, planted = ac.planted_inside(str(tmp_path), vc.E2E_W)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    text, record_ends = vc.text_of(records)
    g.set_text(text)
    assert g.num_records == len(records)
    chars, starts, ends, offsets, seed_ends = rc.windows_of(reads)
    n, num_reads, slots, max_ops = len(starts), len(reads), 4, 32
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
    d_best = torch.full((num_reads,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_align = {name: torch.full((num_reads * (max_ops if name == "ops" else 1),), 0x5A5A5A5A, dtype=torch.int64 if np.dtype(dtype).itemsize == 8 else torch.int32, device="cuda")
               for name, dtype in DTYPES.items()}
    d_counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    scratch = Scratch(torch, g, rc.E2E_READ_LENGTH)
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
    vin = awfm.verify_inputs(d_chars.data_ptr(), len(chars), d_read_offsets.data_ptr(), sequences=slot32["sequences"].data_ptr(),
                             **{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    g.verify_chains(vin, num_reads, awfm.verify_outputs(bestSlots=d_best.data_ptr()), max_candidates=slots, band_pad=vc.E2E_W, max_drift=vc.E2E_X, stream=s)
    aout = awfm.affine_outputs(numUnaligned=d_counters.data_ptr(), numTruncated=d_counters.data_ptr() + 8, **{name: a.data_ptr() for name, a in d_align.items()})
    g.align_chains_affine(vin, d_best.data_ptr(), num_reads, aout, scratch.address, max_candidates=slots, band_pad=vc.E2E_W, max_drift=vc.E2E_X,
                          max_ops=max_ops, max_rows=rc.E2E_READ_LENGTH, stream=s)
    stream_obj.synchronize()
    scratch.check()
    slot_arrays = {name: (slot32.get(name) if name in slot32 else slot64[name]).cpu().numpy().view(vc.SLOT_DTYPES[name]).reshape(num_reads, slots)
                   for name in vc.SLOT_FIELDS}
    case = af.Case(chars.tobytes(), np.arange(num_reads + 1) * rc.E2E_READ_LENGTH, slot_arrays, d_best.cpu().numpy().view(np.uint32), text.tobytes(), record_ends)
    got = {name: d_align[name].cpu().numpy().view(dtype).reshape((num_reads, max_ops) if name == "ops" else (num_reads,)) for name, dtype in DTYPES.items()}
    got["numUnaligned"], got["numTruncated"] = (int(v) for v in d_counters.cpu().numpy())
    af.assert_equal(got, case.host(awfm, vc.E2E_W, vc.E2E_X, max_ops=max_ops), fill=0x5A)
    assert got["numTruncated"] == 0
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        end = at + rc.E2E_READ_LENGTH + (1 if deleted else 0)
        assert case.slots["sequences"][r, int(case.chosen[r])] == record and int(got["scores"][r]) >= rc.E2E_READ_LENGTH - 40, (r, plant)
        assert abs(int(got["textBegins"][r]) - int(got["readBegins"][r]) - at) <= vc.E2E_W and abs(int(got["textEnds"][r]) - end) <= vc.E2E_W + 30, (r, plant)
    assert af.assert_scripts_replay(case, got, vc.E2E_W, vc.E2E_X, af.DEFAULT, max_ops) >= sum(p is not None for p in planted)
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
