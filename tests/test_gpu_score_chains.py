"""awfmGpuScoreChainsAffine (include/awfm_gpu.h "slot scores and mapping quality", csrc/awfm_score_affine_kernel.h) against its
host twin awfmScoreChainsAffine, which tests/test_score_chains.py pins to the plain-Python restatement, to awfmAlignChainsAffine and
to hand-computed values: every output, bit for bit -- on the edge lists at the natural number of lanes per slot and with 32 and
64 forced, with the read buffer skewed by 1, 2 and 3 bytes, on reads of every length around the chunk edges at every band shape
and two scorings, on texts of every length mod 16, on batches of 2^12 reads with 4 and 16 slots in both alphabets, on more reads
than the grid has waves, on one read of 2^16 characters in 16 slots and one more, from two streams at once, without a text, and
end to end from a FASTA file.  Every output and the read buffer lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import test_gpu_verify_chains as gvc  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, Image, _upload  # noqa: E402
from test_score_chains import long_scored_case  # noqa: E402
from test_align_affine import long_expected  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = dict(sc.SLOT_OUTPUTS, **sc.READ_OUTPUTS)
SIZES = {name: (lambda n, C, size=np.dtype(dtype).itemsize: size * n * C) for name, dtype in sc.SLOT_OUTPUTS.items()}
SIZES.update({name: (lambda n, C, size=np.dtype(dtype).itemsize: size * n) for name, dtype in sc.READ_OUTPUTS.items()})
SIZES.update(numUnscored=lambda n, C: 8, numMapped=lambda n, C: 8)


class DeviceCall(gvc.DeviceCall):
    """gvc.DeviceCall's arrays on the device and guarded outputs for the scoring call on them"""

    def run(self, g, w, x, scoring=af.DEFAULT, min_score=0, cap=60, outputs=None, stream=0, unscored_before=0, mapped_before=0, launch=True):
        torch, n, C = self.torch, self.case.num_reads, self.case.C
        outputs = list(SIZES) if outputs is None else list(outputs)
        buffers = {name: torch.full((SIZES[name](n, C) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        for name, before in (("numUnscored", unscored_before), ("numMapped", mapped_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        sout = self.awfm.slot_score_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        torch.cuda.synchronize()

        def enqueue():
            g.score_chains_affine(self.inputs, n, sout, max_candidates=C, band_pad=w, max_drift=x, scoring=scoring, min_score=min_score,
                                  mapq_cap=cap, stream=stream)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), SIZES[name](n, C)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                if name in sc.COUNTERS:
                    result[name] = int(body.view(np.uint64)[0])
                else:
                    result[name] = body.view(DTYPES[name]).reshape((n, C) if name in sc.SLOT_OUTPUTS else (n,))
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, w, x, **kw):
        _, collect = self.run(g, w, x, **kw)
        self.torch.cuda.synchronize()
        return collect()


@pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
def test_edge_lists_equal_the_host_twin_and_the_hand_computed_values(awfm, require_gpu, diag, group):
    import torch
    diag(score_group=group)
    rules = {C: sc.rules_builder(C) for C in (4, 1, 16)}
    image = Image(awfm, rules[4].case())
    try:
        for C, b in rules.items():
            case = b.case()
            for min_score in (0, 38, 100, 101):
                want = case.score(awfm, 8, 15, min_score=min_score, unscored_before=9, mapped_before=2)
                got = DeviceCall(awfm, torch, case)(image.g, 8, 15, min_score=min_score, unscored_before=9, mapped_before=2)
                sc.assert_equal(got, want, what=f"C={C} minScore={min_score}")
                if min_score == 0:
                    b.check(got)
        b, case = rules[4], rules[4].case()
        want = case.score(awfm, 8, 15)
        for cap in (0, 1, 254):
            sc.assert_equal(DeviceCall(awfm, torch, case)(image.g, 8, 15, cap=cap), case.score(awfm, 8, 15, cap=cap), what=f"cap {cap}")
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            sc.assert_equal(DeviceCall(awfm, torch, case, skew=skew)(image.g, 8, 15), want, what=f"buffer skewed by {skew}")
            sc.assert_equal(DeviceCall(awfm, torch, b.case(skew))(image.g, 8, 15), want, what=f"reads skewed by {skew}")
        call = DeviceCall(awfm, torch, case)
        for missing in SIZES:  # every output NULL in turn, and alone
            for outputs in ([n for n in SIZES if n != missing], [missing]):
                got = call(image.g, 8, 15, outputs=outputs)
                assert sorted(got) == sorted(outputs)
                sc.assert_equal(got, want, names=outputs, what=str(outputs))
    finally:
        image.close()
    # the per-slot edge lists of affine alignment: every malformed shape, every overhang, bands outside the record, unit costs
    builders = [(af.edge_builder(w, x), w, x, af.DEFAULT) for w, x in ((2, 3), (8, 15), (3, 4), (24, 15))]  # 8, 32, 11 and 64 diagonals
    builders += [(af.outside_builder(), 0, 0, af.DEFAULT), (af.unit_builder(), 2, 3, (1, 1, 0, 1))]
    image = Image(awfm, builders[0][0].case())
    try:
        for b, w, x, scoring in builders:
            case = sc.as_scored(b.case())
            got = DeviceCall(awfm, torch, case)(image.g, w, x, scoring=scoring, unscored_before=1)
            sc.assert_equal(got, case.score(awfm, w, x, scoring, unscored_before=1), what=f"w={w} x={x} {scoring}")
            for r, value in enumerate(b.values):  # the hand-computed values of the affine list: score, readEnd, textEnd
                if isinstance(value, tuple) and int(case.chosen[r]) == 0:
                    assert (int(got["slotScores"][r, 0]), int(got["slotReadEnds"][r, 0]), int(got["slotTextEnds"][r, 0])) == (value[0], value[2], value[4]), b.names[r]
    finally:
        image.close()


@pytest.mark.parametrize("group", [None, 64], ids=["natural", "64"])
def test_read_lengths_around_the_chunk_edges_at_every_band_shape(awfm, require_gpu, diag, group):
    import torch
    diag(score_group=group)
    b = af.shapes_builder()
    image = Image(awfm, b.case())
    try:
        for width, (w, x) in sorted(af.BAND_SHAPES.items()):
            scoring = af.DEFAULT if width % 2 else (2, 4, 4, 2)
            for skew in (0, 1, 2, 3):
                case = sc.as_scored(b.case(skew))
                want = case.score(awfm, w, x, scoring)
                assert want["numUnscored"] == 0 and (want["slotScores"][3:] > 0).all()
                got = DeviceCall(awfm, torch, case, skew=(4 - skew) % 4 if width % 2 else skew)(image.g, w, x, scoring=scoring)
                sc.assert_equal(got, want, what=f"width {width} skew {skew}")
            other = (2, 4, 4, 2) if width % 2 else af.DEFAULT  # both scorings at every width
            sc.assert_equal(DeviceCall(awfm, torch, case)(image.g, w, x, scoring=other), case.score(awfm, w, x, other), what=f"width {width} {other}")
            if width == 64:
                with pytest.raises(awfm.AwFmError) as e:  # 65 diagonals
                    DeviceCall(awfm, torch, case)(image.g, 32, 0)
                assert e.value.rc == awfm.AwFmIllegalPositionError
    finally:
        image.close()


def test_texts_of_every_length_mod_16_scored_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        b = af.tail_case(length)
        case = sc.as_scored(b.case())
        image = Image(awfm, case)
        try:
            got = DeviceCall(awfm, torch, case)(image.g, 2, 3)
            sc.assert_equal(got, case.score(awfm, 2, 3), what=f"length {length}")
            for r, value in enumerate(b.values):
                assert (int(got["slotScores"][r, 0]), int(got["slotReadEnds"][r, 0]), int(got["slotTextEnds"][r, 0])) == (value[0], value[2], value[4])
        finally:
            image.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_batches_of_4096_reads_with_4_and_16_slots(awfm, require_gpu, alphabet):
    """lengths 1..300 with the chunk edges among them, edits of 0..12 %, a tenth of the slots unused, some malformed, a tenth
    hanging over a record end, a text of 2^16 positions in 37 records (two empty, one of one residue)"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    lengths[:12] = [63, 64, 65, 127, 128, 129, 1, 300, 63, 64, 65, 2]
    four = sc.random_case(20, 1 << 12, 4, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, hanging=0.1, other=1.0)
    sixteen = sc.random_case(20, 1 << 12, 16, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, hanging=0.1, other=1.0)
    assert np.array_equal(sixteen.text, four.text) and np.array_equal(sixteen.ends, four.ends)  # (the seed's text comes before its reads)
    image = Image(awfm, four)
    try:
        for case, (w, x), scoring in ((four, (8, 15), af.DEFAULT), (sixteen, (3, 4), (2, 4, 4, 2)), (sixteen, (20, 23), (1, 1, 0, 1))):  # 32, 16, 64 lanes
            want = case.score(awfm, w, x, scoring, min_score=10, threads=16, unscored_before=3, mapped_before=1)
            s = want["slotScores"]
            assert 0.05 < (s == sc.NONE).mean() < 0.3 and (s == sc.MALFORMED).sum() > 50 and (want["secondSlots"] != sc.NO_SLOT).sum() > 0
            assert 0 < (want["bestSlots"] == sc.NO_SLOT).sum() and want["numMapped"] > 3000
            got = DeviceCall(awfm, torch, case)(image.g, w, x, scoring=scoring, min_score=10, unscored_before=3, mapped_before=1)
            sc.assert_equal(got, want, what=f"C={case.C} w={w} x={x}")
    finally:
        image.close()


def test_more_reads_than_the_grid_has_waves(awfm, require_gpu, diag):
    """2^13 reads of 200..600 characters with 64 lanes a slot: more than the waves of the largest persistent grid"""
    import torch
    diag(score_group=64)
    rng = np.random.default_rng(43)
    case = sc.random_case(19, 1 << 13, 1, text_length=1 << 16, num_records=37, lengths=rng.integers(200, 601, 1 << 13), max_rate=0.06)
    want = case.score(awfm, 8, 15, threads=16)
    image = Image(awfm, case)
    try:
        sc.assert_equal(DeviceCall(awfm, torch, case)(image.g, 8, 15), want)
    finally:
        image.close()


def test_a_read_of_two_to_the_sixteen_characters_in_16_slots_and_one_more(awfm, require_gpu):
    import torch
    n = af.MAX_LENGTH
    long = long_scored_case(n, 16)
    image = Image(awfm, long)
    try:
        for scoring in (af.DEFAULT, (255, 255, 255, 255)):
            want = long.score(awfm, 8, 15, scoring, threads=16)
            assert (want["slotScores"][1] == sc.TOO_LONG).all() and want["numUnscored"] == 16 and want["bestSlots"].tolist() == [0, sc.NO_SLOT]
            assert scoring != af.DEFAULT or want["slotScores"][0].tolist() == [long_expected(n)[0]] * 16
            assert want["secondSlots"].tolist() == [sc.NO_SLOT] * 2  # sixteen times the same alignment: duplicates, not competitors
            sc.assert_equal(DeviceCall(awfm, torch, long)(image.g, 8, 15, scoring=scoring), want, what=str(scoring))
    finally:
        image.close()


def test_without_a_text_bad_arguments_and_two_streams(awfm, require_gpu):
    import torch
    a, b = sc.random_case(5, 600, 4, max_length=200, hanging=0.1), sc.random_case(6, 500, 3, max_length=120, hanging=0.1)
    b.text, b.ends = a.text, a.ends
    image = Image(awfm, a)
    try:
        g = image.g
        calls, params = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)], [(8, 15, af.DEFAULT), (2, 3, (2, 4, 4, 2))]
        want = [a.score(awfm, 8, 15), b.score(awfm, 2, 3, (2, 4, 4, 2))]
        counters = torch.zeros(2, dtype=torch.int64, device="cuda")
        args = (calls[0].inputs, a.num_reads, awfm.slot_score_outputs(numUnscored=counters.data_ptr(), numMapped=counters.data_ptr() + 8))
        g.set_text(None)
        with pytest.raises(awfm.AwFmError) as e:
            g.score_chains_affine(*args, max_candidates=4)
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
        g.set_text(a.text)
        g.score_chains_affine(calls[0].inputs, 0, awfm.slot_score_outputs(), mapq_cap=255)  # no reads: succeeds, touches nothing
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(band_pad=32, max_drift=0), dict(band_pad=0, max_drift=64), dict(mapq_cap=255),
                   dict(mapq_cap=2 ** 32 - 1), dict(scoring=(0, 4, 6, 1)), dict(scoring=(256, 4, 6, 1)), dict(scoring=(1, 256, 6, 1)),
                   dict(scoring=(1, 4, 256, 1)), dict(scoring=(1, 4, 6, 0)), dict(scoring=(1, 4, 6, 256))):
            with pytest.raises(awfm.AwFmError) as e:
                g.score_chains_affine(*args, **dict(dict(max_candidates=4), **kw))
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        with pytest.raises(awfm.AwFmError) as e:
            g.score_chains_affine(*args, max_candidates=4, scoring=None)
        assert e.value.rc == -4  # AwFmNullPtrError
        torch.cuda.synchronize()
        assert counters.cpu().tolist() == [0, 0]  # the refused calls launched nothing
        g.score_chains_affine(calls[0].inputs, a.num_reads, awfm.slot_score_outputs(), max_candidates=4)  # every output NULL
        for scoring in ((1, 0, 0, 1), (255, 255, 255, 255)):  # the bounds themselves
            g.score_chains_affine(*args, max_candidates=4, scoring=scoring, mapq_cap=254, min_score=2 ** 32 - 1)
        torch.cuda.synchronize()
        assert counters.cpu().tolist() == [2 * want[0]["numUnscored"], 0]  # (minScore above every score: nothing mapped)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = []
        for _ in range(3):  # no scratch: the calls of two streams share nothing but the image
            for call, (w, x, scoring), s in zip(calls, params, streams):
                pending.append(call.run(g, w, x, scoring=scoring, stream=s.cuda_stream, launch=False))
        for enqueue, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, (_, collect) in enumerate(pending):
            sc.assert_equal(collect(), want[k % 2], what=f"call {k}")
        for s in streams:
            g.stream_retire(s.cuda_stream)
    finally:
        image.close()


def test_end_to_end_from_a_fasta_file(awfm, require_gpu, tmp_path):
    """reads -> longest suffix matches -> hit offsets -> locate -> local positions -> candidates -> chains -> slot scores -> affine
    alignment of the scoring call's best slots, on one stream, every call's arrays passed straight to the next.  Every output
    equals the host twin's on the same slots; EVERY planted read's best slot is its own record; where its decoy (8 more
    substitutions) has a slot, that is the second, strictly smaller, and mapq > 0; the reads of the record that stands in the file
    twice have mapq 0; and the affine call on the device's bestSlots returns scores == bestScores."""
    import torch
    fa, records, reads, planted, decoy_of, copies = sc.e2e_records(str(tmp_path))
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    text, record_ends = vc.text_of(records)
    g.set_text(text)
    assert g.num_records == len(records)
    chars, starts, ends, offsets, seed_ends = rc.windows_of(reads)
    n, num_reads, slots, max_ops = len(starts), len(reads), sc.E2E_SLOTS, 32
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
    d_scores = {name: torch.full((np.dtype(dtype).itemsize * num_reads * (slots if name in sc.SLOT_OUTPUTS else 1),), 0x5A, dtype=torch.uint8, device="cuda")
                for name, dtype in DTYPES.items()}
    d_align = {name: torch.full((num_reads * (max_ops if name == "ops" else 1),), 0x5A5A5A5A, dtype=torch.int64 if np.dtype(dtype).itemsize == 8 else torch.int32, device="cuda")
               for name, dtype in dict(af.READ_OUTPUTS, ops=np.uint32).items()}
    d_counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    scratch = torch.zeros(g.align_chains_affine_scratch_bytes(rc.E2E_READ_LENGTH), dtype=torch.uint8, device="cuda")
    stream_obj.wait_stream(torch.cuda.current_stream())
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), n, total, d_positions.data_ptr(), s)
    g.local_positions(d_positions.data_ptr(), total, d_sequences.data_ptr(), d_positions.data_ptr(), stream=s)
    inputs = awfm.candidate_inputs(d_offsets.data_ptr(), n, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), total,
                                   d_positions.data_ptr(), d_sequences.data_ptr())
    cand = awfm.candidate_outputs(sequences=slot32["sequences"].data_ptr(), diagonals=slot64["diagonals"].data_ptr(),
                                  diagonalSpans=slot32["diagonalSpans"].data_ptr(), votes=slot32["votes"].data_ptr())
    g.read_candidates(inputs, num_reads, cand, d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=sc.E2E_BAND, min_votes=sc.E2E_MIN_VOTES,
                      max_candidates=slots, stream=s)
    chain_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    chains = awfm.chain_outputs(**{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    g.read_chains(inputs, num_reads, slot32["sequences"].data_ptr(), slot64["diagonals"].data_ptr(), slot32["diagonalSpans"].data_ptr(), chains,
                  d_scratch.data_ptr(), max_hits_per_seed=rc.E2E_MAX_HITS, band=sc.E2E_BAND, max_candidates=slots, gap_penalty=sc.E2E_GAP_PENALTY, stream=s)
    vin = awfm.verify_inputs(d_chars.data_ptr(), len(chars), d_read_offsets.data_ptr(), sequences=slot32["sequences"].data_ptr(),
                             **{name: (slot32.get(name) if name in slot32 else slot64[name]).data_ptr() for name in chain_names})
    sout = awfm.slot_score_outputs(numUnscored=d_counters.data_ptr(), numMapped=d_counters.data_ptr() + 8, **{name: a.data_ptr() for name, a in d_scores.items()})
    g.score_chains_affine(vin, num_reads, sout, max_candidates=slots, band_pad=vc.E2E_W, max_drift=vc.E2E_X, mapq_cap=sc.E2E_CAP, stream=s)
    aout = awfm.affine_outputs(numUnaligned=d_counters.data_ptr() + 16, numTruncated=d_counters.data_ptr() + 24, **{name: a.data_ptr() for name, a in d_align.items()})
    g.align_chains_affine(vin, d_scores["bestSlots"].data_ptr(), num_reads, aout, scratch.data_ptr(), max_candidates=slots, band_pad=vc.E2E_W,
                          max_drift=vc.E2E_X, max_ops=max_ops, max_rows=rc.E2E_READ_LENGTH, stream=s)
    stream_obj.synchronize()
    slot_arrays = {name: (slot32.get(name) if name in slot32 else slot64[name]).cpu().numpy().view(vc.SLOT_DTYPES[name]).reshape(num_reads, slots)
                   for name in vc.SLOT_FIELDS}
    case = sc.Case(chars.tobytes(), np.arange(num_reads + 1) * rc.E2E_READ_LENGTH, slot_arrays, np.zeros(num_reads, np.uint32), text.tobytes(), record_ends)
    got = {name: d_scores[name].cpu().numpy().view(dtype).reshape((num_reads, slots) if name in sc.SLOT_OUTPUTS else (num_reads,)) for name, dtype in DTYPES.items()}
    counters = [int(v) for v in d_counters.cpu().numpy()]
    got["numUnscored"], got["numMapped"] = counters[:2]
    sc.assert_equal(got, case.score(awfm, vc.E2E_W, vc.E2E_X, cap=sc.E2E_CAP))
    decoys_met, copies_met = sc.assert_planted_reads_mapped(case, got, planted, decoy_of, copies)
    assert decoys_met >= len(decoy_of) // 2 and copies_met >= 1
    aligned = d_align["scores"].cpu().numpy().view(np.uint32)
    mapped = got["bestSlots"] != sc.NO_SLOT
    assert np.array_equal(aligned[mapped], got["bestScores"][mapped]) and (aligned[~mapped] == sc.NONE).all() and counters[2:] == [0, 0]
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()
