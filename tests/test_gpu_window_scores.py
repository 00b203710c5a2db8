"""awfmGpuScoreWindowsAffine (include/awfm_gpu.h "window scores", csrc/awfm_window_affine_kernel.h) against its host twin
awfmScoreWindowsAffine, which tests/test_window_scores.py pins to the plain-Python restatement and to hand-computed values: every
output, bit for bit -- on the edge list at the natural number of columns per lane and with 4, 8 and 12 forced (4 and 8 send the
wider windows through column blocks), on read lengths and window widths around every edge of the layout, on windows that begin at
every offset mod 4 of the text, on texts of every length mod 16, with buffer and reads skewed, on one read of 4096 characters in
a window of 4096 and the refused neighbours, on batches of 2^12 reads in both alphabets, on more reads than the grid has waves,
from two streams at once, without a text, with bad arguments, and end to end from a FASTA file on mates the seeds cannot place.
Every output and the read buffer lie between guard words; the slot arrays hold the guard pattern before the call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import window_scores_common as ws  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, Image, _upload  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = dict(ws.READ_OUTPUTS, **ws.SLOT_OUTPUTS)
NAMES = list(ws.READ_OUTPUTS) + list(vc.SLOT_FIELDS) + list(ws.COUNTERS)
TIERS = [None, 4, 8, 12]


def size_of(name, n, stride):
    if name in ws.COUNTERS:
        return 8
    return np.dtype(DTYPES[name]).itemsize * n * (stride if name in ws.SLOT_OUTPUTS else 1)


def pattern_slots(n, stride):
    """what the slot arrays hold before a call, on both sides: the guard pattern"""
    return {name: np.frombuffer(bytes([PATTERN]) * (np.dtype(d).itemsize * n * stride), d).reshape(n, stride) for name, d in ws.SLOT_OUTPUTS.items()}


class DeviceCall:
    """the arrays of one case on the device -- the read buffer `skew` bytes into its allocation, between guard words -- and
    guarded outputs for calls on them"""

    def __init__(self, awfm, torch, case, skew=0):
        self.awfm, self.torch, self.case = awfm, torch, case
        chars = np.concatenate((np.full(GUARD + skew, PATTERN, np.uint8), case.read_chars, np.full(GUARD, PATTERN, np.uint8)))
        self.chars = torch.from_numpy(chars).to("cuda")
        self.arrays = [_upload(torch, a) for a in (case.offsets, case.sequences, case.begins, case.window_ends)]
        self.inputs = awfm.window_inputs(self.chars.data_ptr() + GUARD + skew, case.num_read_chars, *(a.data_ptr() for a in self.arrays))

    def run(self, g, scoring=ws.DEFAULT, min_score=0, stride=1, column=0, max_length=512, outputs=None, stream=0, unscored_before=0,
            found_before=0, launch=True):
        torch, n = self.torch, self.case.num_reads
        outputs = NAMES if outputs is None else list(outputs)
        buffers = {name: torch.full((size_of(name, n, stride) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in outputs}
        for name, before in (("numUnscored", unscored_before), ("numFound", found_before)):
            if name in outputs:
                buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        wout = self.awfm.window_score_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        scratch = torch.empty(max(g.score_windows_affine_scratch_bytes(max_length), 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def enqueue():
            g.score_windows_affine(self.inputs, n, wout, scratch.data_ptr(), max_length, scoring=scoring, min_score=min_score, slot_stride=stride,
                                   slot_column=column, stream=stream)

        def collect():
            result, _ = {}, scratch  # (the scratch lives until the results are collected)
            for name, b in buffers.items():
                raw, size = b.cpu().numpy(), size_of(name, n, stride)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size]
                if name in ws.COUNTERS:
                    result[name] = int(body.view(np.uint64)[0])
                else:
                    result[name] = body.view(DTYPES[name]).reshape((n, stride) if name in ws.SLOT_OUTPUTS else (n,))
            return result

        if launch:
            enqueue()
        return (None if launch else enqueue), collect

    def __call__(self, g, **kw):
        _, collect = self.run(g, **kw)
        self.torch.cuda.synchronize()
        return collect()


def twin(awfm, case, stride=1, **kw):
    return case.host(awfm, stride=stride, slots=pattern_slots(case.num_reads, stride), threads=16, **kw)


@pytest.mark.parametrize("q", TIERS, ids=["natural", "4", "8", "12"])
def test_edge_list_equals_the_host_twin_and_the_hand_computed_values(awfm, require_gpu, diag, q):
    import torch
    diag(window_q=q)
    b = ws.edge_builder()
    case = b.case()
    image = Image(awfm, case)
    try:
        call = DeviceCall(awfm, torch, case)
        for min_score in (0, 12, 13):
            want = twin(awfm, case, min_score=min_score, unscored_before=9, found_before=2)
            got = call(image.g, min_score=min_score, unscored_before=9, found_before=2)
            ws.assert_equal(got, want, what=f"minScore={min_score}")
            if min_score == 0:
                b.check(got)
        for stride, column in ((4, 0), (4, 3), (16, 7), (16, 15)):
            ws.assert_equal(call(image.g, stride=stride, column=column), twin(awfm, case, stride, column=column), what=f"{stride} {column}")
        want = twin(awfm, case)
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            ws.assert_equal(DeviceCall(awfm, torch, case, skew=skew)(image.g), want, what=f"buffer skewed by {skew}")
            ws.assert_equal(DeviceCall(awfm, torch, b.case(skew))(image.g), want, what=f"reads skewed by {skew}")
        for scoring in ws.SCORINGS[1:]:
            ws.assert_equal(call(image.g, scoring=scoring), twin(awfm, case, scoring=scoring), what=str(scoring))
        for missing in NAMES:  # every output NULL in turn, and alone
            for outputs in ([n for n in NAMES if n != missing], [missing]):
                got = call(image.g, outputs=outputs)
                assert sorted(got) == sorted(outputs)
                ws.assert_equal(got, want, names=outputs, what=str(outputs))
    finally:
        image.close()
    ties = ws.tie_builder()  # the two ties of the origin rule, hand-computed
    image = Image(awfm, ties.case())
    try:
        got = DeviceCall(awfm, torch, ties.case())(image.g, scoring=ws.TIE_SCORING)
        ties.check(got)
        ws.assert_equal(got, twin(awfm, ties.case(), scoring=ws.TIE_SCORING))
    finally:
        image.close()


def shapes_case(seed=3):
    """every read length of the list against every window width of the list, the windows beginning at every offset mod 4 of the
    text, the reads planted with a few edits where they fit"""
    rng = np.random.default_rng(seed)
    letters = ws.letters_of(ws.DNA)
    record = bytes(rng.choice(letters, 2400))
    text, ends = ws.text_of([b"acg", record])
    reads, windows = [], []
    widths = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1024, 1025]
    for k, n in enumerate([0, 1, 2, 63, 64, 65, 127, 128, 129, 300]):
        for j, W in enumerate(widths):
            begin = 100 + (k + j) % 4 + 4 * j
            at = begin + int(rng.integers(0, max(W - n, 0) + 1))
            read = bytes(vc.edit(rng, record[at:at + n], 0.06, letters))[:n] if n else b""
            reads.append(read)
            windows.append((1, begin, begin + W))
    return ws.Case(reads, windows, text, ends)


@pytest.mark.parametrize("q", TIERS, ids=["natural", "4", "8", "12"])
def test_read_lengths_and_window_widths_around_every_edge_of_the_layout(awfm, require_gpu, diag, q):
    """n in 0, 1, 2, 63..65, 127..129, 300 by W in 0, 1, 3..5, 63..65, 255..257 and each tier's last width and one more (256 | 257,
    512 | 513, 768 | 769: beyond 768, and beyond 64 Q with Q forced, the window goes in column blocks), at every text offset mod 4"""
    import torch
    diag(window_q=q)
    case = shapes_case()
    image = Image(awfm, case)
    try:
        for scoring in (ws.DEFAULT, (2, 4, 4, 2)):
            want = twin(awfm, case, scoring=scoring)
            assert want["numUnscored"] == 0 and want["numFound"] > 150
            ws.assert_equal(DeviceCall(awfm, torch, case)(image.g, scoring=scoring, max_length=300), want, what=str(scoring))
        ws.assert_equal(DeviceCall(awfm, torch, case, skew=3)(image.g), twin(awfm, case), what="skewed")
    finally:
        image.close()


def test_texts_of_every_length_mod_16_scored_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        case = ws.wide_case(40, length - 45)  # "acgt", NUL, a record of length - 5 without its terminator
        case.text = case.text[:-1]
        case.window_ends[0] = 1 << 50
        case.begins[0] = length % 5
        assert case.text.size == length
        image = Image(awfm, case)
        try:
            got = DeviceCall(awfm, torch, case)(image.g)
            ws.assert_equal(got, twin(awfm, case), what=f"length {length}")
            assert int(got["textEnds"][0]) <= length - 5 and int(got["scores"][0]) >= 30
        finally:
            image.close()


@pytest.mark.parametrize("q", [None, 4], ids=["natural", "4"])
def test_a_read_of_4096_characters_in_a_window_of_4096_and_the_refused_neighbours(awfm, require_gpu, diag, q):
    import torch
    diag(window_q=q)
    case = ws.wide_case(4096, 4096)
    image = Image(awfm, case)
    try:
        want = twin(awfm, case)
        assert int(want["scores"][0]) > 3000
        ws.assert_equal(DeviceCall(awfm, torch, case)(image.g, max_length=4096), want)
        for n, W, value in ((4097, 4096, ws.TOO_LONG), (4096, 4097, ws.TOO_WIDE), (4097, 4097, ws.TOO_WIDE)):
            other = ws.wide_case(n, W)
            other.text, other.ends = case.text, case.ends  # (the image's text: a refused read reads none of it)
            got = DeviceCall(awfm, torch, other)(image.g, max_length=4096)
            ws.assert_equal(got, twin(awfm, other))
            assert int(got["scores"][0]) == value and got["numUnscored"] == 1
        # the device's own rule: a read longer than the scratch was sized for
        short = ws.wide_case(300, 600)
        short.text, short.ends = case.text, case.ends
        got = DeviceCall(awfm, torch, short)(image.g, max_length=299)
        ws.assert_equal(got, short.expected(slots=pattern_slots(1, 1), max_length=299))
        assert int(got["scores"][0]) == ws.TOO_LONG
        ws.assert_equal(DeviceCall(awfm, torch, short)(image.g, max_length=300), twin(awfm, short))
    finally:
        image.close()


@pytest.mark.parametrize("alphabet", [ws.DNA, ws.AMINO], ids=["dna", "amino"])
def test_batches_of_4096_reads(awfm, require_gpu, alphabet):
    """lengths 1..300 before their edits (insertions lengthen a read: the scratch is sized for 400), windows 0..1200, a tenth not looked at, some malformed, a tenth clipped, a text of 2^16 positions in 37
    records, under two scorings"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    case = ws.random_case(20, 1 << 12, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, max_window=1200)
    image = Image(awfm, case)
    try:
        call = DeviceCall(awfm, torch, case)
        for scoring, stride, column in ((ws.DEFAULT, 4, 1), ((2, 4, 4, 2), 1, 0)):
            want = twin(awfm, case, stride, scoring=scoring, min_score=10, column=column, unscored_before=3, found_before=1)
            s = want["scores"]
            assert 0.05 < (s == ws.NONE).mean() < 0.2 and (s == ws.MALFORMED).sum() > 50 and want["numFound"] > 2000
            got = call(image.g, scoring=scoring, min_score=10, stride=stride, column=column, max_length=400, unscored_before=3, found_before=1)
            ws.assert_equal(got, want, what=str(scoring))
    finally:
        image.close()


def test_more_reads_than_the_grid_has_waves(awfm, require_gpu):
    """2^13 reads of 100..200 characters in windows of up to 400: more than the waves of the largest persistent grid"""
    import torch
    rng = np.random.default_rng(43)
    case = ws.random_case(19, 1 << 13, text_length=1 << 16, num_records=37, lengths=rng.integers(100, 201, 1 << 13), max_window=400, max_rate=0.06)
    image = Image(awfm, case)
    try:
        assert 0 < image.g.score_windows_affine_scratch_bytes(256) // (2 * 16 * 256) < 1 << 13  # the grid's waves: fewer than reads
        ws.assert_equal(DeviceCall(awfm, torch, case)(image.g, max_length=256), twin(awfm, case))
    finally:
        image.close()


def test_two_streams_without_a_text_and_bad_arguments(awfm, require_gpu, diag):
    import torch
    diag(window_q=4)  # column blocks: each stream's own scratch is in use
    a, b = shapes_case(5), shapes_case(6)
    b = ws.Case(b.reads, list(zip(b.sequences, b.begins, b.window_ends)), a.text, a.ends)  # (other reads, on the image's text)
    image = Image(awfm, a)
    try:
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        calls = [DeviceCall(awfm, torch, a), DeviceCall(awfm, torch, b)]
        collects = [call.run(image.g, stream=s.cuda_stream, max_length=300)[1] for call, s in zip(calls, streams)]
        torch.cuda.synchronize()
        ws.assert_equal(collects[0](), twin(awfm, a), what="first stream")
        ws.assert_equal(collects[1](), twin(awfm, b), what="second stream")
        # every bad argument: nothing is launched, the outputs keep the pattern
        call = calls[0]
        for kw, rc in ((dict(stride=0), awfm.AwFmIllegalPositionError), (dict(stride=17), awfm.AwFmIllegalPositionError),
                       (dict(stride=4, column=4), awfm.AwFmIllegalPositionError), (dict(max_length=0), awfm.AwFmIllegalPositionError),
                       (dict(max_length=4097), awfm.AwFmIllegalPositionError), (dict(scoring=(0, 4, 6, 1)), awfm.AwFmIllegalPositionError),
                       (dict(scoring=(1, 4, 6, 256)), awfm.AwFmIllegalPositionError), (dict(scoring=None), -4)):
            enqueue, collect = call.run(image.g, launch=False, **kw)
            with pytest.raises(awfm.AwFmError) as e:
                enqueue()
            assert e.value.rc == rc, kw
            torch.cuda.synchronize()
            got = collect()
            assert all((np.asarray(got[name]).view(np.uint8) == PATTERN).all() for name in ws.READ_OUTPUTS), kw
        # NULL structs, each required array NULL, a read buffer that is NULL but not empty, a scratch off its 16 bytes, 2^32 reads
        import ctypes as C
        lib, costs = awfm._lib.lib(), awfm.align_scoring()
        d_scores = torch.full((4 * a.num_reads,), PATTERN, dtype=torch.uint8, device="cuda")
        guarded = awfm.window_score_outputs(scores=d_scores.data_ptr())
        d_scratch = torch.empty(image.g.score_windows_affine_scratch_bytes(300) + 32, dtype=torch.uint8, device="cuda")
        aligned = d_scratch.data_ptr() + (-d_scratch.data_ptr()) % 16
        chars, pointers = call.chars.data_ptr() + GUARD, [t.data_ptr() for t in call.arrays]
        good = awfm.window_inputs(chars, a.num_read_chars, *pointers)

        def raw(inputs, n, outputs, scratch):
            return lib.awfmGpuScoreWindowsAffine(image.g.handle, None if inputs is None else C.byref(inputs), n, C.byref(costs), 0, 1, 0, 300,
                                                 None if outputs is None else C.byref(outputs), scratch, None)

        assert raw(good, a.num_reads, guarded, aligned) == awfm.AwFmSuccess  # (the arguments the refused calls differ from)
        torch.cuda.synchronize()
        assert not (d_scores.cpu().numpy() == PATTERN).all()
        d_scores.fill_(PATTERN)
        torch.cuda.synchronize()
        assert raw(None, a.num_reads, guarded, aligned) == -4 and raw(good, a.num_reads, None, aligned) == -4  # AwFmNullPtrError
        for k in range(4):
            missing = awfm.window_inputs(chars, a.num_read_chars, *[0 if j == k else v for j, v in enumerate(pointers)])
            assert raw(missing, a.num_reads, guarded, aligned) == -4, k
        assert raw(awfm.window_inputs(0, a.num_read_chars, *pointers), a.num_reads, guarded, aligned) == -4
        for off in (1, 4, 8):
            assert raw(good, a.num_reads, guarded, aligned + off) == awfm.AwFmIllegalPositionError, off
        assert raw(good, 1 << 32, guarded, aligned) == awfm.AwFmIllegalPositionError
        torch.cuda.synchronize()
        assert (d_scores.cpu().numpy() == PATTERN).all()  # nothing was launched
        out = awfm.window_score_outputs()
        with pytest.raises(awfm.AwFmError) as e:  # no scratch
            image.g.score_windows_affine(call.inputs, a.num_reads, out, 0, 300)
        assert e.value.rc == -4  # AwFmNullPtrError
        assert image.g.score_windows_affine_scratch_bytes(0) == 0 and image.g.score_windows_affine_scratch_bytes(4097) == 0
        image.g.score_windows_affine(call.inputs, 0, out, 0, 0, slot_stride=99)  # numReads == 0 touches nothing
    finally:
        image.close()
    bare = awfm.create_index(a.text, awfm.AwFmAlphabetDna, 2, 2)
    g = awfm.GpuIndex(bare)
    try:
        enqueue, _ = DeviceCall(awfm, torch, a).run(g, launch=False, max_length=300)
        with pytest.raises(awfm.AwFmError) as e:
            enqueue()
        assert e.value.rc == awfm.AwFmUnsupportedVersionError
    finally:
        g.destroy()
        bare.dealloc()


def test_end_to_end_from_a_fasta_file(awfm, require_gpu, tmp_path):
    """pairs planted on one strand of a FASTA file's records: mate 1 is an exact copy and is placed by the index (located, mapped
    to its record); mate 2, 150 positions behind it, carries a substitution at every 11th character, so no 20-mer of it occurs
    and the seeds give it nothing -- asserted: the longest match ending at every 4th position of every mate 2 is below 20.  The
    new call on the window [mate 1's position, + 400) of mate 1's record finds EVERY mate 2 at its planted interval, equals the
    host twin, and affine alignment (w = 8, x = 15) on the slots it wrote returns the same scores, begins and ends."""
    import torch
    import local_positions_common as lp
    import read_candidates_common as rc
    letters = np.frombuffer(b"acgt", np.uint8)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), [5000, 0, 7001, 3], letters, 12)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    g = awfm.GpuIndex(ix)
    try:
        text, record_ends = vc.text_of(records)
        g.set_text(text)
        assert g.num_records == len(records)
        rng = np.random.default_rng(13)
        pairs, length, width, swap = 96, 100, 400, {ord("a"): ord("c"), ord("c"): ord("g"), ord("g"): ord("t"), ord("t"): ord("a")}
        mates1, mates2, planted = [], [], []
        for _ in range(pairs):
            s = int(rng.choice([0, 2]))
            p = int(rng.integers(0, len(records[s]) - 260))
            mates1.append(records[s][p:p + length])
            mate = bytearray(records[s][p + 150:p + 150 + length])
            for k in range(5, length, 11):
                mate[k] = swap[mate[k]]
            mates2.append(bytes(mate))
            planted.append((s, p))
        # the seeds cannot place mate 2
        chars, starts, ends, _, _ = rc.windows_of(mates2)
        d_chars, d_starts, d_ends = [_upload(torch, a) for a in (chars, starts, ends)]
        d_lengths = torch.zeros(len(starts), dtype=torch.int32, device="cuda")
        d_counts = torch.zeros(len(starts), dtype=torch.int32, device="cuda")
        g.longest_suffix_matches(d_chars.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, len(starts), 20, d_lengths.data_ptr(), 0,
                                 d_counts.data_ptr())
        torch.cuda.synchronize()
        assert int(d_counts.sum()) == 0 and int(d_lengths.max()) < 20
        # mate 1 by the index: one hit each, mapped to its record
        _, hit_offsets, sequences, positions, illegal = g.locate_host_local(np.frombuffer(b"".join(mates1), np.uint8), fixed_length=length)
        assert illegal == 0 and np.array_equal(np.diff(hit_offsets.astype(np.int64)), np.ones(pairs, np.int64))
        assert [(int(s), int(p)) for s, p in zip(sequences, positions)] == planted
        # mate 2 by the new call in mate 1's window
        case = ws.Case(mates2, [(int(s), int(p), int(p) + width) for s, p in zip(sequences, positions)], text, record_ends)
        call = DeviceCall(awfm, torch, case)
        got = call(g, min_score=30, max_length=length)
        ws.assert_equal(got, twin(awfm, case, min_score=30))
        assert got["numFound"] == pairs and got["numUnscored"] == 0
        for r, (s, p) in enumerate(planted):
            assert int(got["sequences"][r, 0]) == s and int(got["readBegins"][r]) <= 5 and int(got["readEnds"][r]) >= length - 6, r
            assert int(got["textBegins"][r]) == p + 150 + int(got["readBegins"][r]) and int(got["textEnds"][r]) == p + 150 + int(got["readEnds"][r]), r
        # affine alignment on the written slots, on the device
        d_slots = {name: _upload(torch, got[name]) for name in vc.SLOT_FIELDS}
        vin = awfm.verify_inputs(call.chars.data_ptr() + GUARD, case.num_read_chars, call.arrays[0].data_ptr(), **{name: a.data_ptr() for name, a in d_slots.items()})
        d_align = {name: torch.zeros(pairs, dtype=torch.int64 if np.dtype(dtype).itemsize == 8 else torch.int32, device="cuda")
                   for name, dtype in af.READ_OUTPUTS.items()}
        d_chosen = torch.zeros(pairs, dtype=torch.int32, device="cuda")
        scratch = torch.zeros(g.align_chains_affine_scratch_bytes(length), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.align_chains_affine(vin, d_chosen.data_ptr(), pairs, awfm.affine_outputs(**{name: a.data_ptr() for name, a in d_align.items()}),
                              scratch.data_ptr(), max_candidates=1, band_pad=8, max_drift=15, max_ops=32, max_rows=length)
        torch.cuda.synchronize()
        for name in ("scores", "readBegins", "readEnds", "textBegins", "textEnds"):
            assert np.array_equal(d_align[name].cpu().numpy().view(ws.READ_OUTPUTS[name]), got[name]), name
    finally:
        g.destroy()
        ix.dealloc()
