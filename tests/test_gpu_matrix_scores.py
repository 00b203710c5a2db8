"""awfmGpuScoreChainsMatrix and awfmGpuAlignChainsMatrix (include/awfm_gpu.h "substitution matrices", csrc/awfm_matrix_kernel.h)
against their host twins awfmScoreChainsMatrix and awfmAlignChainsMatrix, which tests/test_matrix_scores.py pins to the plain-Python
restatement, to hand-computed values and to the affine calls: every output, bit for bit, except the rows of ops of truncated reads
-- on the hand-computed cases and the edge lists at the natural number of lanes and with 32 and 64 forced, with the read buffer
skewed, with every output NULL in turn and alone, with maxOps and maxRows at their edges, on reads of every length around the
chunk edges at every band shape under the adversarial matrices, over all 256 byte values on either side, on 2^12 random reads
per alphabet under matrices over the full int8 range and over -4..11, on more reads than the grid has waves, on texts of every
length mod 16, under the uniform matrix against the affine device calls, on one read of 2^16 letters worth 127 each, from two
streams with two matrices at once, with the caller's struct overwritten as soon as the call has returned, and without a text.
Inputs, outputs and the scratch (exactly its declared size) lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import matrix_scores_common as mx  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import test_gpu_align_affine as gaf  # noqa: E402
import test_gpu_score_chains as gsc  # noqa: E402
from test_gpu_byte_values import Image  # noqa: E402  (an index of a well-formed text, the case's own text installed)
from test_gpu_verify_chains import PATTERN  # noqa: E402

pytestmark = pytest.mark.gpu
Scratch, longest_read = gaf.Scratch, gaf.longest_read


class MatrixCalls:
    """a GpuIndex whose two affine calls are the matrix calls: the guarded device calls of the affine tests run them unchanged.
    `scoring` is a mx.Matrix, or a struct AwFmMatrixScoring that is passed as it is"""

    def __init__(self, awfm, g):
        self.awfm, self.g = awfm, g

    def _struct(self, scoring):
        return scoring.struct(self.awfm) if isinstance(scoring, mx.Matrix) else scoring

    def align_chains_affine(self, *args, scoring=None, **kw):
        return self.g.align_chains_matrix(*args, scoring=self._struct(scoring), **kw)

    def score_chains_affine(self, *args, scoring=None, **kw):
        return self.g.score_chains_matrix(*args, scoring=self._struct(scoring), **kw)

    def __getattr__(self, name):
        return getattr(self.g, name)


class Device:
    """an image of a case's text and the two guarded calls on cases that share it"""

    def __init__(self, awfm, torch, case):
        self.awfm, self.torch, self.image = awfm, torch, Image(awfm, case)
        self.g = MatrixCalls(awfm, self.image.g)

    def align(self, case, w, x, matrix, scratch=None, skew=0, **kw):
        scratch = scratch or Scratch(self.torch, self.image.g, max(longest_read(case), 1))
        return gaf.DeviceCall(self.awfm, self.torch, case, skew=skew)(self.g, w, x, scratch, scoring=matrix, **kw)

    def score(self, case, w, x, matrix, skew=0, **kw):
        return gsc.DeviceCall(self.awfm, self.torch, case, skew=skew)(self.g, w, x, scoring=matrix, **kw)

    def both_equal_the_twins(self, case, w, x, matrix, what="", max_ops=16, threads=4, **kw):
        got = self.align(case, w, x, matrix, max_ops=max_ops, **kw)
        af.assert_equal(got, case.host(self.awfm, w, x, matrix, max_ops=max_ops, threads=threads), what=f"align {what} {matrix}", fill=PATTERN)
        sc.assert_equal(self.score(case, w, x, matrix, min_score=2, cap=254), case.score(self.awfm, w, x, matrix, min_score=2, cap=254, threads=threads),
                        what=f"score {what} {matrix}")
        return got

    def close(self):
        self.image.close()


@pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
def test_hand_computed_cases_and_edge_lists_equal_the_host_twins(awfm, require_gpu, diag, group):
    import torch
    diag(affine_group=group, score_group=group)
    for matrix, b in mx.hand_builders():
        case = b.case()
        device = Device(awfm, torch, case)
        try:
            b.check(device.both_equal_the_twins(case, 0, 0, matrix, "by hand", max_ops=8), 8)
        finally:
            device.close()
    builders = {(w, x): af.edge_builder(w, x) for w, x in ((2, 3), (8, 15), (3, 4), (24, 15))}  # 8, 32, 11 and 64 diagonals
    device = Device(awfm, torch, builders[2, 3].case())
    try:
        scratch = Scratch(torch, device.image.g, 64)
        for (w, x), b in builders.items():
            case = mx.as_matrix(b.case())
            b.check(device.both_equal_the_twins(case, w, x, mx.uniform(af.DNA, af.DEFAULT), f"w={w} x={x}", max_ops=8, scratch=scratch), 8)
            for matrix in mx.ADVERSARIAL:
                device.both_equal_the_twins(case, w, x, matrix, f"w={w} x={x}", max_ops=8, scratch=scratch)
        outside = mx.as_matrix(af.outside_builder().case())
        device.both_equal_the_twins(outside, 0, 0, mx.TRANSITIONS, "outside", scratch=scratch)
        if group is not None:
            return
        b, matrix = builders[2, 3], mx.TRANSITIONS
        case = mx.as_matrix(b.case())
        want, want_scores = case.host(awfm, 2, 3, matrix, max_ops=8), case.score(awfm, 2, 3, matrix)
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            skewed = mx.as_matrix(b.case(skew))
            af.assert_equal(device.align(case, 2, 3, matrix, scratch, skew=skew, max_ops=8), want, what=f"buffer skewed by {skew}")
            af.assert_equal(device.align(skewed, 2, 3, matrix, scratch, max_ops=8), want, what=f"reads skewed by {skew}")
            sc.assert_equal(device.score(case, 2, 3, matrix, skew=skew), want_scores, what=f"buffer skewed by {skew}")
            sc.assert_equal(device.score(skewed, 2, 3, matrix), want_scores, what=f"reads skewed by {skew}")
        most = int(want["numOps"].max())
        for max_ops in (most, most - 1):  # exactly the most runs of a read, and one less
            want_ops = case.host(awfm, 2, 3, matrix, max_ops=max_ops)
            assert (want_ops["numTruncated"] > 0) == (max_ops < most)
            af.assert_equal(device.align(case, 2, 3, matrix, scratch, max_ops=max_ops), want_ops, what=f"{max_ops} runs", fill=PATTERN)
        for names, call, equal, wanted in ((list(gaf.SIZES), lambda o: device.align(case, 2, 3, matrix, scratch, max_ops=8, outputs=o), af.assert_equal, want),
                                           (list(gsc.SIZES), lambda o: device.score(case, 2, 3, matrix, outputs=o), sc.assert_equal, want_scores)):
            for missing in names:  # every output NULL in turn, and alone
                for outputs in ([n for n in names if n != missing], [missing]):
                    got = call(outputs)
                    assert sorted(got) == sorted(outputs)
                    equal(got, wanted, names=outputs, what=str(outputs))
        longest = longest_read(case)
        for max_rows in (longest, longest - 1):  # maxRows at the longest read's length and one less: the rule of the device side, restated
            want_rows = case.expected(2, 3, matrix, max_ops=8, max_rows=max_rows)
            assert ((want_rows["scores"] == af.TOO_LONG).sum() > 0) == (max_rows < longest)
            af.assert_equal(device.align(case, 2, 3, matrix, Scratch(torch, device.image.g, max_rows), max_ops=8), want_rows, what=f"maxRows {max_rows}", fill=PATTERN)
    finally:
        device.close()


def lengths_builder(seed=3):
    """reads of 1 .. 5, 63, 64, 65 and 127 .. 130 characters cut from a record of 700, each with a substitution, a deleted and an
    inserted character where it is long enough, on the diagonal of its first character"""
    rng = np.random.default_rng(seed)
    record = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 700))
    b = mx.Builder([record, b"acgtacgt"])
    for k, n in enumerate((1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 130)):
        at = 40 + 31 * k
        read = bytearray(record[at:at + n])
        if n >= 63:
            read[n // 2] = ord("n")
            del read[n // 3]
            read.insert(2 * n // 3, ord("a"))
        b.add(f"n = {n}", bytes(read), 0, at, at, None)
    return b


def test_read_lengths_around_the_chunk_edges_at_every_band_shape_under_the_adversarial_matrices(awfm, require_gpu):
    import torch
    b = lengths_builder()
    device = Device(awfm, torch, b.case())
    try:
        scratch = Scratch(torch, device.image.g, 130)
        for width, (w, x) in sorted(af.BAND_SHAPES.items()):
            for k, matrix in enumerate(mx.ADVERSARIAL + (mx.random_matrix(width, -128, 127),)):
                skew = (width + k) % 4
                device.both_equal_the_twins(b.case(skew), w, x, matrix, f"width {width} skew {skew}", max_ops=24, scratch=scratch, skew=(4 - skew) % 4)
    finally:
        device.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_all_256_byte_values_on_either_side(awfm, require_gpu, alphabet):
    import torch
    case, x, y = mx.byte_pairs_case(alphabet)
    classes = mx.classes_of_all_bytes(alphabet)
    device = Device(awfm, torch, case)
    try:
        scratch = Scratch(torch, device.image.g, 1)
        for matrix, want in zip(mx.telling_matrices(), (1 + classes[x], 1 + classes[y])):
            got = device.align(case, 0, 0, matrix, scratch, max_ops=2)
            assert np.array_equal(got["scores"], want), matrix
            af.assert_equal(got, case.host(awfm, 0, 0, matrix, max_ops=2, threads=8), what=repr(matrix), fill=PATTERN)
            sc.assert_equal(device.score(case, 0, 0, matrix), case.score(awfm, 0, 0, matrix, threads=8), what=repr(matrix))
    finally:
        device.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_batch_of_4096_reads_under_full_range_and_small_matrices(awfm, require_gpu, alphabet):
    """lengths 1..300 with the chunk edges among them, edits of 0..12 %, a tenth of the slots unused, some malformed, a tenth
    hanging over a record end, a text of 2^16 positions in 37 records, four slots a read"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    lengths[:12] = [63, 64, 65, 127, 128, 129, 1, 300, 63, 64, 65, 2]
    case = mx.random_case(20, 1 << 12, 4, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, hanging=0.1, other=0.005)
    device = Device(awfm, torch, case)
    try:
        scratch = Scratch(torch, device.image.g, longest_read(case))
        gaps = (11, 1) if alphabet == af.AMINO else (6, 1)
        for matrix, (w, x) in ((mx.random_matrix(1, -128, 127, *gaps), (8, 15)), (mx.random_matrix(2, -4, 11, *gaps), (8, 15)), (mx.random_matrix(3, -4, 11, *gaps), (20, 23))):
            got = device.both_equal_the_twins(case, w, x, matrix, f"w={w}", max_ops=64, threads=16, scratch=scratch)
            assert ((got["scores"] > 0) & (got["scores"] < af.TOO_LONG)).sum() > 2000 and (got["scores"] == af.MALFORMED).sum() > 50
    finally:
        device.close()


def test_more_reads_than_the_grid_has_waves(awfm, require_gpu, diag):
    """4100 reads of 200..600 characters with 64 lanes each under the alignment call -- more than the 4096 waves of the largest
    grid --, and 2^15 reads of one slot under the scoring call, more than its grid's waves (256 CUs x 7 workgroups x 4)"""
    import torch
    diag(affine_group=64)
    rng = np.random.default_rng(43)
    matrix = mx.random_matrix(4, -4, 11)
    case = mx.random_case(19, 4100, 1, text_length=1 << 16, num_records=37, lengths=rng.integers(200, 601, 4100), max_rate=0.06)
    many = mx.random_case(21, 1 << 15, 1, text_length=1 << 16, num_records=37, max_length=40)
    many.text, many.ends = case.text, case.ends
    device = Device(awfm, torch, case)
    try:
        af.assert_equal(device.align(case, 8, 15, matrix, max_ops=64), case.host(awfm, 8, 15, matrix, max_ops=64, threads=16), fill=PATTERN)
        sc.assert_equal(device.score(many, 8, 15, matrix), many.score(awfm, 8, 15, matrix, threads=16))
    finally:
        device.close()


def test_texts_of_every_length_mod_16_aligned_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        b = af.tail_case(length)
        case = mx.as_matrix(b.case())
        device = Device(awfm, torch, case)
        try:
            b.check(device.both_equal_the_twins(case, 2, 3, mx.uniform(af.DNA, af.DEFAULT), f"length {length}", max_ops=32), 32)
            device.both_equal_the_twins(case, 2, 3, mx.TRANSITIONS, f"length {length}", max_ops=32)
        finally:
            device.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_the_uniform_matrix_gives_what_the_affine_device_calls_give(awfm, require_gpu, alphabet):
    import torch
    case = mx.random_case(31, 1500, 4, alphabet, text_length=1 << 14, max_length=150, hanging=0.2)
    affine = case.affine()
    device = Device(awfm, torch, case)
    try:
        scratch = Scratch(torch, device.image.g, longest_read(case))
        for scoring, (w, x) in zip([s for s in af.SCORINGS if s[0] <= 127 and s[1] <= 128], ((8, 15), (2, 3), (20, 23), (3, 4))):
            made = awfm.matrix_scoring_uniform(alphabet, scoring)
            got = gaf.DeviceCall(awfm, torch, case)(device.g, w, x, scratch, scoring=made, max_ops=24)
            want = gaf.DeviceCall(awfm, torch, affine)(device.image.g, w, x, scratch, scoring=scoring, max_ops=24)
            af.assert_equal(got, want, what=str(scoring), fill=PATTERN)
            af.assert_equal(got, affine.host(awfm, w, x, scoring, max_ops=24, threads=8), what=f"host {scoring}", fill=PATTERN)
            sc.assert_equal(gsc.DeviceCall(awfm, torch, case)(device.g, w, x, scoring=made, min_score=3), gsc.DeviceCall(awfm, torch, affine)(device.image.g, w, x, scoring=scoring, min_score=3), what=str(scoring))
    finally:
        device.close()


def test_one_read_of_two_to_the_sixteen_letters_worth_127_each(awfm, require_gpu):
    """the end cell's key at its top: the score is 65536 x 127, the end cell (2^16, 2^16); and one letter more is too long"""
    import torch
    n = af.MAX_LENGTH
    letters = np.random.default_rng(8).choice(np.frombuffer(b"acgt", np.uint8), n + 1)
    slots = {name: np.array([[0] * 3, [0] * 3], vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    slots["chainAnchors"][:] = 1
    slots["chainReadEnds"][:, 0] = (n, n + 1)
    slots["chainBeginDiagonals"][:, 2] = slots["chainEndDiagonals"][:, 2] = 1  # a third slot one diagonal off, whose band holds the same cells
    slots["sequences"][:, 1] = vc.NONE
    case = mx.Case(letters[:n].tobytes() + letters.tobytes(), [0, n, 2 * n + 1], slots, [0, 0], letters.tobytes() + b"\0", [n + 1])
    matrix = mx.Matrix(np.where(np.eye(21, dtype=bool), 127, -128), 255, 255, "127 / -128")
    device = Device(awfm, torch, case)
    try:
        got = device.score(case, 8, 15, matrix, cap=254)
        assert got["slotScores"][0].tolist()[:2] == [n * 127, sc.NONE] and got["slotScores"][1].tolist()[:2] == [sc.TOO_LONG, sc.NONE]
        assert int(got["slotReadEnds"][0, 0]) == n and int(got["slotTextEnds"][0, 0]) == n and got["bestScores"].tolist() == [n * 127, 0]
        sc.assert_equal(got, case.score(awfm, 8, 15, matrix, cap=254, threads=2))
    finally:
        device.close()


def test_two_streams_two_matrices_an_overwritten_struct_and_an_image_without_a_text(awfm, require_gpu):
    import torch
    a, b = mx.random_case(5, 600, 4, max_length=200, hanging=0.1), mx.random_case(6, 500, 3, max_length=120, hanging=0.1)
    b.text, b.ends = a.text, a.ends
    device = Device(awfm, torch, a)
    try:
        g, raw = device.g, device.image.g
        matrices = [mx.random_matrix(11, -128, 127), mx.random_matrix(12, -4, 11, 11, 1)]
        params = [(8, 15), (2, 3)]
        scratches = [Scratch(torch, raw, longest_read(a)), Scratch(torch, raw, longest_read(b))]
        want = [c.host(awfm, w, x, m) for c, (w, x), m in zip((a, b), params, matrices)]
        want_scores = [c.score(awfm, w, x, m) for c, (w, x), m in zip((a, b), params, matrices)]
        aligns, scores = [gaf.DeviceCall(awfm, torch, c) for c in (a, b)], [gsc.DeviceCall(awfm, torch, c) for c in (a, b)]
        args = (aligns[0].inputs, aligns[0].chosen.data_ptr(), a.num_reads, awfm.affine_outputs(), scratches[0].address)
        struct = matrices[0].struct(awfm)
        raw.set_text(None)
        for call in (lambda: raw.align_chains_matrix(*args, scoring=struct, max_candidates=4, max_rows=scratches[0].max_rows),
                     lambda: raw.score_chains_matrix(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=struct)):
            with pytest.raises(awfm.AwFmError) as e:
                call()
            assert e.value.rc == awfm.AwFmUnsupportedVersionError
        raw.set_text(a.text)
        raw.align_chains_matrix(aligns[0].inputs, 0, 0, awfm.affine_outputs(), 0)  # no reads: succeeds, touches nothing
        raw.align_chains_matrix(*args, scoring=struct, max_candidates=4, max_rows=scratches[0].max_rows)  # every output NULL
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(band_pad=32, max_drift=0), dict(max_ops=0), dict(max_ops=af.MAX_OPS + 1),
                   dict(max_rows=0), dict(max_rows=af.MAX_LENGTH + 1), dict(scoring=mx.Matrix(matrices[0].values, 256, 1).struct(awfm)),
                   dict(scoring=mx.Matrix(matrices[0].values, 6, 0).struct(awfm))):
            with pytest.raises(awfm.AwFmError) as e:
                raw.align_chains_matrix(*args, **dict(dict(scoring=struct, max_candidates=4, max_rows=scratches[0].max_rows), **kw))
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        for bad, kw in (((args[0], 0) + args[2:], dict(scoring=struct)), (args[:4] + (0,), dict(scoring=struct)), (args, dict(scoring=None))):
            with pytest.raises(awfm.AwFmError) as e:  # no slots, no scratch, no matrix
                raw.align_chains_matrix(*bad, max_candidates=4, max_rows=scratches[0].max_rows, **kw)
            assert e.value.rc == -4  # AwFmNullPtrError
        with pytest.raises(awfm.AwFmError) as e:
            raw.score_chains_matrix(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=None)
        assert e.value.rc == -4
        with pytest.raises(awfm.AwFmError) as e:
            raw.score_chains_matrix(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=struct, mapq_cap=255)
        assert e.value.rc == awfm.AwFmIllegalPositionError
        torch.cuda.synchronize()
        # the caller's struct is overwritten as soon as the call has returned, before anything is waited for
        for k in range(2):
            struct = matrices[k].struct(awfm)
            hold = MatrixCalls(awfm, raw)
            _, collect_align = aligns[k].run(hold, *params[k], scratches[k], scoring=struct)
            awfm._lib.C.memset(awfm._lib.C.byref(struct), 0x7F, awfm._lib.C.sizeof(struct))
            struct = matrices[k].struct(awfm)
            _, collect_scores = scores[k].run(hold, *params[k], scoring=struct)
            awfm._lib.C.memset(awfm._lib.C.byref(struct), 0x7F, awfm._lib.C.sizeof(struct))
            torch.cuda.synchronize()
            af.assert_equal(collect_align(), want[k], what=f"overwritten {k}", fill=PATTERN)
            sc.assert_equal(collect_scores(), want_scores[k], what=f"overwritten {k}")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = []
        for _ in range(3):  # a call's scratch is its own until it has finished: the calls of a stream follow each other
            for k in range(2):
                pending.append((aligns[k].run(g, *params[k], scratches[k], scoring=matrices[k], stream=streams[k].cuda_stream, launch=False), af.assert_equal, want[k]))
                pending.append((scores[k].run(g, *params[k], scoring=matrices[k], stream=streams[k].cuda_stream, launch=False), sc.assert_equal, want_scores[k]))
        for (enqueue, _), _, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, ((_, collect), equal, wanted) in enumerate(pending):
            equal(collect(), wanted, what=f"call {k}")
        for s in streams:
            raw.stream_retire(s.cuda_stream)
    finally:
        device.close()


def test_end_to_end_from_the_golden_amino_fasta_file_through_the_alignment_strings(awfm, require_gpu, tmp_path):
    """examples/protein_aligned.c on tests/golden/: peptides -> longest suffix matches -> locate -> local positions -> candidates ->
    chains -> awfmGpuScoreChainsMatrix -> awfmGpuAlignChainsMatrix -> awfmGpuAlignmentStrings, the matrix parsed from its file; the
    program compares the device's results with the host twins', and its lines are what the Python API's host calls give"""
    from test_examples_protein_aligned import expected_lines, run_example
    out = run_example(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert b"device and host twins: 0 reads differ" in out.stderr and b"on the device" in out.stderr
    want, num_aligned, _, _, _ = expected_lines(awfm, tmp_path)
    assert out.stdout.split(b"\n")[:-1] == want and num_aligned == 6
