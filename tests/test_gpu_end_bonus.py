"""awfmGpuScoreChainsEndBonus and awfmGpuAlignChainsEndBonus (include/awfm_gpu.h "end bonus", csrc/awfm_end_bonus_kernel.h) against
their host twins awfmScoreChainsEndBonus and awfmAlignChainsEndBonus, which tests/test_end_bonus.py pins to the plain-Python
restatement and to hand-computed values: every output, bit for bit, except the rows of ops of truncated reads -- on the hand
table and the edge lists at the natural number of lanes and with 32 and 64 forced, with the read buffer skewed, with every output
NULL in turn and alone, with maxOps and maxRows at their edges, on reads of every length around the chunk edges (row n the
first, the last and an interior row of a chunk) at every band shape with B = 1, 5, 255, on 2^12 random reads per alphabet with
16 slots, on more reads than the grid has waves, on texts of every length mod 16, with B = 0 against the matrix device calls,
on one read of 2^16 letters worth 127 each with B = 255, from two streams with two bonuses at once, and without a text; the
outputs go through awfmGpuAlignmentStrings and equal its host twin.  Inputs, outputs and the scratch (exactly its declared size)
lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import end_bonus_common as eb  # noqa: E402
import matrix_scores_common as mx  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import test_gpu_align_affine as gaf  # noqa: E402
import test_gpu_score_chains as gsc  # noqa: E402
from test_gpu_byte_values import Image  # noqa: E402  (an index of a well-formed text, the case's own text installed)
from test_gpu_matrix_scores import MatrixCalls  # noqa: E402
from test_gpu_verify_chains import PATTERN  # noqa: E402

pytestmark = pytest.mark.gpu
Scratch, longest_read = gaf.Scratch, gaf.longest_read


class EndBonusCalls:
    """a GpuIndex whose two affine calls are the end-bonus calls: the guarded device calls of the affine tests run them unchanged.
    `scoring` is an eb.Scoring"""

    def __init__(self, awfm, g):
        self.awfm, self.g = awfm, g

    def align_chains_affine(self, *args, scoring=None, **kw):
        return self.g.align_chains_end_bonus(*args, scoring=scoring.struct(self.awfm), end_bonus=scoring.B, **kw)

    def score_chains_affine(self, *args, scoring=None, **kw):
        return self.g.score_chains_end_bonus(*args, scoring=scoring.struct(self.awfm), end_bonus=scoring.B, **kw)

    def __getattr__(self, name):
        return getattr(self.g, name)


class Device:
    """an image of a case's text and the two guarded calls on cases that share it"""

    def __init__(self, awfm, torch, case):
        self.awfm, self.torch, self.image = awfm, torch, Image(awfm, case)
        self.g = EndBonusCalls(awfm, self.image.g)

    def align(self, case, w, x, scoring, scratch=None, skew=0, **kw):
        scratch = scratch or Scratch(self.torch, self.image.g, max(longest_read(case), 1))
        return gaf.DeviceCall(self.awfm, self.torch, case, skew=skew)(self.g, w, x, scratch, scoring=scoring, **kw)

    def score(self, case, w, x, scoring, skew=0, **kw):
        return gsc.DeviceCall(self.awfm, self.torch, case, skew=skew)(self.g, w, x, scoring=scoring, **kw)

    def both_equal_the_twins(self, case, w, x, scoring, what="", max_ops=16, threads=4, **kw):
        got = self.align(case, w, x, scoring, max_ops=max_ops, **kw)
        af.assert_equal(got, case.host(self.awfm, w, x, scoring, max_ops=max_ops, threads=threads), what=f"align {what} {scoring}", fill=PATTERN)
        sc.assert_equal(self.score(case, w, x, scoring, min_score=2, cap=254), case.score(self.awfm, w, x, scoring, min_score=2, cap=254, threads=threads),
                        what=f"score {what} {scoring}")
        return got

    def close(self):
        self.image.close()


@pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
def test_the_hand_table_and_edge_lists_equal_the_host_twins(awfm, require_gpu, diag, group):
    import torch
    diag(affine_group=group, score_group=group)
    for scoring, b in eb.hand_builders():
        case = b.case()
        device = Device(awfm, torch, case)
        try:
            b.check(device.both_equal_the_twins(case, 2, 0, scoring, "by hand", max_ops=8), 8)
        finally:
            device.close()
    builders = {(w, x): af.edge_builder(w, x) for w, x in ((2, 3), (8, 15), (3, 4), (24, 15))}  # 8, 32, 11 and 64 diagonals
    device = Device(awfm, torch, builders[2, 3].case())
    try:
        scratch = Scratch(torch, device.image.g, 64)
        for (w, x), b in builders.items():
            case = eb.as_bonus(b.case())
            b.check(device.both_equal_the_twins(case, w, x, eb.uniform(af.DEFAULT, 0), f"w={w} x={x}", max_ops=8, scratch=scratch), 8)
            for k, B in enumerate((1, 5, 7, 255)):
                device.both_equal_the_twins(case, w, x, eb.uniform(af.DEFAULT, B), f"w={w} x={x}", max_ops=8, scratch=scratch)
                device.both_equal_the_twins(case, w, x, eb.Scoring(mx.ADVERSARIAL[(k + w) % 5], B), f"w={w} x={x}", max_ops=8, scratch=scratch)
        outside = eb.as_bonus(af.outside_builder().case())  # bands without a cell in row n, or in row 0
        for B in (1, 5, 255):
            device.both_equal_the_twins(outside, 0, 0, eb.uniform(af.DEFAULT, B), "outside", scratch=scratch)
        if group is not None:
            return
        b, scoring = builders[2, 3], eb.Scoring(mx.TRANSITIONS, 5)
        case = eb.as_bonus(b.case())
        want, want_scores = case.host(awfm, 2, 3, scoring, max_ops=8), case.score(awfm, 2, 3, scoring)
        for skew in (1, 2, 3):  # the read buffer skewed on the device, and the reads further into it
            skewed = eb.as_bonus(b.case(skew))
            af.assert_equal(device.align(case, 2, 3, scoring, scratch, skew=skew, max_ops=8), want, what=f"buffer skewed by {skew}")
            af.assert_equal(device.align(skewed, 2, 3, scoring, scratch, max_ops=8), want, what=f"reads skewed by {skew}")
            sc.assert_equal(device.score(case, 2, 3, scoring, skew=skew), want_scores, what=f"buffer skewed by {skew}")
            sc.assert_equal(device.score(skewed, 2, 3, scoring), want_scores, what=f"reads skewed by {skew}")
        most = int(want["numOps"].max())
        for max_ops in (most, most - 1):  # exactly the most runs of a read, and one less
            want_ops = case.host(awfm, 2, 3, scoring, max_ops=max_ops)
            assert (want_ops["numTruncated"] > 0) == (max_ops < most)
            af.assert_equal(device.align(case, 2, 3, scoring, scratch, max_ops=max_ops), want_ops, what=f"{max_ops} runs", fill=PATTERN)
        for names, call, equal, wanted in ((list(gaf.SIZES), lambda o: device.align(case, 2, 3, scoring, scratch, max_ops=8, outputs=o), af.assert_equal, want),
                                           (list(gsc.SIZES), lambda o: device.score(case, 2, 3, scoring, outputs=o), sc.assert_equal, want_scores)):
            for missing in names:  # every output NULL in turn, and alone
                for outputs in ([n for n in names if n != missing], [missing]):
                    got = call(outputs)
                    assert sorted(got) == sorted(outputs)
                    equal(got, wanted, names=outputs, what=str(outputs))
        longest = longest_read(case)
        for max_rows in (longest, longest - 1):  # maxRows at the longest read's length and one less: the rule of the device side, restated
            want_rows = case.expected(2, 3, scoring, max_ops=8, max_rows=max_rows)
            assert ((want_rows["scores"] == af.TOO_LONG).sum() > 0) == (max_rows < longest)
            af.assert_equal(device.align(case, 2, 3, scoring, Scratch(torch, device.image.g, max_rows), max_ops=8), want_rows, what=f"maxRows {max_rows}", fill=PATTERN)
    finally:
        device.close()


def lengths_builder(seed=3):
    """reads of 0, 1, 2, 63, 64, 65, 127, 128, 129 and 300 characters -- row n the first, the last and an interior row of a chunk of
    64 rows -- cut from a record of 700, each with a substitution in its second and in its last but one character (kept or
    clipped by B), and a deleted and an inserted character where it is long enough, on the diagonal of its first character"""
    rng = np.random.default_rng(seed)
    record = bytes(rng.choice(np.frombuffer(b"acgt", np.uint8), 700))
    b = eb.Builder([record, b"acgtacgt"])
    for k, n in enumerate((0, 1, 2, 63, 64, 65, 127, 128, 129, 300)):
        at = 40 + 31 * k
        read = bytearray(record[at:at + n])
        if n >= 63:
            read[1] = read[n - 2] = ord("n")
            del read[n // 3]
            read.insert(2 * n // 3, ord("a"))
        b.add(f"n = {n}", bytes(read), 0, at, at, None)
    return b


def test_read_lengths_with_row_n_at_every_place_of_a_chunk_at_every_band_shape(awfm, require_gpu):
    import torch
    b = lengths_builder()
    device = Device(awfm, torch, b.case())
    try:
        scratch = Scratch(torch, device.image.g, 300)
        kept = set()
        for width, (w, x) in sorted(af.BAND_SHAPES.items()):
            for k, B in enumerate((1, 5, 255)):
                skew = (width + k) % 4
                matrix = mx.uniform(af.DNA, af.DEFAULT) if (width + k) % 2 else mx.ADVERSARIAL[(width + k) % 5]
                got = device.both_equal_the_twins(b.case(skew), w, x, eb.Scoring(matrix, B), f"width {width} skew {skew}", max_ops=24, scratch=scratch,
                                                  skew=(4 - skew) % 4)
                if matrix.name.startswith("uniform") and w >= 1:
                    kept.add((B, bool(got["readBegins"][3] == 0), bool(got["readEnds"][9] == 300)))
        assert kept == {(1, False, False), (5, True, True), (255, True, True)}, kept  # 1 + B > 4: the second character's substitution is kept
    finally:
        device.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_batch_of_4096_reads_with_16_slots(awfm, require_gpu, alphabet):
    """lengths 1..300 with the chunk edges among them, edits of 0..12 %, a tenth of the slots unused, some malformed, a tenth
    hanging over a record end, a text of 2^16 positions in 37 records, sixteen slots a read"""
    import torch
    rng = np.random.default_rng(41)
    lengths = rng.integers(1, 301, 1 << 12)
    lengths[:12] = [63, 64, 65, 127, 128, 129, 1, 300, 63, 64, 65, 2]
    case = eb.random_case(20, 1 << 12, 16, alphabet, text_length=1 << 16, num_records=37, lengths=lengths, hanging=0.1, other=0.3)
    device = Device(awfm, torch, case)
    try:
        scratch = Scratch(torch, device.image.g, longest_read(case))
        gaps = (11, 1) if alphabet == af.AMINO else (6, 1)
        for scoring, (w, x) in ((eb.Scoring(mx.random_matrix(1, -128, 127, *gaps), 255), (8, 15)), (eb.Scoring(mx.random_matrix(2, -4, 11, *gaps), 5), (20, 23))):
            got = device.both_equal_the_twins(case, w, x, scoring, f"w={w}", max_ops=64, threads=16, scratch=scratch)
            assert ((got["scores"] > 0) & (got["scores"] < af.TOO_LONG)).sum() > 1500 and (got["scores"] == af.MALFORMED).sum() > 50
    finally:
        device.close()


def test_more_reads_than_the_grid_has_waves(awfm, require_gpu, diag):
    """4100 reads of 200..600 characters with 64 lanes each under the alignment call -- more than the 4096 waves of the largest
    grid --, and 2^15 reads of one slot under the scoring call, more than its grid's waves (256 CUs x 7 workgroups x 4)"""
    import torch
    diag(affine_group=64)
    rng = np.random.default_rng(43)
    scoring = eb.Scoring(mx.random_matrix(4, -4, 11), 7)
    case = eb.random_case(19, 4100, 1, text_length=1 << 16, num_records=37, lengths=rng.integers(200, 601, 4100), max_rate=0.06)
    many = eb.random_case(21, 1 << 15, 1, text_length=1 << 16, num_records=37, max_length=40)
    many.text, many.ends = case.text, case.ends
    device = Device(awfm, torch, case)
    try:
        af.assert_equal(device.align(case, 8, 15, scoring, max_ops=64), case.host(awfm, 8, 15, scoring, max_ops=64, threads=16), fill=PATTERN)
        sc.assert_equal(device.score(many, 8, 15, scoring), many.score(awfm, 8, 15, scoring, threads=16))
    finally:
        device.close()


def test_texts_of_every_length_mod_16_aligned_up_to_their_last_byte(awfm, require_gpu):
    import torch
    for length in range(96, 112):
        case = eb.as_bonus(af.tail_case(length).case())
        device = Device(awfm, torch, case)
        try:
            got = device.both_equal_the_twins(case, 2, 3, eb.uniform(af.DEFAULT, 5), f"length {length}", max_ops=32)
            assert got["readBegins"].tolist() == [0, 0] and got["readEnds"].tolist() == [24, 24]  # 1 + 5 > 4: the second character is kept
            device.both_equal_the_twins(case, 2, 3, eb.Scoring(mx.TRANSITIONS, 255), f"length {length}", max_ops=32)
        finally:
            device.close()


@pytest.mark.parametrize("alphabet", [af.DNA, af.AMINO], ids=["dna", "amino"])
def test_no_bonus_gives_what_the_matrix_device_calls_give(awfm, require_gpu, alphabet):
    import torch
    case = eb.random_case(31, 1500, 4, alphabet, text_length=1 << 14, max_length=150, hanging=0.2)
    plain = case.matrix_case()
    device = Device(awfm, torch, case)
    try:
        scratch = Scratch(torch, device.image.g, longest_read(case))
        siblings = MatrixCalls(awfm, device.image.g)
        gaps = (11, 1) if alphabet == af.AMINO else (6, 1)
        for matrix, (w, x) in zip((mx.random_matrix(1, -128, 127, *gaps), mx.random_matrix(2, -4, 11, *gaps), mx.uniform(alphabet, af.DEFAULT)), ((8, 15), (2, 3), (20, 23))):
            scoring = eb.Scoring(matrix, 0)
            got = gaf.DeviceCall(awfm, torch, case)(device.g, w, x, scratch, scoring=scoring, max_ops=24)
            af.assert_equal(got, gaf.DeviceCall(awfm, torch, plain)(siblings, w, x, scratch, scoring=matrix, max_ops=24), what=repr(matrix), fill=PATTERN)
            af.assert_equal(got, plain.host(awfm, w, x, matrix, max_ops=24, threads=8), what=f"host {matrix}", fill=PATTERN)
            sc.assert_equal(gsc.DeviceCall(awfm, torch, case)(device.g, w, x, scoring=scoring, min_score=3),
                            gsc.DeviceCall(awfm, torch, plain)(siblings, w, x, scoring=matrix, min_score=3), what=repr(matrix))
    finally:
        device.close()


def test_one_read_of_two_to_the_sixteen_letters_worth_127_each_with_the_largest_bonus(awfm, require_gpu):
    """the end cell's key at its top: the score is 65536 x 127 + 2 x 255, the end cell (2^16, 2^16); and one letter more is too long"""
    import torch
    n = af.MAX_LENGTH
    letters = np.random.default_rng(8).choice(np.frombuffer(b"acgt", np.uint8), n + 1)
    slots = {name: np.array([[0] * 3, [0] * 3], vc.SLOT_DTYPES[name]) for name in vc.SLOT_FIELDS}
    slots["chainAnchors"][:] = 1
    slots["chainReadEnds"][:, 0] = (n, n + 1)
    slots["chainBeginDiagonals"][:, 2] = slots["chainEndDiagonals"][:, 2] = 1  # a third slot one diagonal off, whose band holds the same cells
    slots["sequences"][:, 1] = vc.NONE
    case = eb.Case(letters[:n].tobytes() + letters.tobytes(), [0, n, 2 * n + 1], slots, [0, 0], letters.tobytes() + b"\0", [n + 1])
    scoring = eb.Scoring(mx.Matrix(np.where(np.eye(21, dtype=bool), 127, -128), 255, 255, "127 / -128"), 255)
    top = n * 127 + 2 * 255
    assert top == 8323072 + 510 and top < 1 << 24
    device = Device(awfm, torch, case)
    try:
        got = device.score(case, 8, 15, scoring, cap=254)
        assert got["slotScores"][0].tolist()[:2] == [top, sc.NONE] and got["slotScores"][1].tolist()[:2] == [sc.TOO_LONG, sc.NONE]
        assert int(got["slotReadEnds"][0, 0]) == n and int(got["slotTextEnds"][0, 0]) == n and got["bestScores"].tolist() == [top, 0]
        sc.assert_equal(got, case.score(awfm, 8, 15, scoring, cap=254, threads=2))
    finally:
        device.close()


def test_two_streams_two_bonuses_refusals_and_an_image_without_a_text(awfm, require_gpu):
    import torch
    a, b = eb.random_case(5, 600, 4, max_length=200, hanging=0.1), eb.random_case(6, 500, 3, max_length=120, hanging=0.1)
    b.text, b.ends = a.text, a.ends
    device = Device(awfm, torch, a)
    try:
        g, raw = device.g, device.image.g
        scorings = [eb.Scoring(mx.random_matrix(11, -128, 127), 255), eb.Scoring(mx.random_matrix(12, -4, 11, 11, 1), 5)]
        params = [(8, 15), (2, 3)]
        scratches = [Scratch(torch, raw, longest_read(a)), Scratch(torch, raw, longest_read(b))]
        want = [c.host(awfm, w, x, m) for c, (w, x), m in zip((a, b), params, scorings)]
        want_scores = [c.score(awfm, w, x, m) for c, (w, x), m in zip((a, b), params, scorings)]
        aligns, scores = [gaf.DeviceCall(awfm, torch, c) for c in (a, b)], [gsc.DeviceCall(awfm, torch, c) for c in (a, b)]
        args = (aligns[0].inputs, aligns[0].chosen.data_ptr(), a.num_reads, awfm.affine_outputs(), scratches[0].address)
        struct = scorings[0].struct(awfm)
        raw.set_text(None)
        for call in (lambda: raw.align_chains_end_bonus(*args, scoring=struct, end_bonus=5, max_candidates=4, max_rows=scratches[0].max_rows),
                     lambda: raw.score_chains_end_bonus(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=struct, end_bonus=5)):
            with pytest.raises(awfm.AwFmError) as e:
                call()
            assert e.value.rc == awfm.AwFmUnsupportedVersionError
        raw.set_text(a.text)
        raw.align_chains_end_bonus(aligns[0].inputs, 0, 0, awfm.affine_outputs(), 0, end_bonus=256)  # no reads: succeeds, touches nothing
        raw.align_chains_end_bonus(*args, scoring=struct, end_bonus=255, max_candidates=4, max_rows=scratches[0].max_rows)  # every output NULL
        for kw in (dict(max_candidates=0), dict(max_candidates=17), dict(band_pad=32, max_drift=0), dict(max_ops=0), dict(max_ops=af.MAX_OPS + 1),
                   dict(max_rows=0), dict(max_rows=af.MAX_LENGTH + 1), dict(scoring=mx.Matrix(scorings[0].values, 256, 1).struct(awfm)),
                   dict(scoring=mx.Matrix(scorings[0].values, 6, 0).struct(awfm)), dict(end_bonus=256), dict(end_bonus=2 ** 32 - 1)):
            with pytest.raises(awfm.AwFmError) as e:
                raw.align_chains_end_bonus(*args, **dict(dict(scoring=struct, end_bonus=5, max_candidates=4, max_rows=scratches[0].max_rows), **kw))
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        for bad, kw in (((args[0], 0) + args[2:], dict(scoring=struct)), (args[:4] + (0,), dict(scoring=struct)), (args, dict(scoring=None))):
            with pytest.raises(awfm.AwFmError) as e:  # no slots, no scratch, no matrix
                raw.align_chains_end_bonus(*bad, max_candidates=4, max_rows=scratches[0].max_rows, **kw)
            assert e.value.rc == -4  # AwFmNullPtrError
        with pytest.raises(awfm.AwFmError) as e:
            raw.score_chains_end_bonus(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=None)
        assert e.value.rc == -4
        for kw in (dict(mapq_cap=255), dict(end_bonus=256)):
            with pytest.raises(awfm.AwFmError) as e:
                raw.score_chains_end_bonus(scores[0].inputs, a.num_reads, awfm.slot_score_outputs(), scoring=struct, **kw)
            assert e.value.rc == awfm.AwFmIllegalPositionError, kw
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        pending = []
        for _ in range(3):  # a call's scratch is its own until it has finished: the calls of a stream follow each other
            for k in range(2):
                pending.append((aligns[k].run(g, *params[k], scratches[k], scoring=scorings[k], stream=streams[k].cuda_stream, launch=False), af.assert_equal, want[k]))
                pending.append((scores[k].run(g, *params[k], scoring=scorings[k], stream=streams[k].cuda_stream, launch=False), sc.assert_equal, want_scores[k]))
        for (enqueue, _), _, _ in pending:  # interleaved, nothing waited for in between
            enqueue()
        torch.cuda.synchronize()
        for k, ((_, collect), equal, wanted) in enumerate(pending):
            equal(collect(), wanted, what=f"call {k}")
        for s in streams:
            raw.stream_retire(s.cuda_stream)
    finally:
        device.close()


def test_the_outputs_go_through_the_alignment_strings_and_equal_the_host_twin(awfm, require_gpu, tmp_path):
    """examples/read_unclipped.c on a FASTA file of its own making: reads -> awfmGpuScoreChainsEndBonus -> awfmGpuAlignChainsEndBonus
    -> awfmGpuAlignmentStrings under B = 0 and B = 5; the program compares the device's results with the host twins', and its lines
    are what the host calls give"""
    from test_examples_read_unclipped import expected_lines, run_example
    want, (plain, bonus), _, by_hand = expected_lines(awfm, tmp_path)
    out = run_example(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert b"device and host twins: 0 reads differ" in out.stderr and b"on the device" in out.stderr
    assert out.stdout.split(b"\n")[:-1] == want
    assert int(plain["readEnds"][by_hand]) == 97 and int(bonus["readEnds"][by_hand]) == 100  # the end that the bonus reaches
