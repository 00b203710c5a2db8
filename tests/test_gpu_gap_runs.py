"""Gap runs of 4 to 63 characters (windows: 2 to 300) through the five device calls of the read path -- awfmGpuVerifyChains,
awfmGpuAlignChains, awfmGpuAlignChainsAffine, awfmGpuScoreChainsAffine, awfmGpuScoreWindowsAffine -- against their host twins,
which tests/test_gap_runs.py pins to the plain-Python restatements on the same corpus (tests/gap_runs_common.py): every output,
bit for bit, under the five scorings, with the read buffer at skew 0 and 3, the banded calls at the natural number of lanes
and with 32 and 64 forced (a run of d characters needs the scan's steps up to the largest power of two in d - 1, and the steps
16 and 32 exist at 32 and 64 lanes only), the window call at the natural number of columns per lane and with 4, 8 and 12
forced (which moves the lane and block edges under the runs).  Inputs, outputs and scratch lie between guard words."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_affine_common as af  # noqa: E402
import align_chains_common as ac  # noqa: E402
import gap_runs_common as gr  # noqa: E402
import score_chains_common as sc  # noqa: E402
import verify_chains_common as vc  # noqa: E402
import window_scores_common as ws  # noqa: E402
import test_gpu_align_affine as gaa  # noqa: E402
import test_gpu_align_chains as gac  # noqa: E402
import test_gpu_score_chains as gsc  # noqa: E402
import test_gpu_verify_chains as gvc  # noqa: E402
import test_gpu_window_scores as gws  # noqa: E402
from test_gpu_verify_chains import GUARD, PATTERN, Image  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABETS = pytest.mark.parametrize("alphabet", [gr.DNA, gr.AMINO], ids=["dna", "amino"])
GROUPS = pytest.mark.parametrize("group", [None, 32, 64], ids=["natural", "32", "64"])
_CORPUS, _TWIN = {}, {}


def corpus_of(alphabet):
    if alphabet not in _CORPUS:
        _CORPUS[alphabet] = gr.banded_corpus(alphabet)
    return _CORPUS[alphabet]


def batches_at(alphabet, group):
    """the batches a forced group size changes anything for: those whose own is smaller"""
    return [(k, b) for k, b in enumerate(corpus_of(alphabet)) if group is None or b.group < group]


def twin(key, call):
    """a host twin's outputs, computed once for all the group sizes and skews they are compared at"""
    if key not in _TWIN:
        _TWIN[key] = call()
    return _TWIN[key]


@ALPHABETS
@GROUPS
def test_verification_of_every_run(awfm, require_gpu, diag, alphabet, group):
    import torch
    diag(verify_group=group)
    image = Image(awfm, corpus_of(alphabet)[0].case)
    try:
        for k, b in batches_at(alphabet, group):
            want = twin(("verify", alphabet, k), lambda: vc.Case.host(b.verified, awfm, b.w, b.x, unverified_before=5))
            assert want["editDistances"][:, 0].tolist() == b.distances
            for skew in (0, 3):
                got = gvc.DeviceCall(awfm, torch, b.verified, skew=skew)(image.g, b.w, b.x, unverified_before=5)
                vc.assert_equal(got, want, what=f"w={b.w} x={b.x} skew {skew}")
    finally:
        image.close()


@ALPHABETS
@GROUPS
def test_chain_alignment_of_every_run(awfm, require_gpu, diag, alphabet, group):
    import torch
    diag(align_group=group)
    image = Image(awfm, corpus_of(alphabet)[0].case)
    try:
        scratch = gac.Scratch(torch, image.g, max(b.max_rows() for b in corpus_of(alphabet)))
        for k, b in batches_at(alphabet, group):
            want = twin(("align", alphabet, k), lambda: ac.Case.host(b.case, awfm, b.w, b.x, gr.UNIT_MAX_OPS, unaligned_before=5, truncated_before=3))
            assert want["numUnaligned"] == 5 and want["numTruncated"] == 3
            for skew in (0, 3):
                got = gac.DeviceCall(awfm, torch, b.case, skew=skew)(image.g, b.w, b.x, scratch, max_ops=gr.UNIT_MAX_OPS, unaligned_before=5, truncated_before=3)
                ac.assert_equal(got, want, what=f"w={b.w} x={b.x} skew {skew}", fill=PATTERN)
    finally:
        image.close()


@ALPHABETS
@GROUPS
def test_affine_alignment_of_every_run(awfm, require_gpu, diag, alphabet, group):
    import torch
    diag(affine_group=group)
    image = Image(awfm, corpus_of(alphabet)[0].case)
    try:
        scratch = gaa.Scratch(torch, image.g, max(b.max_rows() for b in corpus_of(alphabet)))
        for k, b in batches_at(alphabet, group):
            calls = [gaa.DeviceCall(awfm, torch, b.case, skew=skew) for skew in (0, 3)]
            for scoring in gr.SCORINGS:
                max_ops = gr.max_ops(scoring)
                want = twin(("affine", alphabet, k, scoring), lambda: b.case.host(awfm, b.w, b.x, scoring, max_ops, unaligned_before=5, truncated_before=3))
                assert want["numUnaligned"] == 5 and want["numTruncated"] == 3
                for call in calls:
                    got = call(image.g, b.w, b.x, scratch, scoring=scoring, max_ops=max_ops, unaligned_before=5, truncated_before=3)
                    af.assert_equal(got, want, what=f"w={b.w} x={b.x} {scoring}", fill=PATTERN)
    finally:
        image.close()


@ALPHABETS
@GROUPS
def test_slot_scores_of_every_run_from_both_its_ends(awfm, require_gpu, diag, alphabet, group):
    import torch
    diag(score_group=group)
    image = Image(awfm, corpus_of(alphabet)[0].case)
    try:
        for k, b in batches_at(alphabet, group):
            calls = [gsc.DeviceCall(awfm, torch, b.scored, skew=skew) for skew in (0, 3)]
            for scoring in gr.SCORINGS:
                want = twin(("score", alphabet, k, scoring), lambda: b.scored.score(awfm, b.w, b.x, scoring, cap=gr.CAP, unscored_before=5, mapped_before=3))
                assert want["numUnscored"] == 5 and want["numMapped"] == 3 + len(b.plants)
                for call in calls:
                    got = call(image.g, b.w, b.x, scoring=scoring, cap=gr.CAP, unscored_before=5, mapped_before=3)
                    sc.assert_equal(got, want, what=f"w={b.w} x={b.x} {scoring}")
    finally:
        image.close()


class WindowCall(gws.DeviceCall):
    """gws.DeviceCall with the scratch, exactly its declared size, between guard words too"""

    def run(self, g, scoring=ws.DEFAULT, min_score=0, max_length=gr.WINDOW_MAX_LENGTH, unscored_before=0, found_before=0):
        torch, n = self.torch, self.case.num_reads
        buffers = {name: torch.full((gws.size_of(name, n, 1) + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda") for name in gws.NAMES}
        for name, before in (("numUnscored", unscored_before), ("numFound", found_before)):
            buffers[name][GUARD:GUARD + 8] = torch.from_numpy(np.array([before], np.uint64).view(np.uint8)).to("cuda")
        wout = self.awfm.window_score_outputs(**{name: b.data_ptr() + GUARD for name, b in buffers.items()})
        size = g.score_windows_affine_scratch_bytes(max_length)
        assert size > 0 and size % 16 == 0
        scratch = torch.full((size + 2 * GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.score_windows_affine(self.inputs, n, wout, scratch.data_ptr() + GUARD, max_length, scoring=scoring, min_score=min_score)

        def collect():
            result = {}
            for name, b in buffers.items():
                raw, size_of = b.cpu().numpy(), gws.size_of(name, n, 1)
                assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + size_of:] == PATTERN).all(), f"wrote outside {name}"
                body = raw[GUARD:GUARD + size_of]
                result[name] = int(body.view(np.uint64)[0]) if name in ws.COUNTERS else body.view(gws.DTYPES[name]).reshape((n, 1) if name in ws.SLOT_OUTPUTS else (n,))
            assert bool((scratch[:GUARD] == PATTERN).all()) and bool((scratch[GUARD + size:] == PATTERN).all()), "wrote outside the scratch"
            return result

        return None, collect


@pytest.mark.parametrize("q", gws.TIERS, ids=["natural", "4", "8", "12"])
def test_window_scores_of_every_run(awfm, require_gpu, diag, q):
    """the begin and end cells are outputs: what the lanes, the arena and the boundary rows carry of E and its origin is checked
    through them"""
    import torch
    diag(window_q=q)
    case, plants = twin("windows", gr.window_corpus)
    image = Image(awfm, case)
    try:
        calls = [WindowCall(awfm, torch, case, skew=skew) for skew in (0, 3)]
        for scoring in gr.SCORINGS:
            want = twin(("window", scoring), lambda: gws.twin(awfm, case, scoring=scoring, min_score=1, unscored_before=5, found_before=3))
            assert want["numFound"] == 3 + len(plants) and want["numUnscored"] == 5
            for call in calls:
                ws.assert_equal(call(image.g, scoring=scoring, min_score=1, unscored_before=5, found_before=3), want, what=str(scoring))
    finally:
        image.close()
