"""Gap runs of 4 to 63 characters (windows: 2 to 300) through the five host twins of the read path -- awfmVerifyChains,
awfmAlignChains, awfmAlignChainsAffine, awfmScoreChainsAffine, awfmScoreWindowsAffine -- against their plain-Python restatements,
every output bit for bit, on the corpus of tests/gap_runs_common.py; the corpus's own conditions, asserted on the restatement
alone for EVERY case (none is left out): the restated script holds exactly the planted run; and the power condition: the kernel's
row with its scan written out equals the restatement when it runs every step, and differs from it on some case of the matching
group size as soon as one of the steps 2, 4, 8, 16, 32 is left out -- which no gap of up to four characters can show."""
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

IDS = [str(s) for s in gr.SCORINGS]


@pytest.fixture(scope="module")
def corpus():
    """every batch of the banded family: DNA, proteins, the near misses"""
    return gr.banded_corpus(gr.DNA) + gr.banded_corpus(gr.AMINO)


@pytest.fixture(scope="module")
def windows():
    return gr.window_corpus()


def scripts_of(want, r):
    return af.runs_of(want["ops"][r], int(want["numOps"][r]))


def assert_affine_conditions(batch, want, scoring):
    """what the corpus promises of the restated scripts under one scoring"""
    for r, p in enumerate(batch.plants):
        runs = scripts_of(want, r)
        gaps, what = gr.gap_runs(runs), (batch.w, batch.x, p.name, scoring, af.cigar(runs))
        n = len(p.read)
        if p.near is None and scoring in gr.EXPENSIVE:
            assert gaps == [(p.d, gr.OP_OF_KIND[p.kind])], what
            assert int(want["readBegins"][r]) == 0 and int(want["readEnds"][r]) == n, what
        elif p.near is None:
            assert any(op == gr.OP_OF_KIND[p.kind] and run >= min(p.d, 5) for run, op in gaps), what
        elif scoring == af.DEFAULT:
            if "right flank" in p.near:
                assert af.cigar(runs) == f"{p.a}={n - p.a}S" and int(want["scores"][r]) == p.a, what
            elif "clipped" in p.near:
                assert af.cigar(runs) == f"{n - p.c}S{p.c}=" and int(want["scores"][r]) == p.c, what
            else:
                assert af.cigar(runs) == f"{p.a}={p.d}{p.kind}{p.c}=" and int(want["scores"][r]) == p.c + 1, what


def test_the_corpus_has_the_shapes_it_promises(corpus):
    """the bands, the lanes a run begins and ends in, the rows it lies in, the flank rule: arithmetic on the builders' own numbers"""
    dna = [b for b in corpus if b.alphabet == gr.DNA and all(p.near is None for p in b.plants)]
    bands = {(b.w, b.x) for b in dna}
    assert bands == {(0, 63), (8, 15), (24, 15)} | {(0, d) for d in gr.RUNS} | {(d, 0) for d in gr.RUNS if d <= 31}
    assert {b.group for b in dna} == {16, 32, 64}
    lanes, rows = set(), {"D": set(), "I": set()}
    for b in dna:
        for p in b.plants:
            for scoring in gr.EXPENSIVE:
                assert min(p.a, p.c) * scoring[0] > scoring[2] + p.d * scoring[3] + 3 * scoring[0], (p.name, scoring)
            assert min(p.a, p.c) >= 2 * p.d + 10, p.name  # unit costs, and (1, 0, 0, 1): gap_runs_common's flank rule
            if p.kind == "D":  # from lane w to lane w + d of width lanes
                lanes.add((b.w, b.w + p.d, b.x + 2 * b.w + 1))
                rows["D"].add(p.a)
            else:
                rows["I"].add((p.a + 1, p.a + p.d))
    assert {0, 8, 24} <= {first for first, _, _ in lanes} and any(last == width - 1 for _, last, width in lanes)
    assert any(first <= 15 < last for first, last, _ in lanes) and any(first <= 31 < last for first, last, _ in lanes)
    assert set(range(61, 68)) <= rows["D"] and any(a % 64 in range(16, 48) for a in rows["D"])
    assert any(first <= 64 < last for first, last in rows["I"]) and any(first <= 128 < last for first, last in rows["I"])
    assert sorted({p.d for b in dna for p in b.plants}) == sorted(gr.RUNS)
    assert 150 <= sum(len(b.plants) for b in corpus) <= 400


@pytest.mark.parametrize("scoring", gr.SCORINGS, ids=IDS)
def test_affine_alignment_twin_equals_the_restatement_on_every_run(awfm, corpus, scoring):
    replayed = 0
    with gr.shared_local():
        for batch in corpus:
            want = af.Case.expected(batch.case, batch.w, batch.x, scoring, gr.max_ops(scoring))
            assert want["numUnaligned"] == 0 and want["numTruncated"] == 0
            assert_affine_conditions(batch, want, scoring)
            got = batch.case.host(awfm, batch.w, batch.x, scoring, gr.max_ops(scoring), fill=0x5A, threads=4)
            af.assert_equal(got, want, what=f"w={batch.w} x={batch.x} {scoring}", fill=0x5A)
            replayed += af.assert_scripts_replay(batch.case, got, batch.w, batch.x, scoring, gr.max_ops(scoring))
            moved = af.Case(b"###" + batch.case.read_chars.tobytes(), batch.case.offsets + np.uint64(3), batch.case.slots, batch.case.chosen,
                            batch.case.text.tobytes(), batch.case.ends, batch.alphabet)  # the same reads three bytes further into their buffer
            af.assert_equal(moved.host(awfm, batch.w, batch.x, scoring, gr.max_ops(scoring)), got, what="skew 3")
    assert replayed == sum(len(b.plants) for b in corpus)


@pytest.mark.parametrize("scoring", gr.SCORINGS, ids=IDS)
def test_slot_scores_twin_equals_the_restatement_and_both_ends_of_a_run_are_one_placement(awfm, corpus, scoring):
    """slot 0 on the run's begin diagonal and slot 1 on its end diagonal share an end cell: duplicates, no second, mapq = cap --
    unless slot 2 holds the decoy, which is the true second"""
    with gr.shared_local():
        for batch in corpus:
            want = batch.scored.expected_scores(batch.w, batch.x, scoring, cap=gr.CAP)
            assert want["numUnscored"] == 0 and want["numMapped"] == len(batch.plants)
            if scoring in gr.EXPENSIVE:
                for r, p in enumerate(batch.plants):
                    what = (batch.w, batch.x, p.name, scoring, want["slotScores"][r].tolist())
                    if p.near is not None:
                        continue
                    assert all(int(want[name][r, 0]) == int(want[name][r, 1]) for name in sc.SLOT_OUTPUTS), what
                    assert int(want["bestSlots"][r]) == 0 and int(want["slotReadEnds"][r, 0]) == len(p.read), what
                    if r in batch.decoys:
                        assert int(want["secondSlots"][r]) == 2 and 0 < int(want["mappingQualities"][r]) < gr.CAP, what
                        assert 0 < int(want["secondScores"][r]) < int(want["bestScores"][r]), what
                    else:
                        assert int(want["secondSlots"][r]) == sc.NO_SLOT and int(want["mappingQualities"][r]) == gr.CAP, what
            got = batch.scored.score(awfm, batch.w, batch.x, scoring, cap=gr.CAP, threads=4)
            sc.assert_equal(got, want, what=f"w={batch.w} x={batch.x} {scoring}")


def test_verification_and_chain_alignment_twins_equal_their_restatements_on_every_run(awfm, corpus):
    for batch in corpus:
        what = f"w={batch.w} x={batch.x}"
        want = vc.Case.expected(batch.verified, batch.w, batch.x)
        assert want["editDistances"][:, 0].tolist() == batch.distances and want["numUnverified"] == 0, what
        vc.assert_equal(vc.Case.host(batch.verified, awfm, batch.w, batch.x), want, what=what)
        want = ac.Case.expected(batch.case, batch.w, batch.x, gr.UNIT_MAX_OPS)
        assert want["numUnaligned"] == 0 and want["numTruncated"] == 0, what
        for r, p in enumerate(batch.plants):
            if p.near is None:
                runs = ac.runs_of(want["ops"][r], int(want["numOps"][r]))
                assert gr.gap_runs(runs) == [(p.d, gr.OP_OF_KIND[p.kind])] and int(want["editDistances"][r]) == p.d, (what, p.name, ac.cigar(runs))
        ac.assert_equal(ac.Case.host(batch.case, awfm, batch.w, batch.x, gr.UNIT_MAX_OPS, fill=0x5A), want, what=what, fill=0x5A)


def model_of(batch, r, scoring, steps):
    return gr.scan_model(*gr.band_of(batch, r), scoring, batch.alphabet, batch.group, steps)


@pytest.mark.parametrize("scoring", gr.SCORINGS, ids=IDS)
def test_the_row_with_every_step_of_its_scan_equals_the_restatement(corpus, scoring):
    with gr.shared_local() as local:
        for batch in corpus:
            for r, p in enumerate(batch.plants):
                want = local(*gr.band_of(batch, r), scoring, batch.alphabet)
                assert model_of(batch, r, scoring, gr.all_steps(batch.group)) == want, (batch.w, batch.x, p.name)


@pytest.mark.parametrize("group,step", [(G, s) for G in (16, 32, 64) for s in gr.all_steps(G)[1:]])
def test_a_scan_without_one_of_its_steps_differs_on_some_run_at_that_group_size(corpus, group, step):
    """THE POWER CONDITION: the corpus would notice a device scan that is broken at this step"""
    steps = [s for s in gr.all_steps(group) if s != step]
    exposed = []
    with gr.shared_local() as local:
        for batch in corpus:
            if batch.group != group or batch.alphabet != gr.DNA:
                continue
            for r, p in enumerate(batch.plants):
                if p.kind == "D" and p.near is None and (p.d - 1) & step and not exposed:
                    if model_of(batch, r, af.DEFAULT, steps) != local(*gr.band_of(batch, r), af.DEFAULT, batch.alphabet):
                        exposed.append((batch.w, batch.x, p.name))
    assert exposed, (group, step)


def window_runs(case, r, scoring):
    s, begin, end = int(case.sequences[r]), int(case.begins[r]), int(case.window_ends[r])
    S, _ = case.record(s)
    return af.unbanded_local(case.reads[r], bytes(case.text[S + begin:S + end]), scoring)[3]


def test_the_window_corpus_has_the_shapes_it_promises_and_every_window_holds_its_run(windows):
    case, plants = windows
    assert sorted({p.d for p in plants}) == sorted(gr.WINDOW_RUNS) and 60 <= len(plants) <= 200
    assert max(len(r) for r in case.reads) <= gr.WINDOW_MAX_LENGTH and max(p.W for p in plants) <= 1700
    deleted = [(p.col, p.col + p.d) for p in plants if p.kind == "D"]
    for Q in (4, 8, 12):  # a run open across a lane edge, across a block edge, from one on, up to one, over whole lanes
        assert any(first % Q and first // Q != (last - 1) // Q for first, last in deleted)
        assert any(first < 64 * Q * m < last for first, last in deleted for m in (1, 2))
        assert any(first % (64 * Q) == 0 for first, _ in deleted) and any(last % (64 * Q) == 0 for _, last in deleted)
        assert any(last - first >= 3 * Q for first, last in deleted)
    inserted = [(p.a + 1, p.a + p.d, p.col) for p in plants if p.kind == "I"]
    for edge in (64, 256):
        assert any(first <= edge < last and col < 256 + 512 * (edge == 256) for first, last, col in inserted)
        assert any(first <= edge < last and col >= 768 for first, last, col in inserted)
    for r, p in enumerate(plants):
        runs = window_runs(case, r, af.DEFAULT)
        assert gr.gap_runs(runs) == [(p.d, gr.OP_OF_KIND[p.kind])], (p.name, af.cigar(runs))


@pytest.mark.parametrize("scoring", gr.SCORINGS, ids=IDS)
def test_window_scores_twin_equals_the_restatement_on_every_run(awfm, windows, scoring):
    """the begin and end cells are outputs: the origin carried through the run is checked through them"""
    case, plants = windows
    want = case.expected(scoring, min_score=1)
    for r, p in enumerate(plants if scoring in gr.EXPENSIVE else []):  # the whole read, from the planted cell to the planted cell
        begin = int(case.begins[r]) + p.col - p.a
        cells = (0, len(case.reads[r]), begin, begin + p.a + p.c + (p.d if p.kind == "D" else 0))
        assert tuple(int(want[name][r]) for name in ("readBegins", "readEnds", "textBegins", "textEnds")) == cells, (p.name, scoring)
    assert want["numFound"] == len(plants) and want["numUnscored"] == 0
    ws.assert_equal(case.host(awfm, scoring, min_score=1, threads=4), want, what=str(scoring))
