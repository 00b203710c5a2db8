"""The kept hits of a read (include/awfm_gpu.h, "candidate loci") are defined once for awfmReadCandidates and awfmReadChains
(csrc/awfm_hits.h): both twins on ONE table -- the edge list, every malformed shape and dropped seeds that hold whole rounds, at
maxHitsPerSeed 0, 1 and 3, the chains on the candidates' own slots -- report the same keptHits as each other and as the NumPy
restatement, add the same number to numOverflowed, and refuse the same arguments with the same code."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kept_hits_common as kh  # noqa: E402
import read_candidates_common as rc  # noqa: E402


@pytest.fixture(scope="module")
def table(awfm):
    return kh.host_table(awfm)


def test_both_twins_report_the_kept_hits_of_the_definition(table):
    seen = set()
    for what, inst, m, _, candidates, chains in table:
        want, _ = kh.kept_hits_by_the_definition(inst, m)
        assert np.array_equal(candidates["keptHits"], want), (what, "candidates", candidates["keptHits"].tolist(), want.tolist())
        assert np.array_equal(chains["keptHits"], want), (what, "chains", chains["keptHits"].tolist(), want.tolist())
        seen.update(want.tolist())
    # the table holds what it is for: no hit, one, the limit and one more, a malformed read (and seeds of 63, 64 and 65 hits,
    # kept at maxHitsPerSeed 0 and dropped otherwise: rc.dropped_seeds_instance)
    assert {0, 1, rc.MAX_HITS, rc.MAX_HITS + 1, rc.MALFORMED} <= seen, sorted(seen)


def test_both_twins_count_the_same_reads_as_overflowed(table):
    for what, inst, m, _, candidates, chains in table:
        _, overflowed = kh.kept_hits_by_the_definition(inst, m)
        assert candidates["numOverflowed"] - kh.OVERFLOWED_BEFORE == overflowed, (what, "candidates")
        assert chains["numOverflowed"] - kh.OVERFLOWED_BEFORE == overflowed, (what, "chains")
    assert any(kh.kept_hits_by_the_definition(inst, m)[1] for _, inst, m, *_ in table)


@pytest.mark.parametrize("what,changes,code,_text", kh.REFUSALS, ids=[r[0] for r in kh.REFUSALS])
def test_both_twins_refuse_the_same_arguments(awfm, what, changes, code, _text):
    from avxwindowfmindex_amd import _lib
    L = _lib.lib()
    inst = rc.random_instance(5, reads=4)
    arrays = [inst.offsets, inst.seed_ends, inst.seed_lengths, inst.hit_offsets, inst.positions, inst.sequences]
    o, ends, lengths, ho, pos, sn = [a.ctypes.data for a in arrays]
    good = awfm.candidate_inputs(o, inst.num_seeds, ends, lengths, 0, ho, inst.num_hits, pos, sn)
    inputs, num_reads, slots, with_outputs = kh.refused_call(awfm, good, inst.num_reads, changes)
    slot_arrays = [np.full(4 * 17, rc.NONE, np.uint32), np.zeros(4 * 17, np.int64), np.zeros(4 * 17, np.uint32)]
    candidate_out = awfm.candidate_outputs() if with_outputs else None
    chain_out = awfm.chain_outputs() if with_outputs else None
    got = L.awfmReadCandidates(kh.byref_or_null(inputs), num_reads, 0, kh.BAND, 1, slots, kh.byref_or_null(candidate_out), 1)
    assert got == code, (what, "awfmReadCandidates", got)
    got = L.awfmReadChains(kh.byref_or_null(inputs), num_reads, 0, kh.BAND, slots, *[a.ctypes.data for a in slot_arrays], 64, 0,
                           kh.byref_or_null(chain_out), 1)
    assert got == code, (what, "awfmReadChains", got)
