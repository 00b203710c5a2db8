"""awfmReadChains (include/awfm_gpu.h "read chains", csrc/awfm_chains.c): the host twin against the plain-Python restatement of
the definition (tests/read_chains_common.py) on random batches and on the edge list, every output and every output NULL in turn;
a brute-force search over all chains of small slots as a second oracle; hand-written expectations, so that the restatement is
pinned too; the error codes; end to end from a FASTA file; and the twin under AddressSanitizer + UBSan as a stand-alone
program."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402
import read_chains_common as ch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")

# (band, C, lookback, gapPenalty) on top of the edge list's own maxHitsPerSeed
EDGE_PARAMS = [(ch.EDGE_BAND, 4, 64, 0), (ch.EDGE_BAND, 1, 1, 0), (ch.EDGE_BAND, 16, 64, 1), (0, 16, 7, 2), (0xFFFFFFFF, 3, 64, 0),
               (ch.EDGE_BAND, 16, 64, 0xFFFFFFFF), (0xFFFFFFFF, 2, 2, 0xFFFFFFFF)]


@pytest.fixture(scope="module")
def edge():
    return ch.edge_instance()


def _edge_case(awfm, edge, band, slots):
    return ch.candidate_case(awfm, edge, band, slots, max_hits_per_seed=ch.EDGE_MAX_HITS)


@pytest.mark.parametrize("band,slots,lookback,gap_penalty", EDGE_PARAMS)
def test_edge_list_equals_the_restatement(awfm, edge, band, slots, lookback, gap_penalty):
    case = _edge_case(awfm, edge, band, slots)
    params = dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=band, lookback=lookback, gap_penalty=gap_penalty)
    want = ch.expected(case, overflowed_before=3, **params)
    ch.assert_equal(case.host(awfm, overflowed_before=3, fill=0xA5, **params), want)
    assert want["numOverflowed"] == 3 + 1  # the counter is added to
    if gap_penalty == 0xFFFFFFFF and band == ch.EDGE_BAND:  # every step of the drifting read costs more than it brings
        assert want["chainAnchors"][ch.EDGE_READS["drift"], 0] == 1


def _slot(result, r, j=0):
    """(score, anchors, read begin, read end, begin diagonal, end diagonal) of read r's slot j"""
    return tuple(int(result[name][r, j]) for name in ch.SLOT_FIELDS)


def test_edge_list_by_hand(awfm, edge):
    """what the definition says of each entry, written out: pins the restatement as well as the twin"""
    at = ch.EDGE_READS
    case = _edge_case(awfm, edge, ch.EDGE_BAND, 16)
    params = dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=ch.EDGE_BAND)
    got = case.host(awfm, fill=0xA5, **params)
    for name in ("empty read", "seeds without hits"):
        assert got["bestSlots"][at[name]] == ch.NO_SLOT and got["keptHits"][at[name]] == 0
        assert all(_slot(got, at[name], j) == (0,) * 6 for j in range(16))  # all zeros over the 0xA5
    assert _slot(got, at["one anchor"]) == (20, 1, 0, 20, 100, 100) and got["bestSlots"][at["one anchor"]] == 0
    assert _slot(got, at["equal e"]) == (20, 1, 0, 20, 100, 100)  # two hits with one e never chain
    assert _slot(got, at["dt = 0"]) == (10, 1, 10, 20, 100, 100)  # the second anchor would begin where the first begins
    assert _slot(got, at["dt = 1"]) == (11, 2, 10, 24, 100, 97)  # ... one character further: worth one
    assert _slot(got, at["g = band"]) == (20, 2, 10, 30, 100, 105)
    assert _slot(got, at["g = band + 1"]) == (15, 2, 15, 30, 103, 106)
    assert _slot(got, at["one diagonal"]) == (36, 5, 0, 36, 1000, 1000)  # five overlapping 20-mers cover 36 characters
    assert _slot(got, at["drift"]) == (60, 6, 10, 70, 500, 510)
    assert _slot(got, at["zero length alone"]) == (0, 1, 20, 20, 100, 100) and got["bestSlots"][at["zero length alone"]] == 0
    assert _slot(got, at["zero length in a chain"]) == (20, 3, 10, 40, 100, 100)  # the empty seed brings nothing, ties, and is the later one
    assert _slot(got, at["negative diagonals"]) == (30, 3, 5, 45, -5, -2)
    assert _slot(got, at["tie between predecessors"]) == (20, 2, 0, 30, 101, 100)
    assert _slot(got, at["tie between chain ends"]) == (30, 2, 0, 30, 100, 100)
    assert _slot(got, at["a repeat seed"]) == (40, 3, 0, 40, 100, 100)  # the seed with two hits in the band counts once
    assert got["keptHits"][at["at and above maxHitsPerSeed"]] == 4  # the seed of three hits and the one behind it
    assert _slot(got, at["illegal hits in between"]) == (24, 2, 0, 24, 300, 300)
    assert got["keptHits"][at["4096 kept hits"]] == 4096 and got["bestSlots"][at["4096 kept hits"]] != ch.NO_SLOT
    r = at["4097 kept hits"]
    assert got["keptHits"][r] == 4097 and got["bestSlots"][r] == ch.NO_SLOT and got["numOverflowed"] == 1
    assert all(_slot(got, r, j) == (0,) * 6 for j in range(16))
    assert _slot(got, at["after the overflow"]) == (20, 1, 0, 20, 123, 123)
    penalised = case.host(awfm, gap_penalty=3, **params)
    assert _slot(penalised, at["tie between predecessors"]) == (20, 2, 0, 30, 100, 100)
    assert _slot(penalised, at["dt = 1"]) == (10, 1, 10, 20, 100, 100)  # 11 - 3 * 3 is not above the anchor's own 10
    assert _slot(penalised, at["drift"]) == (30, 6, 10, 70, 500, 510)  # five steps of two diagonals: 60 - 5 * 2 * 3
    wide = ch.candidate_case(awfm, edge, 0xFFFFFFFF, 4, max_hits_per_seed=ch.EDGE_MAX_HITS)
    got = wide.host(awfm, max_hits_per_seed=ch.EDGE_MAX_HITS, band=0xFFFFFFFF)
    r = at["across 2^32"]
    j = [int(s) for s in wide.sequences[r]].index(9)
    # the slot's span is saturated at 2^32 - 1: it holds D = 10 and 2^32 + 9, and not 2^33 + 8
    assert int(wide.spans[r, j]) == 0xFFFFFFFF and _slot(got, r, j) == (30, 2, 0, 30, 10, (1 << 32) + 9)


def test_hand_made_slots_and_the_reach_of_lookback(awfm):
    case = ch.lookback_case()
    for lookback, score in ((64, (25, 2, 25, 100, 1001, 1000)), (63, (20, 1, 80, 100, 1000, 1000)), (1, (20, 1, 80, 100, 1000, 1000))):
        params = dict(band=5, lookback=lookback)
        got = case.host(awfm, **params)
        ch.assert_equal(got, ch.expected(case, **params), what=str(lookback))
        assert _slot(got, 0, 0) == score, lookback  # the predecessor at distance 65 would give 32
    assert got["bestSlots"].tolist() == [0, 2, 1] and _slot(got, 1, 0) == (0,) * 6 and _slot(got, 1, 2) == (30, 2, 0, 30, 100, 100)
    assert _slot(got, 2, 1) == (20, 2, 10, 40, 100, 100)  # band 5: the two pairs 40 diagonals apart tie, the first one wins
    assert _slot(case.host(awfm, band=40, lookback=2), 2, 1) == (40, 4, 10, 80, 100, 140)


def test_the_three_cases_of_the_issue_by_hand(awfm):
    """votes against chains; a deletion; a repeat seed"""
    overlapping = [ch.anchor(60 + i, 60, 5000, 1) for i in range(10)]  # ten 60-mers over read offsets [0, 69)
    disjoint = [ch.anchor(30 * (i + 1), 30, 9000, 2) for i in range(4)]  # four 30-mers over [0, 120)
    # a read of 100 characters whose characters 50.. lie two further along in the sequence: 20-mers every 10 characters
    deletion = [ch.anchor(e, 20, 700 if e <= 50 else 702) for e in range(20, 101, 10) if not 50 < e < 70]
    repeat = [ch.anchor(20, 20, 100), (30, 20, [(0, 110), (0, 111)]), ch.anchor(40, 20, 100)]
    inst = rc.from_reads([overlapping + disjoint, deletion, repeat])
    case = ch.candidate_case(awfm, inst, 2, 2)
    got = case.host(awfm, band=2)
    ch.assert_equal(got, ch.expected(case, band=2))
    votes = inst.host(awfm, band=2, max_candidates=2)["votes"][0].tolist()
    assert votes == [10, 4] and case.sequences[0].tolist() == [1, 2]  # votes put the overlapping 60-mers first ...
    assert _slot(got, 0, 0) == (69, 10, 0, 69, 5000, 5000) and _slot(got, 0, 1) == (120, 4, 0, 120, 9000, 9000)
    assert got["bestSlots"][0] == 1  # ... chains the four that cover the read
    assert _slot(got, 1, 0) == (100, 8, 0, 100, 700, 702) and case.sequences[1, 1] == ch.NONE  # one chain across the deletion
    apart = ch.candidate_case(awfm, inst, 0, 2)
    got0 = apart.host(awfm, band=0)
    assert sorted([_slot(got0, 1, 0), _slot(got0, 1, 1)]) == [(50, 4, 0, 50, 700, 700), (50, 4, 50, 100, 702, 702)]  # band 0: two
    assert _slot(got, 2, 0) == (40, 3, 0, 40, 100, 100) and inst.host(awfm, band=2)["votes"][2, 0] == 4  # four votes, three anchors


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", ["lengths", "fixed", "one-sequence"])
def test_random_batches_equal_the_restatement(awfm, seed, shape):
    inst = rc.random_instance(seed, with_sequences=shape != "one-sequence", fixed_length=0 if shape == "lengths" else 20)
    for params, slots in ((dict(band=0), 4), (dict(band=4, max_hits_per_seed=4, lookback=3, gap_penalty=1), 2),
                          (dict(band=1 << 20, gap_penalty=0, lookback=64), 16), (dict(band=3, lookback=1, threads=1), 1)):
        case = ch.candidate_case(awfm, inst, params["band"], slots, max_hits_per_seed=params.get("max_hits_per_seed", 0))
        want = ch.expected(case, **{k: v for k, v in params.items() if k != "threads"})
        assert want["chainAnchors"].max() > 1 or params["band"] == 0
        ch.assert_equal(case.host(awfm, **params), want, what=str(params))


def test_small_slots_equal_the_best_of_all_chains(awfm):
    """the recurrence against brute force: every order-respecting subsequence with compatible neighbours, for slots of at most
    10 anchors and a lookback that reaches all of them"""
    rng = np.random.default_rng(10)
    reads = []
    for _ in range(150):
        loci = [(int(rng.integers(0, 2)), int(rng.integers(0, 1 << 20))) for _ in range(2)]
        read = []
        for _ in range(int(rng.integers(1, 15))):
            length = int(rng.integers(0, 30))
            sequence, diagonal = loci[int(rng.integers(0, 2))]
            read.append(ch.anchor(length + int(rng.integers(0, 60)), length, diagonal + int(rng.integers(0, 4)), sequence))
        reads.append(read)
    inst = rc.from_reads(reads)
    checked = 0
    for band, gap_penalty, lookback in ((3, 0, 10), (3, 2, 64), (1, 1, 11)):
        case = ch.candidate_case(awfm, inst, band, 3)
        got = case.host(awfm, band=band, gap_penalty=gap_penalty, lookback=lookback)
        for r in range(inst.num_reads):
            kept = ch.kept_hits(inst, r, 0)
            for j in range(case.slots):
                if case.sequences[r, j] == ch.NONE:
                    continue
                anchors = ch.slot_anchors(kept, int(case.sequences[r, j]), int(case.diagonals[r, j]), int(case.spans[r, j]))
                if 0 < len(anchors) <= 10:
                    assert got["chainScores"][r, j] == ch.brute_force_score(anchors, band, gap_penalty), (r, j, anchors)
                    checked += len(anchors) > 2
    assert checked > 100


def test_dropped_seeds_between_kept_ones(awfm):
    inst = rc.dropped_seeds_instance()
    for max_hits in (16, 64, 0):
        case = ch.candidate_case(awfm, inst, 7, 8, max_hits_per_seed=max_hits)
        params = dict(band=7, max_hits_per_seed=max_hits, gap_penalty=1)
        want = ch.expected(case, **params)
        assert want["keptHits"][1] == (0 if max_hits else 5000) and want["numOverflowed"] == (0 if max_hits else 1)
        ch.assert_equal(case.host(awfm, **params), want, what=str(max_hits))


@pytest.mark.parametrize("with_sequences", [True, False], ids=["sequences", "one-sequence"])
def test_many_reads_on_the_thread_pool_equal_the_restatement(awfm, with_sequences):
    """6000 reads: above the 4096 items from which awfmParallelFor spreads a loop over its threads, so that the per-thread
    counters of overflowed reads and the threads' own buffers are what is compared"""
    inst = rc.many_small_reads_instance(with_sequences=with_sequences)
    case = ch.candidate_case(awfm, inst, 7, 3, max_hits_per_seed=8)
    inst.offsets = inst.offsets.copy()
    inst.offsets[[100, 3000, 5999]] = np.uint64(1) << np.uint64(40)  # malformed reads in several threads' parts: reads 99, 100, 2999, ...
    params = dict(band=7, max_hits_per_seed=8, gap_penalty=1, lookback=16)
    want = ch.expected(case, overflowed_before=5, **params)
    assert want["numOverflowed"] == 5 + 6 and want["chainAnchors"].max() > 2
    for threads in (4, 16):
        ch.assert_equal(case.host(awfm, threads=threads, overflowed_before=5, **params), want, what=str(threads))


def test_malformed_reads_are_reported_and_nothing_else_is_read(awfm):
    inst = rc.malformed_instance()
    good = rc.Instance(inst.offsets[:2], inst.seed_ends, [0, 2, 4, 4, 5, 5, 6], inst.positions, inst.sequences, fixed_length=20)
    slots = good.host(awfm, band=4, max_candidates=4)  # the slots of the well-formed first read, for every read
    n = inst.num_reads
    case = ch.Case(inst, np.repeat(slots["sequences"], n, 0), np.repeat(slots["diagonals"], n, 0), np.repeat(slots["diagonalSpans"], n, 0))
    want = ch.expected(case, band=4, overflowed_before=7)
    assert [r for r in range(n) if want["keptHits"][r] == ch.MALFORMED] == list(rc.MALFORMED_READS)
    assert want["numOverflowed"] == 7 + len(rc.MALFORMED_READS)  # added to, not set
    got = case.host(awfm, band=4, overflowed_before=7, fill=0x5A)
    ch.assert_equal(got, want)
    assert _slot(got, 0) == (24, 2, 0, 24, 100, 100) and _slot(got, 1) == (0,) * 6 and got["bestSlots"][1] == ch.NO_SLOT
    case = ch.intersecting_case()
    want = ch.expected(case, band=20, overflowed_before=1)
    assert [r for r in range(5) if want["keptHits"][r] == ch.MALFORMED] == list(ch.INTERSECTING_READS) and want["numOverflowed"] == 4
    got = case.host(awfm, band=20, overflowed_before=1, fill=0x5A)
    ch.assert_equal(got, want)
    assert _slot(got, 0, 0) == (20, 1, 0, 20, 100, 100) and _slot(got, 0, 1) == (20, 1, 10, 30, 111, 111) and _slot(got, 3, 1) == (0,) * 6


@pytest.mark.parametrize("missing", [None] + list(ch.FIELDS))
def test_every_output_may_be_null(awfm, edge, missing):
    """each output NULL in turn, and all of them but one"""
    case = _edge_case(awfm, edge, ch.EDGE_BAND, 3)
    params = dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=ch.EDGE_BAND, gap_penalty=1)
    want = ch.expected(case, **params)
    for outputs in ([f for f in ch.FIELDS if f != missing], [missing] if missing else []):
        got = case.host(awfm, outputs=outputs, **params)
        assert sorted(got) == sorted(outputs)
        ch.assert_equal(got, want, names=outputs)


def test_error_codes(awfm):
    from avxwindowfmindex_amd import _lib
    inst = rc.random_instance(5, reads=4)
    case = ch.candidate_case(awfm, inst, 3, 4)
    null_ptr = -4
    for bad in (dict(lookback=0), dict(lookback=65)):
        with pytest.raises(awfm.AwFmError) as err:
            case.host(awfm, **bad)
        assert err.value.rc == _lib.AwFmIllegalPositionError
    L = _lib.lib()
    cin = awfm.candidate_inputs(inst.offsets.ctypes.data, inst.num_seeds, inst.seed_ends.ctypes.data, 0, 20, inst.hit_offsets.ctypes.data,
                                inst.num_hits, inst.positions.ctypes.data, 0)
    cout = awfm.chain_outputs()
    slots = [case.sequences.ctypes.data, case.diagonals.ctypes.data, case.spans.ctypes.data]

    def call(inputs, n, slot_count, arrays, lookback=64):
        return L.awfmReadChains(C.byref(inputs), n, 0, 3, slot_count, arrays[0], arrays[1], arrays[2], lookback, 0, C.byref(cout), 1)

    assert call(cin, 4, 4, slots) == _lib.AwFmSuccess  # every output NULL
    assert call(cin, 1 << 32, 4, slots) == _lib.AwFmIllegalPositionError
    assert call(cin, 4, 0, slots) == _lib.AwFmIllegalPositionError and call(cin, 4, 17, slots) == _lib.AwFmIllegalPositionError
    for k in range(3):  # a missing slot array
        assert call(cin, 4, 4, [None if i == k else a for i, a in enumerate(slots)]) == null_ptr, k
    for field in ("readSeedOffsets", "seedEnds", "hitOffsets", "positions"):
        broken = awfm.candidate_inputs(inst.offsets.ctypes.data, inst.num_seeds, inst.seed_ends.ctypes.data, 0, 20,
                                       inst.hit_offsets.ctypes.data, inst.num_hits, inst.positions.ctypes.data, 0)
        setattr(broken, field, None)
        assert call(broken, 4, 4, slots) == null_ptr, field
    broken = awfm.candidate_inputs(inst.offsets.ctypes.data, inst.num_seeds, inst.seed_ends.ctypes.data, 0, 0, inst.hit_offsets.ctypes.data,
                                   inst.num_hits, inst.positions.ctypes.data, 0)
    assert call(broken, 4, 4, slots) == null_ptr  # neither lengths nor a fixed length
    assert L.awfmReadChains(None, 0, 0, 0, 99, None, None, None, 0, 0, None, 1) == _lib.AwFmSuccess  # no reads: nothing is looked at


def test_end_to_end_on_the_host_chains_every_planted_read(awfm, tmp_path):
    lengths = lp.record_lengths(43, count=200, longest=1500)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    reads, planted = rc.planted_reads(records)
    inst = rc.host_pipeline(awfm, ix, reads)
    case = ch.candidate_case(awfm, inst, 2, 4, max_hits_per_seed=rc.E2E_MAX_HITS, min_votes=2)
    params = dict(max_hits_per_seed=rc.E2E_MAX_HITS, band=2, gap_penalty=1)
    got = case.host(awfm, **params)
    ch.assert_equal(got, ch.expected(case, **params))
    # the longest window is 64 characters: what a chain may miss at either end is less than one seed
    ch.assert_planted_reads_chained(got, case, planted, rc.E2E_CAP)
    for r, plant in enumerate(planted):
        if plant is not None and plant[2]:  # the deletion: one chain whose diagonal moves by one
            j = int(got["bestSlots"][r])
            assert got["chainEndDiagonals"][r, j] - got["chainBeginDiagonals"][r, j] == 1, (r, plant)
    ix.dealloc()


SANITIZER_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include "awfm_gpu.h"
/* arrays from a file of little-endian words (each array in a malloc block of exactly its size, so that a read one past it is seen):
 * the call's outputs to stdout */
static void *block(FILE *f, size_t bytes) {
  void *p = malloc(bytes ? bytes : 1);
  if (bytes && fread(p, 1, bytes, f) != bytes) exit(2);
  return p;
}
int main(int argc, char **argv) {
  FILE *f = argc < 2 ? NULL : fopen(argv[1], "rb");
  if (!f) return 2;
  uint64_t h[14];
  if (fread(h, 8, 14, f) != 14) return 2;
  const uint64_t numReads = h[0], sizeSeeds = h[1], sizeHits = h[2], slots = h[9];
  struct AwFmCandidateInputs in = {0};
  in.numSeeds = h[3];
  in.numHits = h[4];
  in.fixedLength = (uint32_t)h[5];
  in.readSeedOffsets = block(f, (numReads + 1) * 8);
  in.seedEnds = block(f, sizeSeeds * 4);
  in.seedLengths = h[5] ? NULL : block(f, sizeSeeds * 4);
  in.hitOffsets = block(f, (sizeSeeds + 1) * 8);
  in.positions = block(f, sizeHits * 8);
  in.sequenceNumbers = h[10] ? block(f, sizeHits * 4) : NULL;
  const uint32_t *sequences = block(f, numReads * slots * 4);
  const int64_t *diagonals = block(f, numReads * slots * 8);
  const uint32_t *spans = block(f, numReads * slots * 4);
  uint64_t overflowed = h[11];
  struct AwFmChainOutputs out = {malloc(numReads * slots * 4), malloc(numReads * slots * 4), malloc(numReads * slots * 4),
                                 malloc(numReads * slots * 4), malloc(numReads * slots * 8), malloc(numReads * slots * 8),
                                 malloc(numReads * 4),         malloc(numReads * 4),         &overflowed};
  const int rc = awfmReadChains(&in, numReads, (uint32_t)h[6], (uint32_t)h[7], (uint32_t)slots, sequences, diagonals, spans, (uint32_t)h[8],
                                (uint32_t)h[13], &out, (unsigned)h[12]);
  if (rc != AwFmSuccess) return 3;
  fwrite(out.chainScores, 4, numReads * slots, stdout);
  fwrite(out.chainAnchors, 4, numReads * slots, stdout);
  fwrite(out.chainReadBegins, 4, numReads * slots, stdout);
  fwrite(out.chainReadEnds, 4, numReads * slots, stdout);
  fwrite(out.chainBeginDiagonals, 8, numReads * slots, stdout);
  fwrite(out.chainEndDiagonals, 8, numReads * slots, stdout);
  fwrite(out.bestSlots, 4, numReads, stdout);
  fwrite(out.keptHits, 4, numReads, stdout);
  fwrite(&overflowed, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(awfm, tmp_path):
    """the twin indexes arrays by offsets and slots its caller supplies: awfm_chains.c and the thread pool it runs on, compiled
    with a stand-alone main under -fsanitize=address,undefined, run on the edge list, on the hand-made and the intersecting
    slots, on the malformed reads and on 6000 reads spread over four threads of the pool (every array in a heap block of exactly
    its size)"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "chains_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_chains.c"), os.path.join(CSRC, "awfm_threads.c"), "-o", exe])
    edge = ch.edge_instance()
    bad = rc.malformed_instance()
    bad_slots = np.tile(np.array([[0, 1]], np.uint32), (bad.num_reads, 1))
    many = rc.many_small_reads_instance(with_sequences=False)
    cases = (("edge", ch.candidate_case(awfm, edge, ch.EDGE_BAND, 16, max_hits_per_seed=ch.EDGE_MAX_HITS),
              dict(max_hits_per_seed=ch.EDGE_MAX_HITS, band=ch.EDGE_BAND, gap_penalty=1)),
             ("edge-wide", ch.candidate_case(awfm, edge, 0xFFFFFFFF, 1), dict(band=0xFFFFFFFF, gap_penalty=0xFFFFFFFF, lookback=2)),
             ("hand-made", ch.lookback_case(), dict(band=5)),
             ("intersecting", ch.intersecting_case(), dict(band=20, overflowed_before=2)),
             ("malformed", ch.Case(bad, bad_slots, np.full(bad_slots.shape, 100), np.full(bad_slots.shape, 300)), dict(band=4, overflowed_before=3)),
             # 6000 reads on four threads of the pool, without sequence numbers
             ("many", ch.candidate_case(awfm, many, 7, 2, max_hits_per_seed=8), dict(band=7, max_hits_per_seed=8, lookback=9, threads=4)))
    for name, case, params in cases:
        inst, n, slots = case.inst, case.inst.num_reads, case.slots
        header = np.array([n, len(inst.seed_ends), len(inst.positions), inst.num_seeds, inst.num_hits, inst.fixed_length,
                           params.get("max_hits_per_seed", 0), params["band"], params.get("lookback", 64), slots, inst.sequences is not None,
                           params.get("overflowed_before", 0), params.pop("threads", 2), params.get("gap_penalty", 0)], np.uint64)
        arrays = [header, inst.offsets, inst.seed_ends] + ([inst.seed_lengths] if not inst.fixed_length else []) + [inst.hit_offsets, inst.positions]
        arrays += [inst.sequences] if inst.sequences is not None else []
        arrays += [case.sequences, case.diagonals, case.spans]
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, (name, run.stderr.decode(errors="replace")[-3000:])
        want = ch.expected(case, **params)
        at = 0
        for field in ch.SLOT_FIELDS + ch.READ_FIELDS:
            count = n * slots if field in ch.SLOT_FIELDS else n
            got = np.frombuffer(run.stdout, ch.DTYPES[field], count, at)
            at += got.nbytes
            assert np.array_equal(got, want[field].reshape(-1)), (name, field)
        assert int(np.frombuffer(run.stdout, np.uint64, 1, at)[0]) == want["numOverflowed"]
