"""awfmReadCandidates (include/awfm_gpu.h "candidate loci", csrc/awfm_candidates.c): the host twin against the NumPy restatement
of the definition (tests/read_candidates_common.py) on random batches and on the edge list, every output and the NULL-output
combinations; hand-written expectations for the entries of the edge list, so that the restatement is pinned too; the error
codes; end to end from a FASTA file; and the twin under AddressSanitizer + UBSan as a stand-alone program."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402
import read_candidates_common as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "avxwindowfmindex_amd", "csrc")

# (band, minVotes, C) on top of the edge list's own band and maxHitsPerSeed
EDGE_PARAMS = [(rc.EDGE_BAND, 1, 4), (rc.EDGE_BAND, 0, 1), (rc.EDGE_BAND, 2, 16), (0, 1, 16), (0xFFFFFFFF, 1, 3), (rc.EDGE_BAND, 5000, 4)]


@pytest.fixture(scope="module")
def edge():
    return rc.edge_instance()


@pytest.mark.parametrize("band,min_votes,slots", EDGE_PARAMS)
def test_edge_list_equals_the_restatement(awfm, edge, band, min_votes, slots):
    params = dict(max_hits_per_seed=rc.EDGE_MAX_HITS, band=band, min_votes=min_votes, max_candidates=slots)
    want = rc.expected(edge, **params)
    rc.assert_equal(edge.host(awfm, **params), want)
    assert want["numOverflowed"] == 1
    if min_votes == 5000:
        assert not want["numCandidates"].any() and (want["sequences"] == rc.NONE).all()


def _slots(result, r):
    """read r's stored candidates as tuples (sequence, diagonal, votes, span, begin, end)"""
    n = int((result["sequences"][r] != rc.NONE).sum())
    return [tuple(int(result[name][r, j]) for name in rc.SLOT_FIELDS) for j in range(n)]


def test_edge_list_by_hand(awfm, edge):
    """what the definition says of each entry, written out: pins the restatement as well as the twin"""
    at = rc.EDGE_READS
    got = edge.host(awfm, max_hits_per_seed=rc.EDGE_MAX_HITS, band=rc.EDGE_BAND, min_votes=1, max_candidates=16, fill=0xA5)
    none = (rc.NONE, 0, 0, 0, 0, 0)
    for name in ("no seeds", "seeds without hits"):
        assert _slots(got, at[name]) == [] and got["keptHits"][at[name]] == 0 and got["numCandidates"][at[name]] == 0
        assert tuple(int(got[f][at[name], 15]) for f in rc.SLOT_FIELDS) == none  # the fill of an unused slot, over the 0xA5
    assert _slots(got, at["one hit"]) == [(2, 777, 1, 0, 0, 20)]
    assert _slots(got, at["one diagonal"]) == [(1, 1000, 5, 0, 0, 36)]
    assert _slots(got, at["gaps of band"]) == [(0, 100, 3, 10, 0, 28)]
    assert _slots(got, at["gaps of band + 1"]) == [(0, 100, 1, 0, 0, 20), (0, 106, 1, 0, 4, 24)]
    assert _slots(got, at["neighbouring sequences"]) == [(3, 50, 2, 0, 0, 22), (4, 50, 2, 0, 0, 22)]
    assert _slots(got, at["negative diagonals"]) == [(0, -5, 3, 6, 5, 30)]
    assert _slots(got, at["across 2^32"])[0] == (0, (1 << 32) - 2, 2, 4, 0, 30)
    assert _slots(got, at["ties"]) == [(1, 100, 2, 0, 0, 24), (1, 900, 2, 0, 0, 24), (2, 500, 2, 0, 0, 24)]
    assert got["numCandidates"][at["more than C"]] == 20 and len(_slots(got, at["more than C"])) == 16
    # the seed of three hits is kept, the seed of four is not
    assert got["keptHits"][at["at and above maxHitsPerSeed"]] == 3 and got["numCandidates"][at["at and above maxHitsPerSeed"]] == 3
    assert _slots(got, at["length beyond seedEnd"]) == [(0, 60, 1, 0, 0, 20)]
    assert _slots(got, at["illegal hits in between"]) == [(1, 300, 2, 0, 0, 24)]
    assert _slots(got, at["zero length"]) == [(0, 30, 2, 0, 0, 20)]  # anchor 20 and anchor 0: both on diagonal 30
    assert got["keptHits"][at["4096 kept hits"]] == 4096 and got["numCandidates"][at["4096 kept hits"]] > 16
    r = at["4097 kept hits"]
    assert got["keptHits"][r] == 4097 and got["numCandidates"][r] == 0 and _slots(got, r) == [] and got["numOverflowed"] == 1
    assert _slots(got, at["after the overflow"]) == [(5, 123, 1, 0, 0, 20)]
    wide = edge.host(awfm, max_hits_per_seed=rc.EDGE_MAX_HITS, band=0xFFFFFFFF, max_candidates=1)
    # band 2^32 - 1 chains 10, 2^32 - 1 + 10 and 2^33 - 2 + 10 of sequence 9: three votes, the span saturated
    assert _slots(wide, at["across 2^32"]) == [(9, 10, 3, 0xFFFFFFFF, 0, 20)]
    # C = 1 keeps the best of the ties
    assert _slots(edge.host(awfm, max_hits_per_seed=3, band=5, max_candidates=1), at["ties"]) == [(1, 100, 2, 0, 0, 24)]
    # without the repeat filter the seed of four hits votes too
    assert edge.host(awfm, band=5)["keptHits"][at["at and above maxHitsPerSeed"]] == 7


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("shape", ["lengths", "fixed", "one-sequence"])
def test_random_batches_equal_the_restatement(awfm, seed, shape):
    inst = rc.random_instance(seed, with_sequences=shape != "one-sequence", fixed_length=0 if shape == "lengths" else 20)
    for params in (dict(band=0), dict(band=4, min_votes=2, max_candidates=2, max_hits_per_seed=4), dict(band=1 << 20, max_candidates=16),
                   dict(band=3, min_votes=3, max_candidates=1, threads=1)):
        want = rc.expected(inst, **{k: v for k, v in params.items() if k != "threads"})
        assert want["numCandidates"].max() > params.get("max_candidates", 4) or params.get("min_votes", 1) > 1
        rc.assert_equal(inst.host(awfm, **params), want, what=str(params))


def test_dropped_seeds_between_kept_ones(awfm):
    inst = rc.dropped_seeds_instance()
    for max_hits in (16, 64, 0):
        params = dict(band=7, max_candidates=8, max_hits_per_seed=max_hits)
        want = rc.expected(inst, **params)
        assert want["keptHits"][1] == (0 if max_hits else 5000) and want["numOverflowed"] == (0 if max_hits else 1)
        rc.assert_equal(inst.host(awfm, **params), want, what=str(max_hits))


@pytest.mark.parametrize("with_sequences", [True, False], ids=["sequences", "one-sequence"])
def test_many_reads_on_the_thread_pool_equal_the_restatement(awfm, with_sequences):
    """6000 reads: above the 4096 items from which awfmParallelFor spreads a loop over its threads, so that the per-thread
    counters of overflowed reads and the threads' own buffers are what is compared"""
    inst = rc.many_small_reads_instance(with_sequences=with_sequences)
    inst.offsets = inst.offsets.copy()
    inst.offsets[[100, 3000, 5999]] = np.uint64(1) << np.uint64(40)  # malformed reads in several threads' parts: reads 99, 100, 2999, ...
    for threads in (4, 16):
        params = dict(band=7, max_candidates=3, max_hits_per_seed=7)
        want = rc.expected(inst, overflowed_before=5, **params)
        assert want["numOverflowed"] == 5 + 6 and want["numCandidates"].max() > 3
        rc.assert_equal(inst.host(awfm, threads=threads, overflowed_before=5, **params), want, what=str(threads))


def test_malformed_reads_are_reported_and_nothing_else_is_read(awfm):
    inst = rc.malformed_instance()
    want = rc.expected(inst, band=4, overflowed_before=7)
    assert [r for r in range(inst.num_reads) if want["keptHits"][r] == rc.MALFORMED] == list(rc.MALFORMED_READS)
    assert want["numOverflowed"] == 7 + len(rc.MALFORMED_READS)  # added to, not set
    got = inst.host(awfm, band=4, overflowed_before=7, fill=0x5A)
    rc.assert_equal(got, want)
    assert _slots(got, 0)[0] == (0, 100, 2, 0, 0, 24) and _slots(got, 2)[0] == (1, 300, 1, 0, 0, 20) and _slots(got, 1) == []


@pytest.mark.parametrize("outputs", [["numCandidates"], ["sequences", "diagonals", "votes", "diagonalSpans", "numOverflowed"], ["readBegins"],
                                     ["readEnds", "keptHits"], [f for f in rc.FIELDS if f != "numOverflowed"]])
def test_every_output_may_be_null(awfm, edge, outputs):
    params = dict(max_hits_per_seed=rc.EDGE_MAX_HITS, band=rc.EDGE_BAND, max_candidates=3)
    got = edge.host(awfm, outputs=outputs, **params)
    assert sorted(got) == sorted(outputs)
    rc.assert_equal(got, rc.expected(edge, **params), names=outputs)


def test_error_codes(awfm):
    from avxwindowfmindex_amd import _lib
    inst = rc.random_instance(5, reads=4)
    null_ptr = -4
    for bad, code in ((dict(max_candidates=0), _lib.AwFmIllegalPositionError), (dict(max_candidates=17), _lib.AwFmIllegalPositionError)):
        with pytest.raises(awfm.AwFmError) as err:
            inst.host(awfm, **bad)
        assert err.value.rc == code
    with pytest.raises(awfm.AwFmError) as err:  # neither lengths nor a fixed length
        awfm.read_candidates_host(inst.offsets, inst.seed_ends, inst.hit_offsets, inst.positions, inst.sequences)
    assert err.value.rc == null_ptr
    L = _lib.lib()
    cin = awfm.candidate_inputs(inst.offsets.ctypes.data, inst.num_seeds, inst.seed_ends.ctypes.data, 0, 20, inst.hit_offsets.ctypes.data,
                                inst.num_hits, inst.positions.ctypes.data, 0)
    cout = awfm.candidate_outputs()
    import ctypes as C
    assert L.awfmReadCandidates(C.byref(cin), 1 << 32, 0, 0, 1, 4, C.byref(cout), 1) == _lib.AwFmIllegalPositionError
    assert L.awfmReadCandidates(C.byref(cin), 4, 0, 0, 1, 4, C.byref(cout), 1) == _lib.AwFmSuccess  # every output NULL
    for field in ("readSeedOffsets", "seedEnds", "hitOffsets", "positions"):
        broken = awfm.candidate_inputs(inst.offsets.ctypes.data, inst.num_seeds, inst.seed_ends.ctypes.data, 0, 20,
                                       inst.hit_offsets.ctypes.data, inst.num_hits, inst.positions.ctypes.data, 0)
        setattr(broken, field, None)
        assert L.awfmReadCandidates(C.byref(broken), 4, 0, 0, 1, 4, C.byref(cout), 1) == null_ptr, field
    assert L.awfmReadCandidates(None, 0, 0, 0, 1, 99, None, 1) == _lib.AwFmSuccess  # no reads: nothing is looked at


def test_end_to_end_on_the_host_finds_every_planted_read(awfm, tmp_path):
    lengths = lp.record_lengths(43, count=200, longest=1500)
    fa = tmp_path / "records.fa"
    records = lp.write_fasta(str(fa), lengths, lp.DNA_LETTERS, 13)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, 8, file_src=str(tmp_path / "records.awfmi"))
    reads, planted = rc.planted_reads(records)
    inst = rc.host_pipeline(awfm, ix, reads)
    assert inst.num_hits > 300  # 40 planted reads, nine or more windows of 14 matching characters and more in each
    by_band = {}
    for band in (2, 0):
        # minVotes = 2: a lone chance occurrence of a 14-mer is no locus, whereas each side of a deletion holds the windows of a
        # whole stretch of 29 matching characters
        params = dict(max_hits_per_seed=rc.E2E_MAX_HITS, band=band, min_votes=2, max_candidates=4)
        got = by_band[band] = inst.host(awfm, **params)
        rc.assert_equal(got, rc.expected(inst, **params))
        assert got["numOverflowed"] == 0 and got["keptHits"].max() <= 30 * rc.E2E_MAX_HITS
    rc.assert_planted_reads_found(by_band[2], planted, 2)  # every planted read, the ones with a deletion included
    for r, plant in enumerate(planted):
        if plant is None:
            continue
        record, at, deleted = plant
        if not deleted:
            assert by_band[0]["sequences"][r, 0] == record and by_band[0]["diagonals"][r, 0] == at
            continue
        assert by_band[2]["numCandidates"][r] == 1 and by_band[0]["numCandidates"][r] == 2, (r, plant)
        assert (by_band[0]["sequences"][r, :2] == record).all() and sorted(by_band[0]["diagonals"][r, :2].tolist()) == [at, at + 1]
        assert by_band[2]["diagonals"][r, 0] == at and by_band[2]["diagonalSpans"][r, 0] == 1
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
  FILE *f = fopen(argv[1], "rb");
  if (argc < 2 || !f) return 2;
  uint64_t h[13];
  if (fread(h, 8, 13, f) != 13) return 2;
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
  uint64_t overflowed = h[11];
  struct AwFmCandidateOutputs out = {malloc(numReads * slots * 4), malloc(numReads * slots * 8), malloc(numReads * slots * 4),
                                     malloc(numReads * slots * 4), malloc(numReads * slots * 4), malloc(numReads * slots * 4),
                                     malloc(numReads * 4),         malloc(numReads * 4),         &overflowed};
  const int rc = awfmReadCandidates(&in, numReads, (uint32_t)h[6], (uint32_t)h[7], (uint32_t)h[8], (uint32_t)slots, &out, (unsigned)h[12]);
  if (rc != AwFmSuccess) return 3;
  fwrite(out.sequences, 4, numReads * slots, stdout);
  fwrite(out.diagonals, 8, numReads * slots, stdout);
  fwrite(out.votes, 4, numReads * slots, stdout);
  fwrite(out.diagonalSpans, 4, numReads * slots, stdout);
  fwrite(out.readBegins, 4, numReads * slots, stdout);
  fwrite(out.readEnds, 4, numReads * slots, stdout);
  fwrite(out.numCandidates, 4, numReads, stdout);
  fwrite(out.keptHits, 4, numReads, stdout);
  fwrite(&overflowed, 8, 1, stdout);
  return 0;
}
"""


def test_host_twin_under_address_and_undefined_sanitizers(tmp_path):
    """the twin indexes arrays by offsets its caller supplies: awfm_candidates.c and the thread pool it runs on, compiled with a
    stand-alone main under -fsanitize=address,undefined, run on the edge list, on the malformed reads and on 6000 reads spread over
    four threads of the pool (every array in a heap block of exactly its size)"""
    (tmp_path / "main.c").write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "candidates_asan")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, str(tmp_path / "main.c"),
                           os.path.join(CSRC, "awfm_candidates.c"), os.path.join(CSRC, "awfm_threads.c"), "-o", exe])
    for name, inst, params in (("edge", rc.edge_instance(), dict(max_hits_per_seed=rc.EDGE_MAX_HITS, band=rc.EDGE_BAND, max_candidates=16)),
                               ("edge-wide", rc.edge_instance(), dict(band=0xFFFFFFFF, max_candidates=1)),
                               ("malformed", rc.malformed_instance(), dict(band=4, max_candidates=4, overflowed_before=3)),
                               # 6000 reads on four threads of the pool, without sequence numbers
                               ("many", rc.many_small_reads_instance(with_sequences=False), dict(band=7, max_candidates=2, max_hits_per_seed=7, threads=4))):
        n, slots = inst.num_reads, params["max_candidates"]
        header = np.array([n, len(inst.seed_ends), len(inst.positions), inst.num_seeds, inst.num_hits, inst.fixed_length,
                           params.get("max_hits_per_seed", 0), params["band"], 1, slots, inst.sequences is not None,
                           params.get("overflowed_before", 0), params.pop("threads", 2)], np.uint64)
        arrays = [header, inst.offsets, inst.seed_ends] + ([inst.seed_lengths] if not inst.fixed_length else []) + [inst.hit_offsets, inst.positions]
        arrays += [inst.sequences] if inst.sequences is not None else []
        (tmp_path / name).write_bytes(b"".join(a.tobytes() for a in arrays))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
        run = subprocess.run([exe, str(tmp_path / name)], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
        want = rc.expected(inst, **params)
        at = 0
        for field in rc.SLOT_FIELDS + rc.READ_FIELDS:
            count = n * slots if field in rc.SLOT_FIELDS else n
            got = np.frombuffer(run.stdout, rc.DTYPES[field], count, at)
            at += got.nbytes
            assert np.array_equal(got, want[field].reshape(-1)), (name, field)
        assert int(np.frombuffer(run.stdout, np.uint64, 1, at)[0]) == want["numOverflowed"]
