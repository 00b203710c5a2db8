"""Shared by tests/test_kept_hits.py and tests/test_gpu_kept_hits.py: ONE table of reads and ONE table of refused arguments that
both units of the read path -- candidate loci and read chains -- are held to, on the host and on the device.  The kept hits of
a read (include/awfm_gpu.h, "candidate loci") are defined once for both (csrc/awfm_hits.h, csrc/awfm_hits_kernel.h); the
expectation here is the NumPy restatement of tests/read_candidates_common.py, which shares no code with the C."""
import ctypes as C

import numpy as np

import read_candidates_common as rc
import read_chains_common as ch

SUCCESS, NULL_PTR, ILLEGAL = 1, -4, -6  # AwFmSuccess, AwFmNullPtrError, AwFmIllegalPositionError (include/AwFmIndex.h)
BAND, SLOTS = rc.EDGE_BAND, 4
MAX_HITS_PER_SEED = (0, 1, rc.EDGE_MAX_HITS)
OVERFLOWED_BEFORE = 5


def instances():
    """name -> instance: the edge list (0, 1, 4096 and 4097 kept hits among them), every malformed shape, and dropped seeds that
    hold whole rounds of a wave (63 / 64 / 65 hits at a round's edge)"""
    return {"edge": rc.edge_instance(), "malformed": rc.malformed_instance(), "dropped seeds": rc.dropped_seeds_instance()}


def kept_hits_by_the_definition(inst, max_hits_per_seed):
    """-> (the keptHits word of every read, the reads that count as overflowed)"""
    words = []
    for r in range(inst.num_reads):
        kept = rc._kept_hits(inst, r, max_hits_per_seed)
        words.append(rc.MALFORMED if kept is None else min(len(kept[0]), rc.SATURATED))
    words = np.array(words, np.uint32)
    return words, int(((words == rc.MALFORMED) | (words > rc.MAX_HITS)).sum())


def host_table(awfm):
    """[(what, instance, maxHitsPerSeed, the candidates' slots as a chains case, the two twins' results)]"""
    rows = []
    for name, inst in instances().items():
        for m in MAX_HITS_PER_SEED:
            candidates = inst.host(awfm, max_hits_per_seed=m, band=BAND, max_candidates=SLOTS, overflowed_before=OVERFLOWED_BEFORE)
            case = ch.candidate_case(awfm, inst, BAND, SLOTS, max_hits_per_seed=m)  # (never intersect: no read is malformed by them)
            chains = case.host(awfm, max_hits_per_seed=m, band=BAND, overflowed_before=OVERFLOWED_BEFORE)
            rows.append((f"{name}, maxHitsPerSeed {m}", inst, m, case, candidates, chains))
    return rows


# ---- refused arguments: (what, changes to a good call, the code of BOTH calls, the device's text behind the call's name) ----
NULL_TEXT = "null argument"
LENGTHS_TEXT = "the seeds need their lengths or a fixed length"
RANGE_TEXT = "read numbers are 32-bit, and a read has 1 to 16 slots"
REFUSALS = [
    ("no inputs", dict(inputs=None), NULL_PTR, NULL_TEXT),
    ("no outputs", dict(outputs=None), NULL_PTR, NULL_TEXT),
    ("no readSeedOffsets", dict(readSeedOffsets=None), NULL_PTR, NULL_TEXT),
    ("no seedEnds", dict(seedEnds=None), NULL_PTR, NULL_TEXT),
    ("no hitOffsets", dict(hitOffsets=None), NULL_PTR, NULL_TEXT),
    ("no positions", dict(positions=None), NULL_PTR, NULL_TEXT),
    ("neither lengths nor a fixed length", dict(seedLengths=None, fixedLength=0), NULL_PTR, LENGTHS_TEXT),
    ("2^32 reads", dict(num_reads=1 << 32), ILLEGAL, RANGE_TEXT),
    ("no slots", dict(max_candidates=0), ILLEGAL, RANGE_TEXT),
    ("17 slots", dict(max_candidates=17), ILLEGAL, RANGE_TEXT),
    ("a null comes before the lengths", dict(positions=None, seedLengths=None, fixedLength=0), NULL_PTR, NULL_TEXT),
    ("the lengths come before the ranges", dict(seedLengths=None, fixedLength=0, max_candidates=17, num_reads=1 << 32), NULL_PTR, LENGTHS_TEXT),
    ("no reads: nothing is looked at", dict(inputs=None, outputs=None, num_reads=0, max_candidates=0), SUCCESS, None),
]


def refused_call(awfm, inputs, num_reads, changes):
    """a good call's arguments with `changes` -> (inputs or None, numReads, maxCandidates, whether the outputs are passed)"""
    changes = dict(changes)
    num_reads = changes.pop("num_reads", num_reads)
    max_candidates = changes.pop("max_candidates", SLOTS)
    with_outputs = changes.pop("outputs", True) is not None
    if changes.pop("inputs", True) is None:
        return None, num_reads, max_candidates, with_outputs
    fields = {name: getattr(inputs, name) for name, _ in type(inputs)._fields_}
    fields.update(changes)
    return type(inputs)(**fields), num_reads, max_candidates, with_outputs


def byref_or_null(struct):
    return C.byref(struct) if struct is not None else None
