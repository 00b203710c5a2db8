"""Shared by the tests of the batch mapping global text position -> (sequence number, local position): the FASTA fixtures and
the checker.  The checker is a NumPy restatement of the definition in include/awfm_gpu.h ("sequence coordinates"), never the
code under test: with the records' ends E and starts S[0] = 0, S[r] = E[r-1] + 1, position p belongs to the first r with
E[r] > p when p >= S[r]; every other position is illegal (sequence 0xFFFFFFFF, position kept)."""
import numpy as np

ILLEGAL = 0xFFFFFFFF
DNA_LETTERS = np.frombuffer(b"acgt", np.uint8)
AMINO_LETTERS = np.frombuffer(b"acdefghiklmnpqrstvwy", np.uint8)


def record_lengths(seed, count=320, longest=2500):
    """lengths 0 (first, last, two in a row at the start, a run of five in the middle), 1, and up to `longest`"""
    rng = np.random.default_rng(seed)
    kind = rng.random(count)
    lengths = np.where(kind < 0.12, 0, np.where(kind < 0.25, 1, rng.integers(2, 400, count)))
    lengths[rng.integers(0, count, 12)] = rng.integers(longest // 2, longest + 1, 12)
    lengths[0] = lengths[1] = 0
    lengths[count // 2:count // 2 + 5] = 0
    lengths[count // 3] = 1
    lengths[count // 3 + 1] = longest
    lengths[-1] = 0
    return lengths.astype(np.int64)


def ends_of(lengths):
    """sequenceEndPosition of every record: its residues end there, its terminator sits there"""
    lengths = np.asarray(lengths, np.uint64)
    return (np.cumsum(lengths) + np.arange(len(lengths), dtype=np.uint64)).astype(np.uint64)


def write_fasta(path, lengths, letters, seed):
    """one record per length (an empty record is a header without residues); returns the records' residues"""
    rng = np.random.default_rng(seed)
    records = [letters[rng.integers(0, len(letters), int(n))].tobytes() for n in lengths]
    with open(path, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">r%d len %d\n" % (i, len(r)))
            for j in range(0, len(r), 70):
                f.write(r[j:j + 70] + b"\n")
    return records


def expected(ends, positions):
    """(sequence uint32[n], local uint64[n], number of illegal positions) by the definition"""
    ends = np.asarray(ends, np.uint64)
    p = np.asarray(positions, np.uint64)
    starts = np.concatenate([np.zeros(1, np.uint64), ends[:-1] + np.uint64(1)])
    r = np.searchsorted(ends, p, side="right")  # first record whose end is beyond p
    inside = r < len(ends)
    rr = np.minimum(r, len(ends) - 1)
    legal = inside & (p >= starts[rr])
    seq = np.where(legal, rr, ILLEGAL).astype(np.uint32)
    local = np.where(legal, p - starts[rr], p).astype(np.uint64)
    return seq, local, int((~legal).sum())
