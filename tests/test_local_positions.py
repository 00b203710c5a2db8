"""awfmLocalPositions (include/awfm_gpu.h, csrc/awfm_fasta.c): the batch form of awFmGetLocalSequencePositionFromIndexPosition
(ref src/AwFmSearch.c:284-301) on the host.  Expected values: the NumPy restatement of the definition
(local_positions_common.expected), cross-checked on a sample against the single-position function, which is older than
the batch form."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402

TEST2_FA = ">t\nacdef\n>v\ng\n>w\nhikl\n>y\nm\n"  # the reference's test/multiSequenceIndexTest/test2.fa, as in test_fasta.py


def _fixture(awfm, tmp_path, amino):
    lengths = lp.record_lengths(31 if amino else 17)
    assert len(lengths) >= 300 and lengths[0] == 0 and lengths[1] == 0 and lengths[-1] == 0 and (lengths == 1).any()
    fa = tmp_path / ("amino.fa" if amino else "dna.fa")
    lp.write_fasta(str(fa), lengths, lp.AMINO_LETTERS if amino else lp.DNA_LETTERS, 5)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 4, 2 if amino else 4,
                                      file_src=str(fa) + ".awfmi")
    ends = lp.ends_of(lengths)
    assert ix.bwt_length == int(ends[-1]) + 2  # residues and terminators, then the sentinel
    return ix, ends


def _single(awfm, ix, p):
    """what the single-position function says: (sequence, local), or None for an illegal position"""
    try:
        return ix.local_position(int(p))
    except awfm.AwFmError as e:
        assert e.rc == awfm.AwFmIllegalPositionError
        return None


@pytest.mark.parametrize("amino", [False, True], ids=["dna", "amino"])
def test_every_position_matches_the_definition(awfm, tmp_path, amino):
    ix, ends = _fixture(awfm, tmp_path, amino)
    positions = np.arange(ix.bwt_length + 1, dtype=np.uint64)  # 0 .. bwtLength inclusive
    want_seq, want_local, want_illegal = lp.expected(ends, positions)
    # every terminator and everything from the last end on is illegal, nothing else
    illegal_at = set(np.flatnonzero(want_seq == lp.ILLEGAL).tolist())
    assert illegal_at == set(ends.tolist()) | set(range(int(ends[-1]), ix.bwt_length + 1))
    seq, local, illegal = awfm.local_positions_host(ix, positions, threads=4)
    assert seq.dtype == np.uint32 and local.dtype == np.uint64
    assert np.array_equal(seq, want_seq) and np.array_equal(local, want_local) and illegal == want_illegal
    assert illegal == len(illegal_at)
    # one thread gives what four give
    seq1, local1, illegal1 = awfm.local_positions_host(ix, positions, threads=1)
    assert np.array_equal(seq1, seq) and np.array_equal(local1, local) and illegal1 == illegal
    # in place
    work = positions.copy()
    seq2, local2, illegal2 = awfm.local_positions_host(ix, work, threads=4, out_local=work)
    assert local2 is work and np.array_equal(seq2, seq) and np.array_equal(work, local) and illegal2 == illegal
    # an empty batch
    seq0, local0, illegal0 = awfm.local_positions_host(ix, np.zeros(0, np.uint64))
    assert seq0.size == 0 and local0.size == 0 and illegal0 == 0
    # the checker against the function that predates the batch form, on a sample
    rng = np.random.default_rng(2)
    sample = np.concatenate([rng.integers(0, ix.bwt_length + 1, 400), ends[:40].astype(np.int64), [0, ix.bwt_length - 1, ix.bwt_length]])
    for p in sample:
        single = _single(awfm, ix, p)
        if single is None:
            assert want_seq[p] == lp.ILLEGAL and want_local[p] == p
        else:
            assert single == (int(want_seq[p]), int(want_local[p]))
    # the index read back from its file answers the same
    back = awfm.read_index_from_file(ix.file_src)
    seq3, local3, illegal3 = awfm.local_positions_host(back, positions)
    assert np.array_equal(seq3, seq) and np.array_equal(local3, local) and illegal3 == illegal
    back.dealloc()
    ix.dealloc()


def test_five_empty_records_among_two(awfm, tmp_path):
    """>a >b >c acgt >d >e >f g >g: E = [0, 1, 6, 7, 8, 10, 11]; 2..5 are record 2, 9 is record 5, everything else is illegal"""
    fa = tmp_path / "empties.fa"
    fa.write_text(">a\n>b\n>c\nacgt\n>d\n>e\n>f\ng\n>g\n")
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 2, 2)
    positions = np.arange(ix.bwt_length + 1, dtype=np.uint64)
    seq, local, illegal = awfm.local_positions_host(ix, positions)
    want_seq, want_local, want_illegal = lp.expected(np.array([0, 1, 6, 7, 8, 10, 11], np.uint64), positions)
    assert np.array_equal(seq, want_seq) and np.array_equal(local, want_local) and illegal == want_illegal
    assert seq[2:6].tolist() == [2] * 4 and local[2:6].tolist() == [0, 1, 2, 3] and (seq[9], local[9]) == (5, 0)
    assert illegal == len(positions) - 5
    ix.dealloc()


def test_terminators_of_test2_fa_are_illegal(awfm, tmp_path):
    fa = tmp_path / "test2.fa"
    fa.write_text(TEST2_FA)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetAmino, sa_ratio=2, seed_k=2)
    assert ix.bwt_length == 16
    seq, local, illegal = awfm.local_positions_host(ix, np.array([5, 7, 12, 14, 15, 16, 0, 6, 8, 13, 1], np.uint64))
    assert seq.tolist() == [lp.ILLEGAL] * 6 + [0, 1, 2, 3, 0] and local.tolist() == [5, 7, 12, 14, 15, 16, 0, 0, 0, 0, 1]
    assert illegal == 6
    ix.dealloc()


def test_index_without_a_record_table(awfm):
    plain = awfm.create_index(np.frombuffer(b"acgtacgt", np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    seq = np.full(4, 7, np.uint32)
    local = np.full(4, 9, np.uint64)
    with pytest.raises(awfm.AwFmError) as err:
        awfm.local_positions_host(plain, np.arange(4, dtype=np.uint64), out_sequence=seq, out_local=local)
    assert err.value.rc == awfm.AwFmUnsupportedVersionError
    assert (seq == 7).all() and (local == 9).all()  # nothing written
    plain.dealloc()
