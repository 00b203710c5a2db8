"""awfmGpuLocalPositions / awfmGpuIndexSetRecordTable / awfmGpuLocateHostLocal (include/awfm_gpu.h, csrc/awfm_gpu_records.hip):
located hits -> (sequence number, local position) on the device.  Expected values come from the host batch form
(awfmLocalPositions, itself pinned to the NumPy restatement of the definition by tests/test_local_positions.py) and from that
restatement directly where there is no host index with the table (tables installed with set_record_table)."""
import os
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import local_positions_common as lp  # noqa: E402

pytestmark = pytest.mark.gpu

TEST2_FA = ">t\nacdef\n>v\ng\n>w\nhikl\n>y\nm\n"  # the reference's test/multiSequenceIndexTest/test2.fa, as in test_fasta.py


def _fasta_index(awfm, tmp_path, amino, seed=None, count=320, sa_ratio=4, seed_k=None):
    lengths = lp.record_lengths(seed if seed is not None else (31 if amino else 17), count=count)
    fa = tmp_path / ("amino.fa" if amino else "dna.fa")
    records = lp.write_fasta(str(fa), lengths, lp.AMINO_LETTERS if amino else lp.DNA_LETTERS, 5)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, sa_ratio,
                                      seed_k if seed_k is not None else (2 if amino else 4))
    return ix, lp.ends_of(lengths), records


def _map(g, positions, torch, in_place=False, count=None, capacity=None, stream=0):
    """positions (numpy uint64) through GpuIndex.local_positions -> (seq, local, illegal) as numpy; entries past the count keep
    the fill (seq 0x77777777; local: the position itself in place, 0x55.. out of place)"""
    dev = torch.device("cuda")
    n = len(positions)
    capacity = n if capacity is None else capacity
    d_pos = torch.from_numpy(positions.view(np.int64).copy()).to(dev)
    d_seq = torch.full((n,), 0x77777777, dtype=torch.int32, device=dev)
    d_local = d_pos if in_place else torch.full((n,), 0x5555555555555555, dtype=torch.int64, device=dev)
    d_illegal = torch.zeros(1, dtype=torch.int64, device=dev)
    d_count = torch.tensor([count], dtype=torch.int64, device=dev) if count is not None else None
    torch.cuda.synchronize()
    g.local_positions(d_pos.data_ptr(), capacity, d_seq.data_ptr(), d_local.data_ptr(), d_count.data_ptr() if d_count is not None else 0,
                      d_illegal.data_ptr(), stream)
    torch.cuda.synchronize()
    return d_seq.cpu().numpy().view(np.uint32), d_local.cpu().numpy().view(np.uint64), int(d_illegal.item())


@pytest.mark.parametrize("lookup", ["lds", "dir"])
@pytest.mark.parametrize("amino", [False, True], ids=["dna", "amino"])
def test_every_position_equals_the_host_mapping(awfm, require_gpu, tmp_path, wide, diag, lookup, amino):
    import torch
    diag(record_lookup=lookup)
    ix, ends, _ = _fasta_index(awfm, tmp_path, amino)
    g = awfm.GpuIndex(ix)
    assert g.is_wide == wide and g.num_records == len(ends)
    assert f"record table: {len(ends)} records, lookup {lookup}" in g.describe()
    positions = np.arange(ix.bwt_length + 1, dtype=np.uint64)
    want_seq, want_local, want_illegal = awfm.local_positions_host(ix, positions)
    assert want_illegal > len(ends)  # every terminator, and the tail
    n = len(positions)
    for in_place in (False, True):
        seq, local, illegal = _map(g, positions, torch, in_place=in_place)
        assert np.array_equal(seq, want_seq) and np.array_equal(local, want_local) and illegal == want_illegal, in_place
        # the count on the device: smaller than, equal to and larger than the capacity; entries past it stay as they were
        for count, capacity in ((n // 3, n), (n - 7, n - 7), (n + 1000, n - 7), (0, n)):
            seq, local, illegal = _map(g, positions, torch, in_place=in_place, count=count, capacity=capacity)
            m = min(count, capacity)
            assert np.array_equal(seq[:m], want_seq[:m]) and np.array_equal(local[:m], want_local[:m]), (in_place, count, capacity)
            assert illegal == int((want_seq[:m] == lp.ILLEGAL).sum())
            assert (seq[m:] == 0x77777777).all()
            assert np.array_equal(local[m:], positions[m:]) if in_place else (local[m:] == 0x5555555555555555).all()
    g.destroy()
    ix.dealloc()


def test_table_with_ends_beyond_32_bits_and_refused_tables(awfm, require_gpu):
    import torch
    ix = awfm.create_index(np.frombuffer(b"acgtacgtacgtacgt" * 8, np.uint8), awfm.AwFmAlphabetDna, 2, 2)
    g = awfm.GpuIndex(ix)
    plain_bytes = g.device_bytes
    assert g.num_records == 0 and "record table" not in g.describe()
    dev = torch.device("cuda")
    d = torch.zeros(8, dtype=torch.int64, device=dev)
    with pytest.raises(awfm.AwFmError) as err:  # no table: the error code, nothing launched
        g.local_positions(d.data_ptr(), 4, d.data_ptr() + 32, d.data_ptr())
    assert err.value.rc == awfm.AwFmUnsupportedVersionError
    # seven records of about 3 * 10^9 positions, an empty one among them
    lengths = np.array([3_000_000_000, 2_999_999_999, 0, 3_000_000_001, 1, 3_100_000_000, 2_900_000_000], np.uint64)
    ends = lp.ends_of(lengths)
    assert ends[1] > 1 << 32
    g.set_record_table(ends)
    assert g.num_records == 7 and g.device_bytes > plain_bytes
    rng = np.random.default_rng(11)
    positions = np.concatenate([rng.integers(0, int(ends[-1]) + 5000, 3_000_000, dtype=np.uint64), ends, ends - np.uint64(1), ends + np.uint64(1),
                                np.array([0, (1 << 64) - 1, 1 << 63], np.uint64)])
    want = lp.expected(ends, positions)
    seq, local, illegal = _map(g, positions, torch)
    assert np.array_equal(seq, want[0]) and np.array_equal(local, want[1]) and illegal == want[2]
    # refused tables leave the old one in place
    for bad in (np.array([10, 5, 20], np.uint64), np.array([10, 10, 20], np.uint64), np.array([5, 1 << 63], np.uint64)):
        with pytest.raises(awfm.AwFmError) as err:
            g.set_record_table(bad)
        assert err.value.rc == awfm.AwFmIllegalPositionError
    assert g.num_records == 7
    seq, local, illegal = _map(g, positions[:1000], torch)
    assert np.array_equal(seq, want[0][:1000]) and np.array_equal(local, want[1][:1000])
    # dropping the table restores the image's size and the error code
    g.set_record_table(np.zeros(0, np.uint64))
    assert g.num_records == 0 and g.device_bytes == plain_bytes
    with pytest.raises(awfm.AwFmError) as err:
        g.local_positions(d.data_ptr(), 4, d.data_ptr() + 32, d.data_ptr())
    assert err.value.rc == awfm.AwFmUnsupportedVersionError
    with pytest.raises(awfm.AwFmError) as err:
        g.locate_host_local(np.frombuffer(b"acgt", np.uint8), fixed_length=4)
    assert err.value.rc == awfm.AwFmUnsupportedVersionError
    g.destroy()
    ix.dealloc()


def test_many_records_take_the_directory_in_memory(awfm, require_gpu):
    """a protein-set-shaped table: 5.7 * 10^5 records of 0..700 residues with runs of empty ones, installed on a small index (the
    pass never touches the BWT)"""
    import torch
    ix = awfm.create_index(np.frombuffer(b"acdefghiklmnpqrstvwy" * 8, np.uint8), awfm.AwFmAlphabetAmino, 2, 2)
    g = awfm.GpuIndex(ix)
    rng = np.random.default_rng(570000)
    lengths = rng.integers(0, 701, 570_000)
    for at in rng.integers(0, 569_000, 40):  # runs of empty records, up to 300 in a row
        lengths[at:at + int(rng.integers(2, 300))] = 0
    lengths[200_000:200_000 + 5000] = 1  # and a long run of one-residue records: many ends in every bucket they touch
    ends = lp.ends_of(lengths)
    g.set_record_table(ends)
    assert "record table: 570000 records, lookup dir" in g.describe()
    positions = np.concatenate([rng.integers(0, int(ends[-1]) + 100_000, 10_000_000, dtype=np.uint64), ends])
    want = lp.expected(ends, positions)
    assert want[2] >= len(ends)
    for in_place in (False, True):
        seq, local, illegal = _map(g, positions, torch, in_place=in_place)
        assert np.array_equal(seq, want[0]) and np.array_equal(local, want[1]) and illegal == want[2]
    g.destroy()
    ix.dealloc()


def test_amino_fasta_index_of_a_few_thousand_records(awfm, require_gpu, tmp_path):
    import torch
    lengths = np.random.default_rng(9).integers(0, 60, 4500)
    fa = tmp_path / "set.fa"
    lp.write_fasta(str(fa), lengths, lp.AMINO_LETTERS, 6)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetAmino, 4, 2)
    g = awfm.GpuIndex(ix)
    assert g.num_records == 4500 and "lookup dir" in g.describe()  # more records than the LDS lookup holds
    positions = np.arange(ix.bwt_length + 1, dtype=np.uint64)
    want = awfm.local_positions_host(ix, positions)
    assert np.array_equal(want[0], lp.expected(lp.ends_of(lengths), positions)[0])
    seq, local, illegal = _map(g, positions, torch)
    assert np.array_equal(seq, want[0]) and np.array_equal(local, want[1]) and illegal == want[2]
    g.destroy()
    ix.dealloc()


def _planted(records, count, k, seed):
    """k-mers cut out of records that hold at least k residues, and as many random ones"""
    rng = np.random.default_rng(seed)
    long_enough = [r for r in records if len(r) >= k]
    out = []
    for _ in range(count):
        r = long_enough[int(rng.integers(0, len(long_enough)))]
        at = int(rng.integers(0, len(r) - k + 1))
        out.append(np.frombuffer(r[at:at + k], np.uint8))
    out += list(lp.DNA_LETTERS[rng.integers(0, 4, (count, k))])
    q = np.stack(out)
    return q[rng.permutation(len(q))]


@pytest.mark.parametrize("budget", [None, 64 * 1024])
def test_search_to_sequence_coordinates_without_a_host_wait(awfm, require_gpu, tmp_path, monkeypatch, budget):
    """search -> hit offsets -> locate -> local positions on one stream with one synchronise at the end, dense and listed; equal
    to locate_host + local_positions_host, and locate_host_local equals both -- also with a hit budget that cuts the host-buffer
    locate into several windows"""
    import torch
    if budget is not None:
        monkeypatch.setenv("AWFM_GPU_HIT_BUDGET_BYTES", str(budget))
    K = 21
    ix, ends, records = _fasta_index(awfm, tmp_path, False, seed=77, count=1200, sa_ratio=8, seed_k=8)
    assert len(ends) >= 1000
    g = awfm.GpuIndex(ix)
    g.set_ordered(1)
    g.set_deep_seed(11)
    q = _planted(records, 30000, K, 3)
    Q = len(q)
    chars = np.ascontiguousarray(q).reshape(-1)
    # the host path: global positions, mapped on the host
    _, hit_off, pos = g.locate_host(chars, fixed_length=K)
    total = int(hit_off[Q])
    assert total >= 30000
    if budget is not None:
        assert total * 8 > 3 * budget  # several windows
    want_seq, want_local, want_illegal = awfm.local_positions_host(ix, pos)
    starts = np.zeros_like(ends)
    starts[1:] = ends[:-1] + np.uint64(1)
    assert want_illegal == 0 and (want_local + np.uint64(K) <= (ends - starts)[want_seq]).all()  # every hit lies inside its record
    _, hit_off2, seq2, local2, illegal2 = g.locate_host_local(chars, fixed_length=K)
    assert np.array_equal(hit_off2, hit_off) and np.array_equal(seq2, want_seq) and np.array_equal(local2, want_local) and illegal2 == 0
    # the device path, dense: one stream, nothing read back before the end
    dev = torch.device("cuda")
    stream_obj = torch.cuda.Stream()
    s = stream_obj.cuda_stream
    with torch.cuda.stream(stream_obj):
        d_chars = torch.from_numpy(chars).to(dev)
        d_ranges = torch.zeros(Q * 2, dtype=torch.int64, device=dev)
        d_counts = torch.zeros(Q, dtype=torch.int32, device=dev)
        d_off = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        d_scratch = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(Q), dtype=torch.uint8, device=dev)
        cap_hits = total + 500
        d_pos = torch.full((cap_hits,), -1, dtype=torch.int64, device=dev)
        d_seq = torch.full((cap_hits,), -2, dtype=torch.int32, device=dev)
        d_illegal = torch.zeros(1, dtype=torch.int64, device=dev)
    stream_obj.synchronize()
    g.search_hits(d_chars.data_ptr(), 0, K, Q, d_ranges.data_ptr(), d_counts.data_ptr(), s)
    g.hit_offsets_on_device(d_counts.data_ptr(), 0, Q, d_off.data_ptr(), d_scratch.data_ptr(), s)
    g.locate_on_device(d_ranges.data_ptr(), d_off.data_ptr(), Q, cap_hits, d_pos.data_ptr(), s)
    g.local_positions(d_pos.data_ptr(), cap_hits, d_seq.data_ptr(), d_pos.data_ptr(), d_off.data_ptr() + 8 * Q, d_illegal.data_ptr(), s)
    stream_obj.synchronize()
    assert int(d_off[Q].item()) == total and int(d_illegal.item()) == 0
    assert np.array_equal(d_seq[:total].cpu().numpy().view(np.uint32), want_seq)
    assert np.array_equal(d_pos[:total].cpu().numpy().view(np.uint64), want_local)
    assert (d_seq[total:] == -2).all()  # nothing past the count
    # ... and listed: the count is the entry of the list's hit offsets at its capacity
    cap = Q
    d_kmers = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_list = torch.zeros(cap * 2, dtype=torch.int64, device=dev)
    d_skmers = torch.zeros(cap, dtype=torch.int32, device=dev)
    d_sorted = torch.zeros(cap * 2, dtype=torch.int64, device=dev)
    d_num = torch.zeros(1, dtype=torch.int32, device=dev)
    d_loff = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    d_pos.fill_(-1)
    d_seq.fill_(-2)
    torch.cuda.synchronize()
    g.search_hits_compact(d_chars.data_ptr(), 0, K, Q, d_kmers.data_ptr(), d_list.data_ptr(), cap, d_num.data_ptr(), stream=s)
    g.list_locate_on_device(d_kmers.data_ptr(), d_list.data_ptr(), cap, d_num.data_ptr(), Q, d_skmers.data_ptr(), d_sorted.data_ptr(),
                            d_loff.data_ptr(), cap_hits, d_pos.data_ptr(), s)
    g.local_positions(d_pos.data_ptr(), cap_hits, d_seq.data_ptr(), d_pos.data_ptr(), d_loff.data_ptr() + 8 * cap, d_illegal.data_ptr(), s)
    stream_obj.synchronize()
    assert int(d_loff[cap].item()) == total and int(d_illegal.item()) == 0
    # (the list holds the k-mers with hits in k-mer order: its flat hit list is the dense one)
    assert np.array_equal(d_seq[:total].cpu().numpy().view(np.uint32), want_seq)
    assert np.array_equal(d_pos[:total].cpu().numpy().view(np.uint64), want_local)
    assert (d_seq[total:] == -2).all()
    g.stream_retire(s)
    g.destroy()
    ix.dealloc()


def test_ambiguity_letters_hit_the_terminators_of_test2_fa(awfm, require_gpu, tmp_path):
    fa = tmp_path / "test2.fa"
    fa.write_text(TEST2_FA)
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetAmino, sa_ratio=2, seed_k=2)
    g = awfm.GpuIndex(ix)
    assert g.num_records == 4
    kmers = [b"x", b"acdef", b"g", b"hikl", b"m", b"cde"]
    chars = np.frombuffer(b"".join(kmers), np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(k) for k in kmers])]).astype(np.uint64)
    _, hit_off, seq, local, illegal = g.locate_host_local(chars, offsets=offsets)
    assert np.diff(hit_off).tolist() == [4, 1, 1, 1, 1, 1] and illegal == 4
    assert seq[:4].tolist() == [lp.ILLEGAL] * 4 and sorted(local[:4].tolist()) == [5, 7, 12, 14]  # the four terminators, positions kept
    assert list(zip(seq[4:].tolist(), local[4:].tolist())) == [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1)]
    g.destroy()
    ix.dealloc()


def test_two_lanes_map_while_the_table_is_replaced(awfm, require_gpu, tmp_path):
    """two host threads map on two lanes of one image -- on device buffers and through the host-buffer locate -- while a third
    installs the same table again and again: no error, the same results every round"""
    import torch
    ix, ends, records = _fasta_index(awfm, tmp_path, False, seed=5, count=400, sa_ratio=8, seed_k=8)
    lanes = awfm.GpuIndex.acquire_all(ix)
    assert len(lanes) >= 2
    positions = np.arange(ix.bwt_length + 1, dtype=np.uint64)
    want = awfm.local_positions_host(ix, positions)
    q = _planted(records, 3000, 15, 8)
    chars = np.ascontiguousarray(q).reshape(-1)
    _, _, pos = lanes[0].locate_host(chars, fixed_length=15)
    want_hits = awfm.local_positions_host(ix, pos)
    errors, stop = [], threading.Event()

    def mapper(g):
        try:
            stream_obj = torch.cuda.Stream()
            for _ in range(30):
                seq, local, illegal = _map(g, positions, torch, stream=stream_obj.cuda_stream)
                if not (np.array_equal(seq, want[0]) and np.array_equal(local, want[1]) and illegal == want[2]):
                    raise AssertionError("device mapping differs")
                _, _, seq, local, illegal = g.locate_host_local(chars, fixed_length=15)
                if not (np.array_equal(seq, want_hits[0]) and np.array_equal(local, want_hits[1]) and illegal == want_hits[2]):
                    raise AssertionError("host-buffer mapping differs")
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    def setter(g):
        try:
            while not stop.is_set():
                g.set_record_table(ends)
                time.sleep(0.002)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=mapper, args=(lanes[0],)), threading.Thread(target=mapper, args=(lanes[1],))]
    third = threading.Thread(target=setter, args=(lanes[0],))
    third.start()
    for t in threads:
        t.start()
    for t in threads:
        t.join(600)
    stop.set()
    third.join(600)
    assert not any(t.is_alive() for t in threads + [third]), "a caller did not come back"
    assert not errors, errors
    assert lanes[0].num_records == len(ends)
    ix.dealloc()
