"""The second table window of lookupSearchKernel (csrc/awfm_ordered_kernel.h): a k-mer still alive after the deeper-table entry
of its LAST characters is looked up once more, by its LEFTMOST characters (the table's depth, plus the two the next-step bits
speak of), and dropped before any step when that entry is empty or its bit is clear.  A k-mer that occurs in the text has every
window of itself in the text, so under the hits-only contract nothing changes: every output must be the oracle's with the window
forced on ($AWFM_GPU_DIAG second_window=1), forced off (=0) and left to the kernel's gate (unset), and the two counters
awfmGpuLastSecondWindow reports must be what the text's own 14-mers say.

All on a 200 000-letter text, seed table 8, deeper table 12, set_ordered(1), $AWFM_GPU_LOOKUP_FIRST=1."""
import functools

import numpy as np
import pytest

from avxwindowfmindex_amd import synth

pytestmark = pytest.mark.gpu

N, SEED_K, DEEP_K, Q = 200000, 8, 12, 70013
W = DEEP_K + 2  # the characters a window takes when the next-step bits are in use


@functools.lru_cache(maxsize=None)
def _text():
    txt = synth.text(N + 7, N, synth.DNA_ALPHABET).copy()
    txt.setflags(write=False)
    return txt


def _codes(chars):
    """2 bits a letter (either case); anything else: 4"""
    lut = np.full(256, 4, dtype=np.int64)
    for i, c in enumerate(b"acgt"):
        lut[c] = lut[c & 0xDF] = i
    return lut[chars]


def _windows(codes2d, first, width):
    """the letters first .. first + width - 1 of every row as one number"""
    v = np.zeros(codes2d.shape[0], dtype=np.int64)
    for j in range(first, first + width):
        v = v * 4 + codes2d[:, j]
    return v


@functools.lru_cache(maxsize=None)
def _text_windows(width):
    """the sorted set of the text's `width`-mers"""
    c = _codes(_text())
    v = np.zeros(N - width + 1, dtype=np.int64)
    for j in range(width):
        v = v * 4 + c[j:N - width + 1 + j]
    return np.unique(v)


def _substitute(q, column):
    """the letter at `column` of every row replaced by the next of a, c, g, t"""
    nxt = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"acgt", b"cgta"):
        nxt[a] = b
    q[:, column] = nxt[q[:, column]]


def _batch_size(K):
    """70 013 k-mers -- but 2048 of 32 characters: a search takes lookupSearchKernel only when {the k-mer's characters beyond its
    bucket, its number} fit an 8-byte record (bucketFits, csrc/awfm_ordered_kernel.h: 2 K - 11 + the bits of the largest number
    <= 64), which at K = 32 leaves 11 bits for the number; 29 is the longest k-mer a batch of 70 013 takes there"""
    return 2048 if K == 32 else Q


@functools.lru_cache(maxsize=None)
def _batch(K):
    """k-mers without ambiguity letters, permuted: 7/8 random, and a 1/32 each of planted ones as they are, with the leftmost
    letter substituted (alive after the first window), with the rightmost substituted, and with a substitution in the stretch
    neither window covers (K = 32: letters 15..18, K = 29: letter 15; a smaller K has no such stretch: the leftmost letter
    again)"""
    txt = _text()
    nq = _batch_size(K)
    part = nq // 32
    planted = [synth.planted_queries(40 + i, part, K, txt).copy() for i in range(4)]
    _substitute(planted[1], 0)
    _substitute(planted[2], K - 1)
    if K > 2 * W:
        rng = np.random.default_rng(K)
        cols = rng.integers(W, K - W, size=part)  # K = 32: letters 15..18, counted from 1
        for col in range(W, K - W):
            rows = np.flatnonzero(cols == col)
            sub = planted[3][rows]
            _substitute(sub, col)
            planted[3][rows] = sub
    else:
        _substitute(planted[3], 0)
    q = np.concatenate([synth.random_queries(39, nq - 4 * part, K)] + planted)
    q = q[np.random.default_rng(1000 + K).permutation(nq)].copy()
    q.setflags(write=False)
    return q


def _expected_counters(q, K):
    """(k-mers whose last 14 letters occur in the text, those of them whose first 14 do not); no round of 256 may have more
    survivors than the 64 slots of a wave, or the counters would not be exact"""
    if K <= W:
        return 0, 0
    c = _codes(q)
    assert c.max() < 4
    last = np.isin(_windows(c, K - W, W), _text_windows(W))
    first = np.isin(_windows(c, 0, W), _text_windows(W))
    per_round = np.add.reduceat(last.astype(np.int64), np.arange(0, len(q), 256))
    assert per_round.max() < 64, "a round of this batch would overflow its slots"
    return int(last.sum()), int((last & ~first).sum())


def _index(awfm, oracle, txt=None):
    txt = _text() if txt is None else txt
    ix = awfm.create_index(txt, awfm.AwFmAlphabetDna, 8, SEED_K)
    oi = oracle.Index.wrap(oracle.DNA, 8, SEED_K, ix.bwt_length, ix.blocks(), ix.prefix_sums(), ix.seed_table(), ix.packed_sa())
    g = awfm.GpuIndex(ix)
    g.set_ordered(1)
    g.set_deep_seed(DEEP_K)
    return ix, oi, g


def _check_hits_contract(ranges, counts, sp, ep, cnt):
    hit = cnt > 0
    assert np.array_equal(counts, cnt), "counts differ"
    assert np.array_equal(ranges[hit, 0], sp[hit]) and np.array_equal(ranges[hit, 1], ep[hit]), "ranges of hits differ"
    assert np.all(ranges[~hit, 0] > ranges[~hit, 1]), "a query without hits must have an empty range"


def _search_all(g, chars, K, nq, sp, ep, cnt, misalignments=(0, 1, 2, 3)):
    """dense ranges and counts at every misalignment of the character buffer, counts only, and the list form, each checked
    against the oracle; returns the arrays (for comparisons between runs) and the counters of the first dense search"""
    import torch
    dev = torch.device("cuda")
    out, window = [], None
    for mis in misalignments:
        buf = torch.zeros(chars.size + 64, dtype=torch.uint8, device=dev)
        buf[mis:mis + chars.size] = torch.from_numpy(chars).to(dev)
        d_ranges = torch.full((nq * 2,), 7, dtype=torch.int64, device=dev)
        d_counts = torch.full((nq,), 7, dtype=torch.int32, device=dev)
        g.search_hits(buf.data_ptr() + mis, 0, K, nq, d_ranges.data_ptr(), d_counts.data_ptr())
        torch.cuda.synchronize()
        assert g.last_ordered_kernel_is_lookup()
        if window is None:
            window = g.last_second_window()
        else:
            assert g.last_second_window() == window, f"counters at misalignment {mis}"
        ranges, counts = d_ranges.cpu().numpy().view(np.uint64).reshape(nq, 2), d_counts.cpu().numpy().view(np.uint32)
        _check_hits_contract(ranges, counts, sp, ep, cnt)
        hit = cnt > 0
        out += [ranges[hit].copy(), counts.copy()]
    d_counts2 = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    g.search_hits(buf.data_ptr() + mis, 0, K, nq, 0, d_counts2.data_ptr())  # counts only
    torch.cuda.synchronize()
    assert g.last_ordered_kernel_is_lookup()
    counts2 = d_counts2.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts2, cnt)
    d_kmers = torch.zeros(nq, dtype=torch.int32, device=dev)
    d_hit_ranges = torch.zeros(nq * 2, dtype=torch.int64, device=dev)
    d_num = torch.zeros(1, dtype=torch.int32, device=dev)
    g.search_hits_compact(buf.data_ptr() + mis, 0, K, nq, d_kmers.data_ptr(), d_hit_ranges.data_ptr(), nq, d_num.data_ptr())
    torch.cuda.synchronize()
    assert g.last_ordered_kernel_is_lookup()
    listed = int(d_num.item())
    assert listed == int((cnt > 0).sum())
    g.sort_hits(d_kmers.data_ptr(), d_hit_ranges.data_ptr(), listed)
    torch.cuda.synchronize()
    ids = d_kmers[:listed].cpu().numpy().view(np.uint32)
    r = d_hit_ranges[:listed * 2].cpu().numpy().view(np.uint64).reshape(listed, 2)
    assert np.array_equal(ids, np.flatnonzero(cnt > 0)) and np.array_equal(r[:, 0], sp[cnt > 0]) and np.array_equal(r[:, 1], ep[cnt > 0])
    out += [counts2.copy(), ids.copy(), r.copy()]
    return out, window


@pytest.mark.parametrize("K", [14, 15, 21, 29, 32])
def test_exact_counters_and_parity(oracle, awfm, require_gpu, wide, monkeypatch, diag, K):
    """the window forced on: `tested` is every k-mer whose last 14 letters occur in the text, `dropped` those of them whose
    first 14 do not (K = 14: the two windows are the same one, nothing is tested); dense, counts-only and list results are the
    oracle's at every misalignment of the buffer, and the same arrays with the window forced off and left to the gate.
    (K = 32 on 2048 k-mers, the largest batch of that length the lookup kernel takes, and K = 29 on the full batch beside it:
    _batch_size)"""
    monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", "1")
    q = _batch(K)
    nq = len(q)
    expected = _expected_counters(q, K)
    if K > W:
        assert expected[0] > nq // 16 and 0 < expected[1] < expected[0]
    ix, oi, g = _index(awfm, oracle)
    assert g.has_pair_image and "with next-step bits" in g.describe()
    chars, offsets = synth.fixed_csr(q)
    sp, ep, cnt, _ = oi.batch_search(chars, offsets, threads=4)
    assert cnt.sum() > 0 and (cnt == 0).sum() > nq // 4
    if K > 2 * W:  # the k-mers substituted between the windows pass both and are emptied by the steps
        assert expected[0] - expected[1] > int((cnt > 0).sum()) + nq // 64
    results = {}
    for mode in ("1", "0", None):
        diag(second_window=mode)
        results[mode], window = _search_all(g, chars, K, nq, sp, ep, cnt)
        print(f"K={K} second_window={mode}: tested, dropped = {window}; expected {expected}")
        if mode == "1":
            assert window == expected
        elif mode == "0":
            assert window == (0, 0)
        else:
            assert window[0] <= expected[0] and window[1] <= expected[1]
    for mode in ("0", None):
        assert len(results[mode]) == len(results["1"])
        for a, b in zip(results[mode], results["1"]):
            assert np.array_equal(a, b), f"second_window={mode} against 1"
    g.destroy()
    ix.dealloc()


@pytest.mark.parametrize("knob", ["AWFM_GPU_DEEP_NEXT", "AWFM_GPU_PAIR"])
@pytest.mark.parametrize("K", [21, 15])
def test_ambiguity_letters_and_knobs(oracle, awfm, require_gpu, wide, monkeypatch, diag, knob, K):
    """the same batch with 0.05 % of its letters replaced by x and 30 % in upper case, on a table without next-step bits and on
    an image without pair steps (the window is then the table's 12 letters): the oracle's results with the window forced on"""
    monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", "1")
    monkeypatch.setenv(knob, "0")
    diag(second_window="1")
    q = _batch(K).copy()
    rng = np.random.default_rng(77 + K)
    flat = q.reshape(-1)
    flat[rng.random(flat.size) < 0.0005] = ord("x")
    up = rng.random(flat.size) < 0.3
    flat[up] = flat[up] & 0xDF
    ix, oi, g = _index(awfm, oracle)
    chars, offsets = synth.fixed_csr(q)
    sp, ep, cnt, _ = oi.batch_search(chars, offsets, threads=4)
    assert cnt.sum() > 0 and (cnt == 0).sum() > Q // 4
    _, (tested, dropped) = _search_all(g, chars, K, Q, sp, ep, cnt)
    print(f"{knob}=0 K={K}: tested {tested}, dropped {dropped}")
    assert 0 < dropped <= tested
    g.destroy()
    ix.dealloc()


@pytest.mark.parametrize("tail", [1, 63, 255])
@pytest.mark.parametrize("K", [21, 15])
def test_all_hits_short_last_round(oracle, awfm, require_gpu, wide, monkeypatch, diag, tail, K):
    """planted k-mers only, the batch ending where its buffer ends, several tiles per share and a batch smaller than one share:
    forced on, the window drops nothing and every k-mer is found with the oracle's range; left alone, the gate shuts -- on the
    large batch fewer than a quarter of the survivors are put to the window"""
    import torch
    monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", "1")
    txt = _text()
    ix, oi, g = _index(awfm, oracle)
    dev = torch.device("cuda")
    for rounds in (8 * 64, 3):
        nq = rounds * 256 + tail
        q = synth.planted_queries(100 + tail, nq, K, txt)
        chars, offsets = synth.fixed_csr(q)
        sp, ep, cnt, _ = oi.batch_search(chars, offsets, threads=4)
        assert cnt.min() >= 1
        buf = torch.zeros(4096 + chars.size, dtype=torch.uint8, device=dev)
        buf[4096:] = torch.from_numpy(chars).to(dev)  # the batch ends where the buffer ends
        for mode in ("1", None):
            diag(second_window=mode)
            d_ranges = torch.full((nq * 2,), 7, dtype=torch.int64, device=dev)
            d_counts = torch.full((nq,), 7, dtype=torch.int32, device=dev)
            g.search_hits(buf.data_ptr() + 4096, 0, K, nq, d_ranges.data_ptr(), d_counts.data_ptr())
            torch.cuda.synchronize()
            assert g.last_ordered_kernel_is_lookup()
            kept = g.last_ordered_kept()
            tested, dropped = g.last_second_window()
            print(f"K={K} nq={nq} second_window={mode}: kept {kept}, tested {tested}, dropped {dropped}")
            assert kept == nq and dropped == 0
            if mode == "1":
                assert tested > 0
            elif rounds > 3:
                assert tested < kept / 4
            _check_hits_contract(d_ranges.cpu().numpy().view(np.uint64).reshape(nq, 2), d_counts.cpu().numpy().view(np.uint32), sp, ep, cnt)
    g.destroy()
    ix.dealloc()


def test_edges_of_the_text(oracle, awfm, require_gpu, wide, monkeypatch, diag, tmp_path):
    """three records, two runs of N: the 21-mers at offset 0, ending at the last letter, starting right after a run of N and
    ending right before one are found with the oracle's range, the window forced on"""
    import torch
    monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", "1")
    diag(second_window="1")
    K = 21
    recs = [synth.text(300 + i, N // 3 + 11 * i, synth.DNA_ALPHABET).copy() for i in range(3)]
    runs = [(0, 5000, 40), (2, 30000, 700)]  # (record, start, length)
    for rec, start, length in runs:
        recs[rec][start:start + length] = ord("N")
    fa = tmp_path / "edges.fa"
    with open(fa, "wb") as out:
        for i, r in enumerate(recs):
            out.write(b">record %d\n" % i)
            for at in range(0, len(r), 70):
                out.write(r[at:at + 70].tobytes() + b"\n")
    ix = awfm.create_index_from_fasta(str(fa), awfm.AwFmAlphabetDna, 8, SEED_K, file_src=str(tmp_path / "edges.awfmi"))
    oi = oracle.Index.wrap(oracle.DNA, 8, SEED_K, ix.bwt_length, ix.blocks(), ix.prefix_sums(), ix.seed_table(), ix.packed_sa())
    g = awfm.GpuIndex(ix)
    g.set_ordered(1)
    g.set_deep_seed(DEEP_K)
    edges = [recs[0][:K], recs[2][-K:]]
    for i, r in enumerate(recs):
        edges += [r[:K], r[-K:]]
    for rec, start, length in runs:
        edges += [recs[rec][start + length:start + length + K], recs[rec][start - K:start]]
    edges = np.stack(edges)
    assert not np.any(edges == ord("N"))
    # among random k-mers, in every lane position of a round
    nq = 4099
    q = synth.random_queries(5, nq, K).copy()
    at = (np.arange(len(edges)) * 409 + 3) % nq
    q[at] = edges
    chars, offsets = synth.fixed_csr(q)
    sp, ep, cnt, _ = oi.batch_search(chars, offsets, threads=4)
    assert cnt[at].min() >= 1
    dev = torch.device("cuda")
    buf = torch.from_numpy(chars).to(dev)
    d_ranges = torch.full((nq * 2,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    g.search_hits(buf.data_ptr(), 0, K, nq, d_ranges.data_ptr(), d_counts.data_ptr())
    torch.cuda.synchronize()
    assert g.last_ordered_kernel_is_lookup()
    tested, dropped = g.last_second_window()
    assert tested >= len(edges) and dropped <= tested - len(edges)
    ranges, counts = d_ranges.cpu().numpy().view(np.uint64).reshape(nq, 2), d_counts.cpu().numpy().view(np.uint32)
    _check_hits_contract(ranges, counts, sp, ep, cnt)
    assert np.array_equal(ranges[at, 0], sp[at]) and np.array_equal(ranges[at, 1], ep[at]) and counts[at].min() >= 1
    g.destroy()
    ix.dealloc()


@pytest.mark.parametrize("survivors", ["hits", "droppable"])
def test_gate_shuts_on_hits_and_stays_open_on_droppable_survivors(oracle, awfm, require_gpu, wide, monkeypatch, diag, survivors):
    """the gate itself, key unset, on a batch of 16 trips per wave of a full grid (7 workgroups of 4 waves on each of 256 CUs, 1024
    k-mers a trip; the 64-bit instantiation: 6 workgroups, 18-19 trips) in which every 8th k-mer survives the first window --
    32 a round, never more than the slots, so the rule about crowded rounds does not apply -- counts only, the k-mers made on
    the device:
    * survivors that are all hits (planted k-mers): a wave tests its first two trips (32 + 32 = 64 tested, none dropped), shuts,
      and looks again on its 16th trip: 3 trips of 16 (0.19 of the survivors; 64-bit: 0.16).  A gate that never shut would
      test all of them, one that never looked again 2 of 16 (0.125; 0.107): the bounds are 0.13 and 0.25.
    * survivors that the window drops (planted k-mers with the leftmost letter substituted): 2 * dropped >= tested holds on every
      trip, the gate stays open: at least 0.98 of the survivors are tested and at least 0.9 of those dropped.
    Forced on, every survivor is tested; the counts are the same arrays under the three settings, and every planted k-mer is found."""
    import torch
    from avxwindowfmindex_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv("AWFM_GPU_LOOKUP_FIRST", "1")
    K, nq = 21, 16 * 7 * 256 * 1024
    ix, oi, g = _index(awfm, oracle)
    dev = torch.device("cuda")
    d_text = torch.from_numpy(_text().copy()).to(dev)
    d_chars = torch.empty(nq * K, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthRandomQueries(d_chars.data_ptr(), 0, nq, K, 61, 0, None) == 1
    d_planted = torch.empty((nq // 8) * K, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthPlantedQueries(d_planted.data_ptr(), 0, nq // 8, K, 62, d_text.data_ptr(), N, None) == 1
    torch.cuda.synchronize()
    planted = d_planted.view(nq // 8, K)
    if survivors == "droppable":
        nxt = torch.zeros(256, dtype=torch.uint8)
        for a, b in zip(b"acgt", b"cgta"):
            nxt[a] = b
        planted[:, 0] = nxt.to(dev)[planted[:, 0].long()]
    d_chars.view(nq, K)[::8] = planted
    del d_planted, planted
    counts = {}
    for mode in (None, "1", "0"):
        diag(second_window=mode)
        d_counts = torch.full((nq,), 7, dtype=torch.int32, device=dev)
        g.search_hits(d_chars.data_ptr(), 0, K, nq, 0, d_counts.data_ptr())
        torch.cuda.synchronize()
        assert g.last_ordered_kernel_is_lookup()
        kept = g.last_ordered_kept()
        tested, dropped = g.last_second_window()
        print(f"{survivors} second_window={mode}: kept {kept}, tested {tested} ({tested / kept:.4f}), dropped {dropped}")
        assert nq // 8 <= kept < nq // 8 + nq // 1000  # (a random 14-mer is in the 200 000-letter text once in 1300)
        if mode == "0":
            assert (tested, dropped) == (0, 0)
        elif mode == "1":
            assert tested == kept
        elif survivors == "hits":
            assert 0.13 * kept < tested < 0.25 * kept
        else:
            assert tested >= 0.98 * kept
        if mode != "0":
            if survivors == "hits":
                assert dropped < nq // 1000  # only the few random k-mers alive after the first window
            else:
                assert dropped >= 0.9 * tested
        counts[mode] = d_counts
    assert torch.equal(counts[None], counts["0"]) and torch.equal(counts["1"], counts["0"])
    every8th = counts["0"][::8]
    if survivors == "hits":
        assert int(every8th.min().item()) >= 1
    assert int((counts["0"] > 0).sum().item()) <= (nq // 8 if survivors == "hits" else 0) + nq // 1000
    g.destroy()
    ix.dealloc()
