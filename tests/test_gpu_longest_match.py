"""awfmGpuLongestSuffixMatches (include/awfm_gpu.h, csrc/awfm_match_kernel.h) against its host twin awfmLongestSuffixMatches,
itself pinned to two independent checkers by tests/test_longest_match.py: match length, range and count of every query,
no tolerance, nothing skipped -- with and without the deeper table and the pair image, narrow and wide."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_match_common as lm  # noqa: E402

pytestmark = pytest.mark.gpu


def _device(g, chars, starts=None, ends=None, fixed_length=0, n=None, min_length=0, stream=None, skew=0):
    """one device call on buffers filled with a pattern -> (lengths, ranges, counts) as numpy; skew: the characters are uploaded
    behind `skew` other bytes and the call gets the address of the first character, which is then not 4-byte aligned"""
    import torch
    dev = torch.device("cuda")
    d_chars = torch.from_numpy(np.concatenate([np.full(skew, ord("#"), np.uint8), np.array(chars, dtype=np.uint8)])).to(dev)
    assert d_chars.data_ptr() % 4 == 0
    d_starts = torch.from_numpy(starts.view(np.int64)).to(dev) if starts is not None else None
    d_ends = torch.from_numpy(ends.view(np.int64)).to(dev) if ends is not None else None
    n = starts.size if starts is not None else n
    d_len = torch.full((max(n, 1),), 7, dtype=torch.int32, device=dev)
    d_ranges = torch.full((max(n, 1) * 2,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((max(n, 1),), 7, dtype=torch.int32, device=dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    g.longest_suffix_matches(d_chars.data_ptr() + skew, d_starts.data_ptr() if d_starts is not None else 0,
                             d_ends.data_ptr() if d_ends is not None else 0, fixed_length, n, min_length, d_len.data_ptr(),
                             d_ranges.data_ptr(), d_counts.data_ptr(), stream=stream.cuda_stream if stream is not None else 0)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    return (d_len[:n].cpu().numpy().view(np.uint32), d_ranges[:2 * n].cpu().numpy().view(np.uint64).reshape(n, 2),
            d_counts[:n].cpu().numpy().view(np.uint32), (d_chars, d_starts, d_ends, d_len, d_ranges, d_counts))


def _same(got, want, what):
    for k, name in enumerate(("match lengths", "ranges", "counts")):
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))
        assert bad.size == 0, (what, name, bad[:5].tolist(), got[k][bad[:5]].tolist(), want[k][bad[:5]].tolist())


def _configurations(g, amino, deep_k):
    """the image with and without its deeper table, with and without the pair image"""
    if amino:
        for deep in (deep_k, 0):
            g.set_deep_seed(deep)
            assert g.deep_seed_k == deep
            yield f"amino deep={deep}"
        return
    for pair in (1, 0):
        g.set_pair_image(pair)
        for deep in (deep_k, 0):
            g.set_deep_seed(deep)
            assert g.deep_seed_k == deep and bool(g.has_pair_image) == bool(pair)
            yield f"pair={pair} deep={deep}"


@pytest.mark.parametrize("name,seed_k,deep_k", [("random", 8, 10), ("random", 4, 6), ("two-letter", 4, 7), ("n-runs", 8, 10), ("amino", 2, 3),
                                                ("amino", 1, 3)])
def test_small_texts_equal_the_host_twin(awfm, require_gpu, wide, name, seed_k, deep_k):
    text, amino = lm.small_texts()[name]
    ix = awfm.create_index(text, awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 4, seed_k)
    rng = np.random.default_rng(seed_k + 40)
    queries = [q for q, _ in lm.make_queries(rng, text, amino, 1500)]
    chars, starts, ends = lm.pack(queries)
    want = awfm.longest_suffix_matches_host(ix, chars, starts, ends)
    want16 = awfm.longest_suffix_matches_host(ix, chars, starts, ends, min_length=16)
    assert (want[0] > 64).any() and (want[0] == 0).any()
    g = awfm.GpuIndex(ix)
    assert bool(g.is_wide) == bool(wide)
    for what in _configurations(g, amino, deep_k):
        _same(_device(g, chars, starts, ends), want, (name, what))
        _same(_device(g, chars, starts, ends, min_length=16), want16, (name, what, "min 16"))
        for skew in (1, 2, 3):  # a character buffer that does not begin on a 4-byte boundary
            _same(_device(g, chars, starts, ends, skew=skew), want, (name, what, "misaligned", skew))
    # fixed length, and each output NULL in turn
    fixed = np.frombuffer(text[:2400], np.uint8)
    want_fixed = awfm.longest_suffix_matches_host(ix, fixed, fixed_length=24)
    got = _device(g, fixed, fixed_length=24, n=100)
    _same(got, want_fixed, (name, "fixed"))
    d_chars, _, _, d_len, d_ranges, d_counts = got[3]
    import torch
    for missing in range(3):
        outs = [d_len, d_ranges, d_counts]
        for o in outs:
            o.fill_(7)
        ptrs = [o.data_ptr() for o in outs]
        ptrs[missing] = 0
        g.longest_suffix_matches(d_chars.data_ptr(), 0, 0, 24, 100, 0, *ptrs)
        torch.cuda.synchronize()
        assert bool((outs[missing] == 7).all())
        back = (d_len.cpu().numpy().view(np.uint32), d_ranges.cpu().numpy().view(np.uint64).reshape(100, 2), d_counts.cpu().numpy().view(np.uint32))
        for k in range(3):
            assert k == missing or np.array_equal(back[k], want_fixed[k])
    # nothing to do; no way to find the queries
    g.longest_suffix_matches(0, 0, 0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(awfm.AwFmError) as err:
        g.longest_suffix_matches(d_chars.data_ptr(), 0, 0, 0, 5, 0, d_len.data_ptr(), 0, 0)
    assert err.value.rc == -4  # AwFmNullPtrError
    g.destroy()
    ix.dealloc()


def _big(awfm, seed_k):
    rng = np.random.default_rng(77)
    n = (1 << 24) + 1000
    text = lm.random_text(rng, n, lm.DNA)
    ix = awfm.gpu_create_index(text, awfm.AwFmAlphabetDna, 8, seed_k)
    return ix, np.frombuffer(text, np.uint8), rng


def _mixes(rng, text):
    """(name, chars, starts, ends): planted substrings; windows over reads with substitutions; random strings -- 2^20 queries each"""
    n, Q = text.size, 1 << 20
    at = rng.integers(0, n - 64, Q).astype(np.uint64)
    lengths = rng.integers(12, 64, Q).astype(np.uint64)
    yield "planted", text, at, at + lengths
    reads, starts, ends = [], [], []
    base = 0
    per_rate = Q // 3 // 24 + 1  # 25 to 37 windows per read
    for rate in (0.01, 0.05, 0.15):
        for _ in range(per_rate):
            m = int(rng.integers(100, 151))
            p = int(rng.integers(0, n - m))
            read = text[p:p + m].copy()
            hit = np.flatnonzero(rng.random(m) < rate)
            read[hit] = np.frombuffer(lm.DNA, np.uint8)[rng.integers(0, 4, hit.size)]
            e = np.arange(4, m + 1, 4, dtype=np.uint64)
            starts.append(base + np.where(e > 64, e - 64, 0).astype(np.uint64))
            ends.append(base + e)
            reads.append(read)
            base += m
    starts, ends = np.concatenate(starts), np.concatenate(ends)
    assert starts.size >= Q
    yield "reads", np.concatenate(reads), starts[:Q].copy(), ends[:Q].copy()
    chars = np.frombuffer(lm.random_text(rng, Q * 24, lm.DNA), np.uint8)
    off = np.arange(0, Q * 24 + 1, 24, dtype=np.uint64)
    yield "random", chars, off[:-1].copy(), off[1:].copy()


@pytest.mark.parametrize("seed_k,deep_k", [(8, 10), (12, 14)])
def test_a_text_of_2_to_the_24_in_three_mixes_and_located_end_to_end(awfm, require_gpu, seed_k, deep_k):
    import torch
    ix, text, rng = _big(awfm, seed_k)
    g = awfm.GpuIndex(ix, acquire=True)
    mixes = list(_mixes(rng, text))
    wants = [awfm.longest_suffix_matches_host(ix, chars, starts, ends, threads=16) for _, chars, starts, ends in mixes]
    assert (wants[0][0] == (mixes[0][3] - mixes[0][2])).all()  # planted: the whole query
    assert np.median(wants[2][0]) < 16 < np.median(wants[1][0])
    for what in _configurations(g, False, deep_k):
        for (name, chars, starts, ends), want in zip(mixes, wants):
            _same(_device(g, chars, starts, ends), want, (name, what))
    # ---- end to end on the reads: min_length -> hit offsets from the counts -> locate; every position spells the match ----
    _, chars, starts, ends = mixes[1]
    Q, L = starts.size, 20
    lengths, ranges, counts, (d_chars, d_starts, d_ends, d_len, d_ranges, d_counts) = _device(g, chars, starts, ends, min_length=L)
    assert ((counts > 0) == (lengths >= L)).all() and (counts > 0).sum() > Q // 4
    d_hit_off = torch.zeros(Q + 1, dtype=torch.int64, device="cuda")
    d_scratch = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(Q), dtype=torch.uint8, device="cuda")
    total = g.hit_offsets_from_counts(d_counts.data_ptr(), Q, d_hit_off.data_ptr(), d_scratch.data_ptr())
    assert total == int(counts.astype(np.uint64).sum())
    d_pos = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
    g.locate(d_ranges.data_ptr(), d_hit_off.data_ptr(), Q, total, d_pos.data_ptr())
    torch.cuda.synchronize()
    pos = d_pos[:total].cpu().numpy()
    owner = np.repeat(np.arange(Q), counts.astype(np.int64))
    span = lengths[owner].astype(np.int64)
    tail = ends[owner].astype(np.int64)  # the match is the last `span` characters of its query
    padded = np.concatenate([text, np.zeros(256, np.uint8)])
    for k in range(int(span.max())):  # character k of every match against character k at every located position
        live = span > k
        assert np.array_equal(padded[pos[live] + k], chars[tail[live] - span[live] + k]), k
    assert (pos + span <= text.size).all()
    # independent recount of the occurrences for a sample of queries
    sample = rng.choice(np.flatnonzero(counts > 0), 1000, replace=False)
    text_bytes = text.tobytes()
    for i in sample:
        pattern = chars[int(ends[i]) - int(lengths[i]):int(ends[i])].tobytes()
        found, at = 0, text_bytes.find(pattern)
        while at >= 0:
            found, at = found + 1, text_bytes.find(pattern, at + 1)
        assert found == int(counts[i]), (int(i), pattern)
    g.set_deep_seed(0)
    ix.dealloc()


def test_two_streams_on_one_image(awfm, require_gpu):
    import torch
    text, _ = lm.small_texts()["random"]
    ix = awfm.create_index(text, awfm.AwFmAlphabetDna, 4, 8)
    g = awfm.GpuIndex(ix)
    rng = np.random.default_rng(3)
    batches = [lm.pack([q for q, _ in lm.make_queries(rng, text, False, 20000)]) for _ in range(2)]
    wants = [_device(g, *b)[:3] for b in batches]
    for b, w in zip(batches, wants):
        _same(w, awfm.longest_suffix_matches_host(ix, *b), "single stream")
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            for _ in range(5):
                results[k] = _device(g, *batches[k], stream=stream)[:3]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        _same(results[k], wants[k], ("stream", k))
    g.destroy()
    ix.dealloc()
