"""awfmGpuOneSubstitutionSearch (include/awfm_gpu.h, csrc/awfm_subst_kernel.h) against its host twin awfmOneSubstitutionSearch,
itself pinned to independent checkers by tests/test_one_substitution.py: the records as sets of (query, edit, sp, ep), the two
per-query arrays, no tolerance, nothing skipped -- with and without the deeper table and the pair image, on the plain path,
narrow and wide, with skewed character buffers, below capacity, on two streams, and located end to end."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longest_match_common as lm  # noqa: E402
import one_substitution_common as osc  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xFFFFFFFF


def _device(g, chars, offsets=None, fixed_length=0, n=None, include_exact=True, capacity=0, stream=None, skew=0, lists=True):
    """one device call -> (queries, edits, ranges) of the whole list at its capacity, num_hits, variants, occurrences, tensors"""
    import torch
    dev = torch.device("cuda")
    d_chars = torch.from_numpy(np.concatenate([np.full(skew, ord("#"), np.uint8), np.array(chars, dtype=np.uint8)])).to(dev)
    assert d_chars.data_ptr() % 4 == 0
    d_offsets = torch.from_numpy(offsets.view(np.int64)).to(dev) if offsets is not None else None
    n = offsets.size - 1 if offsets is not None else n
    cap = max(capacity, 1)
    d_q = torch.full((cap,), 7, dtype=torch.int32, device=dev)
    d_e = torch.full((cap,), 7, dtype=torch.int32, device=dev)
    d_r = torch.full((cap * 2,), 7, dtype=torch.int64, device=dev)
    d_total = torch.full((1,), 7, dtype=torch.int64, device=dev)
    d_var = torch.full((max(n, 1),), 7, dtype=torch.int32, device=dev)
    d_occ = torch.full((max(n, 1),), 7, dtype=torch.int64, device=dev)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    g.one_substitution_search(d_chars.data_ptr() + skew, d_offsets.data_ptr() if d_offsets is not None else 0, fixed_length, n,
                              include_exact, d_q.data_ptr() if lists else 0, d_e.data_ptr() if lists else 0,
                              d_r.data_ptr() if lists else 0, capacity if lists else 0, d_total.data_ptr(), d_var.data_ptr(),
                              d_occ.data_ptr(), stream=stream.cuda_stream if stream is not None else 0)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    return (d_q[:capacity].cpu().numpy().view(np.uint32), d_e[:capacity].cpu().numpy().view(np.uint32),
            d_r[:2 * capacity].cpu().numpy().view(np.uint64).reshape(capacity, 2), int(d_total.cpu().numpy().view(np.uint64)[0]),
            d_var[:n].cpu().numpy().view(np.uint32), d_occ[:n].cpu().numpy().view(np.uint64),
            (d_chars, d_offsets, d_q, d_e, d_r, d_total, d_var, d_occ))


def _same(got, want, what):
    """got: a device result whose capacity was at least the number of records; want: the host twin's"""
    total = want[3]
    assert got[3] == total, (what, got[3], total)
    assert got[0].size >= total
    filled = got[0] != FILL
    assert int(filled.sum()) == total, (what, int(filled.sum()), total)
    # the appends fill slots 0 .. total - 1, the tail keeps the fill {0xFFFFFFFF, 0xFFFFFFFF, {1, 0}}
    assert filled[:total].all() and (got[1][total:] == FILL).all(), what
    assert (got[2][total:] == np.array([1, 0], np.uint64)).all(), what
    a, b = osc.as_set(got[0][:total], got[1][:total], got[2][:total]), osc.as_set(*want[:3])
    assert a == b, (what, sorted(a - b)[:5], sorted(b - a)[:5])
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]), what


def _configurations(g, amino, deep_k):
    """the image with and without its deeper table, with and without the pair image.  The kernel never reads the pair image: the
    pair loop pins only that having one changes nothing"""
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


_small = {}


def _small_case(awfm, name, seed_k, deep_k):
    """index, batch and the host twin's answers of one small text, computed once for the three widths"""
    key = (name, seed_k, deep_k)
    if key not in _small:
        text, amino = lm.small_texts()[name]
        ix = awfm.create_index(text, awfm.AwFmAlphabetAmino if amino else awfm.AwFmAlphabetDna, 4, seed_k)
        mix = osc.make_mix(np.random.default_rng(seed_k + 60), text, amino, seed_k, deep_k)
        chars, offsets = osc.pack([q for q, _, _ in mix])
        want = awfm.one_substitution_search_host(ix, chars, offsets)
        want_off = awfm.one_substitution_search_host(ix, chars, offsets, include_exact=False)
        fixed = np.frombuffer(text[:2100], np.uint8)
        want_fixed = awfm.one_substitution_search_host(ix, fixed, fixed_length=21)
        assert want[3] > 1000 and want_off[3] < want[3] and want_fixed[3] >= 100
        _small[key] = (text, amino, ix, chars, offsets, want, want_off, fixed, want_fixed)
    return _small[key]


@pytest.mark.parametrize("name,seed_k,deep_k", [("random", 8, 10), ("random", 4, 6), ("two-letter", 4, 7), ("n-runs", 8, 10), ("amino", 2, 3),
                                                ("amino", 1, 3)])
def test_small_texts_equal_the_host_twin(awfm, require_gpu, wide, name, seed_k, deep_k):
    text, amino, ix, chars, offsets, want, want_off, fixed, want_fixed = _small_case(awfm, name, seed_k, deep_k)
    g = awfm.GpuIndex(ix)
    assert bool(g.is_wide) == bool(wide)
    cap = want[3] + 100
    for what in _configurations(g, amino, deep_k):
        _same(_device(g, chars, offsets, capacity=cap), want, (name, what))
        _same(_device(g, chars, offsets, capacity=cap, include_exact=False), want_off, (name, what, "no exact"))
        for skew in (1, 2, 3):  # a character buffer that does not begin on a 4-byte boundary
            _same(_device(g, chars, offsets, capacity=cap, skew=skew), want, (name, what, "misaligned", skew))
    # the plain path: letter by letter, no table, on an image that has the tables
    if not amino:
        g.set_pair_image(1)
    g.set_deep_seed(deep_k)
    _same(_device(g, chars, offsets, capacity=cap), want, (name, "tables again"))
    g.set_kernel(awfm.AWFM_GPU_KERNEL_GROUP2)
    _same(_device(g, chars, offsets, capacity=cap), want, (name, "plain path"))
    _same(_device(g, fixed, fixed_length=21, n=100, capacity=want_fixed[3] + 7), want_fixed, (name, "plain path, fixed"))
    g.set_kernel(awfm.AWFM_GPU_KERNEL_AUTO)
    # the fixed-length form
    _same(_device(g, fixed, fixed_length=21, n=100, capacity=want_fixed[3] + 7), want_fixed, (name, "fixed"))
    g.destroy()


def test_overflow_counts_only_and_edge_cases(awfm, require_gpu):
    import torch
    text, amino, ix, chars, offsets, want, want_off, fixed, want_fixed = _small_case(awfm, "random", 8, 10)
    g = awfm.GpuIndex(ix)
    g.set_deep_seed(10)
    total, true = want[3], osc.as_set(*want[:3])
    cap = total // 3
    got = _device(g, chars, offsets, capacity=cap)
    assert got[3] == total  # the true number of records, beyond the capacity
    stored = osc.as_set(got[0], got[1], got[2])  # distinct ...
    assert len(stored) == cap and stored <= true  # ... members of the true set, the list full
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])  # per-query arrays complete
    _same(_device(g, chars, offsets, capacity=total + 1000), want, "a larger list keeps the fill in its tail")
    # counts only: capacity 0 with NULL lists
    got = _device(g, chars, offsets, capacity=0, lists=False)
    assert got[3] == total and np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])
    d_chars, d_offsets, d_q, d_e, d_r, d_total, d_var, d_occ = got[6]
    assert int(d_q[0]) == 7 and int(d_r[0]) == 7
    n = offsets.size - 1
    # every output NULL in turn (the lists need the counter they are appended through)
    d_total.fill_(7)
    d_var.fill_(7)
    g.one_substitution_search(d_chars.data_ptr(), d_offsets.data_ptr(), 0, n, True, 0, 0, 0, 0, 0, 0, d_occ.data_ptr())
    torch.cuda.synchronize()
    assert int(d_total[0]) == 7 and bool((d_var == 7).all()) and np.array_equal(d_occ.cpu().numpy().view(np.uint64), want[5])
    g.one_substitution_search(d_chars.data_ptr(), d_offsets.data_ptr(), 0, n, True, 0, 0, 0, 0, 0, 0, 0)
    torch.cuda.synchronize()
    # nothing to do; no way to find the queries
    g.one_substitution_search(0, 0, 0, 0, True, 0, 0, 0, 0, 0, 0, 0)
    for args in ((0, d_offsets.data_ptr(), 0), (d_chars.data_ptr(), 0, 0)):  # missing dChars; neither offsets nor a length
        with pytest.raises(awfm.AwFmError) as err:
            g.one_substitution_search(*args, n, True, 0, 0, 0, 0, d_total.data_ptr(), 0, 0)
        assert err.value.rc == -4  # AwFmNullPtrError
    with pytest.raises(awfm.AwFmError) as err:  # lists without the counter
        g.one_substitution_search(d_chars.data_ptr(), d_offsets.data_ptr(), 0, n, True, d_q.data_ptr(), 0, 0, 1, 0, 0, 0)
    assert err.value.rc == -4
    with pytest.raises(awfm.AwFmError):  # query numbers are 32-bit
        g.one_substitution_search(d_chars.data_ptr(), d_offsets.data_ptr(), 0, 1 << 32, True, 0, 0, 0, 0, d_total.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    g.destroy()


def test_a_batch_larger_than_the_persistent_grid(awfm, require_gpu):
    """oneSubstitutionKernel runs on a grid of at most CUs x 8 workgroups of 64 groups (gridFor, csrc/awfm_device.h), one query per
    group and round: only a batch beyond that makes a group come back for a second query (q += numGroups, with the loop's
    values parked in vector registers).  2^14 queries of the mix, 17 times over plus 3: the host twin answers the 2^14 once and
    the expectation is tiled, the records shifted by the query number."""
    import torch
    text, amino, ix = _small_case(awfm, "random", 8, 10)[:3]
    rng = np.random.default_rng(68)
    queries = []
    while len(queries) < 1 << 14:
        queries += [q for q, _, _ in osc.make_mix(rng, text, amino, 8, 10)]
    queries = queries[:1 << 14]
    base, times, more = len(queries), 17, 3
    n = base * times + more
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"\n{cus} CUs: the grid has at most {cus * 8 * 64} groups, the batch {n} queries")
    assert n == 278531 and n > cus * 8 * 64, (n, cus)  # a larger part has to get a larger batch
    chars, offsets = osc.pack(queries * times + queries[:more])
    for include_exact in (True, False):
        q1, e1, r1, total1, v1, o1 = awfm.one_substitution_search_host(ix, *osc.pack(queries), include_exact=include_exact, threads=16)
        assert total1 > 10000
        first = q1 < more
        shift = (np.arange(times, dtype=np.uint32) * np.uint32(base)).repeat(q1.size)
        want = (np.concatenate([np.tile(q1, times) + shift, q1[first] + np.uint32(base * times)]), np.concatenate([np.tile(e1, times), e1[first]]),
                np.concatenate([np.tile(r1, (times, 1)), r1[first]]), total1 * times + int(first.sum()),
                np.concatenate([np.tile(v1, times), v1[:more]]), np.concatenate([np.tile(o1, times), o1[:more]]))
        g = awfm.GpuIndex(ix)
        g.set_pair_image(1)
        g.set_deep_seed(10)
        for kernel, what in ((awfm.AWFM_GPU_KERNEL_AUTO, "tables"), (awfm.AWFM_GPU_KERNEL_GROUP2, "plain path")):
            g.set_kernel(kernel)
            got = _device(g, chars, offsets, capacity=want[3] + 100, include_exact=include_exact)
            total = want[3]
            assert got[3] == total and int((got[0] != FILL).sum()) == total, (what, got[3], total)
            assert (got[0][:total] != FILL).all() and (got[1][total:] == FILL).all() and (got[2][total:] == np.array([1, 0], np.uint64)).all(), what
            # the records as sets: both lists in the order of (query, edit), which is a key (no record twice)
            for k, (hq, he, hr) in enumerate((got[:3], want[:3])):
                key = hq[:total].astype(np.uint64) << np.uint64(32) | he[:total].astype(np.uint64)
                order = np.argsort(key, kind="stable")
                assert (np.diff(key[order].view(np.int64)) != 0).all(), (what, "a record twice", k)
                if k == 0:
                    got_key, got_ranges = key[order], hr[:total][order]
                else:
                    assert np.array_equal(got_key, key[order]) and np.array_equal(got_ranges, hr[:total][order]), what
            assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]), what
        g.destroy()


def test_two_streams_on_one_image(awfm, require_gpu):
    import torch
    text, _ = lm.small_texts()["random"]
    ix = awfm.create_index(text, awfm.AwFmAlphabetDna, 4, 8)
    g = awfm.GpuIndex(ix)
    g.set_deep_seed(10)
    rng = np.random.default_rng(3)
    batches = [osc.pack([q for q, _ in lm.make_queries(rng, text, False, 5000)]) for _ in range(2)]
    wants = [awfm.one_substitution_search_host(ix, *b, threads=8) for b in batches]
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream()
            for _ in range(5):
                results[k] = _device(g, *batches[k], capacity=wants[k][3] + 10, stream=stream)[:6]
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


# ---- a text of 2^20 positions with a copied stretch, 2^17 queries, located end to end ----
_medium = {}


def _medium_case(awfm):
    if not _medium:
        rng = np.random.default_rng(2026)
        n, Q, L = 1 << 20, 1 << 16, 21
        text = np.frombuffer(lm.random_text(rng, n, lm.DNA), np.uint8).copy()
        text[700000:700000 + (1 << 16)] = text[100000:100000 + (1 << 16)]  # so that some ranges are longer than 1
        letters = np.frombuffer(lm.DNA, np.uint8)
        ix = awfm.create_index(text.tobytes(), awfm.AwFmAlphabetDna, 8, 8)

        def planted(count, m, one_off):
            at = rng.integers(0, n - m, count)
            at[:count // 4] = rng.integers(100000, 100000 + (1 << 16) - m, count // 4)  # inside the copied stretch
            q = text[at[:, None] + np.arange(m)[None, :]].copy()
            if one_off:
                p = rng.integers(0, m, count)
                q[np.arange(count), p] = letters[(np.searchsorted(letters, q[np.arange(count), p]) + rng.integers(1, 4, count)) % 4]
            return q

        fixed = np.concatenate([planted(Q // 2, L, True), planted(Q // 4, L, False),
                                letters[rng.integers(0, 4, (Q // 4, L))]]).reshape(-1)
        lens = rng.integers(12, 41, Q)
        offsets = np.zeros(Q + 1, np.uint64)
        np.cumsum(lens, out=offsets[1:])
        csr = np.concatenate([planted(1, int(m), i % 2 == 0)[0] for i, m in enumerate(lens)])
        batches = {"fixed": (fixed, None, L), "csr": (csr, offsets, 0)}
        wants = {k: awfm.one_substitution_search_host(ix, c, o, fixed_length=f, threads=16) for k, (c, o, f) in batches.items()}
        assert max(int((w[2][:, 1] - w[2][:, 0]).max()) for w in wants.values()) >= 1
        _medium.update(text=text, ix=ix, batches=batches, wants=wants, Q=Q)
    return _medium


def test_a_text_of_2_to_the_20_located_end_to_end(awfm, require_gpu, wide):
    import torch
    m = _medium_case(awfm)
    text, Q = m["text"], m["Q"]
    g = awfm.GpuIndex(m["ix"])
    assert bool(g.is_wide) == bool(wide)
    g.set_pair_image(1)
    g.set_deep_seed(10)
    letters = np.frombuffer(lm.DNA, np.uint8)
    for name, (chars, offsets, fixed_length) in m["batches"].items():
        want = m["wants"][name]
        cap = want[3] + 1000
        got = _device(g, chars, offsets, fixed_length=fixed_length, n=Q, capacity=cap)
        _same(got, want, name)
        # the list AT ITS CAPACITY through the locate chain
        d_q, d_e, d_r = got[6][2:5]
        d_hit_off = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        d_scratch = torch.zeros(awfm.GpuIndex.scan_scratch_bytes(cap), dtype=torch.uint8, device="cuda")
        g.hit_offsets_on_device(0, d_r.data_ptr(), cap, d_hit_off.data_ptr(), d_scratch.data_ptr())
        occurrences = int(want[5].sum())
        d_pos = torch.zeros(occurrences + 8, dtype=torch.int64, device="cuda")
        g.locate_on_device(d_r.data_ptr(), d_hit_off.data_ptr(), cap, occurrences + 8, d_pos.data_ptr())
        torch.cuda.synchronize()
        hit_off = d_hit_off.cpu().numpy()
        assert int(hit_off[cap]) == occurrences  # as many positions as the per-query arrays say
        pos = d_pos[:occurrences].cpu().numpy()
        sizes = np.diff(hit_off)
        owner = np.repeat(np.arange(cap), sizes)  # record of every position
        query, edit = got[0][owner].astype(np.int64), got[1][owner]
        start = offsets[query].astype(np.int64) if offsets is not None else query * fixed_length
        length = (offsets[query + 1].astype(np.int64) - start) if offsets is not None else np.full(query.size, fixed_length)
        assert (pos + length <= text.size).all()
        edited = edit != osc.EDIT_NONE
        where, letter = (edit >> 5).astype(np.int64), letters[edit & 3]
        assert (where[edited] < length[edited]).all() and ((edit & 31)[edited] < 4).all()
        for k in range(int(length.max())):  # character k at every located position against character k of its query
            live = length > k
            expect = chars[start[live] + k].copy()
            swap = edited[live] & (where[live] == k)
            assert (expect[swap] != letter[live][swap]).all()  # the edit names another letter than the query's own
            expect[swap] = letter[live][swap]
            assert np.array_equal(text[pos[live] + k], expect), (name, k)
    g.destroy()
