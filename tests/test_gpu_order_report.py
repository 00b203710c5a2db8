"""What the reporting calls say after a seed-order search (awfmGpuLastOrderedKernelIsLookup, awfmGpuLastOrderedKept,
awfmGpuLastSecondWindow: AwFmGpuIndex::OrderReport, csrc/awfm_device.h) depends on that search alone, not on what the handle
searched before it: the report is reset as a whole when a search begins, and its device words go when the scratch they lie in
is freed.

One handle on a 200 000-letter text (seed table 8, deeper table 12, set_ordered(1)) takes the calls
  A  4096 planted 21-mers, $AWFM_GPU_LOOKUP_FIRST=1          lookupSearchKernel, forced
  B  70 013 random 21-mers, $AWFM_GPU_LOOKUP_FIRST=0          the ordering passes alone; larger than A: the slot's scratch is
                                                             freed and allocated again, A's counters lay in it
  A
  C  4096 8..30-mers in CSR form, $AWFM_GPU_MIXED_LOOKUP=1    mixedLookupSearchKernel, forced
  B
and after each of them the results are the oracle's and the three calls answer what they answer on a fresh handle of the same
index that has made that one call only.  Once on one stream, once with the calls alternating between two streams, so that both
scratch slots are in use.  (awfmGpuLastLookupFront is about sampled searches of 2^20 k-mers and more: not here.)

The library passed this module before the report became one struct as well -- there a stale pointer to the freed counters was
merely never read: the module pins the behaviour, it did not change."""
import functools
import os
import sys

import numpy as np
import pytest

from avxwindowfmindex_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bucket_records_common import _check_hits_contract  # noqa: E402

pytestmark = pytest.mark.gpu

N, SEED_K, DEEP_K = 200000, 8, 12
KNOBS = ("AWFM_GPU_LOOKUP_FIRST", "AWFM_GPU_MIXED_LOOKUP")
SEQUENCE = "ABACB"


@functools.lru_cache(maxsize=None)
def _text():
    txt = synth.text(N + 7, N, synth.DNA_ALPHABET).copy()
    txt.setflags(write=False)
    return txt


@functools.lru_cache(maxsize=None)
def _call(name):
    """(chars, offsets, fixed length or 0 for CSR, the knobs of the call)"""
    if name == "A":
        chars, offsets = synth.fixed_csr(synth.planted_queries(71, 4096, 21, _text()))
        return chars, offsets, 21, {"AWFM_GPU_LOOKUP_FIRST": "1"}
    if name == "B":
        chars, offsets = synth.fixed_csr(synth.random_queries(72, 70013, 21))
        return chars, offsets, 21, {"AWFM_GPU_LOOKUP_FIRST": "0"}
    chars, offsets = synth.mixed_queries(73, 4096, _text(), synth.DNA_ALPHABET, 8, 30)
    return chars, offsets, 0, {"AWFM_GPU_MIXED_LOOKUP": "1"}


_expected = {}  # call -> the oracle's (sp, ep, cnt): the index is the same one in every test


def _handle(awfm, ix):
    g = awfm.GpuIndex(ix)
    g.set_ordered(1)
    g.set_deep_seed(DEEP_K)
    return g


def _search(g, name, oi, monkeypatch, stream=0):
    """the call on `stream`, its dense results checked against the oracle; returns the report's triple"""
    import torch
    chars, offsets, fixed, knobs = _call(name)
    for knob in KNOBS:
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)
    if name not in _expected:
        _expected[name] = oi.batch_search(chars, offsets, threads=4)[:3]
    sp, ep, cnt = _expected[name]
    nq = len(offsets) - 1
    dev = torch.device("cuda")
    d_chars = torch.from_numpy(chars).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_ranges = torch.full((nq * 2,), 7, dtype=torch.int64, device=dev)
    d_counts = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # the buffers are ready whichever stream searches them
    g.search_hits(d_chars.data_ptr(), 0 if fixed else d_off.data_ptr(), fixed, nq, d_ranges.data_ptr(), d_counts.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    _check_hits_contract(d_ranges.cpu().numpy().view(np.uint64).reshape(nq, 2), d_counts.cpu().numpy().view(np.uint32), sp, ep, cnt)
    return g.last_ordered_kernel_is_lookup(), g.last_ordered_kept(), g.last_second_window()


@pytest.mark.parametrize("num_streams", [1, 2])
def test_report_does_not_depend_on_the_handles_history(oracle, awfm, require_gpu, monkeypatch, num_streams):
    import torch
    ix = awfm.create_index(_text(), awfm.AwFmAlphabetDna, 8, SEED_K)
    oi = oracle.Index.wrap(oracle.DNA, 8, SEED_K, ix.bwt_length, ix.blocks(), ix.prefix_sums(), ix.seed_table(), ix.packed_sa())
    fresh = {}
    for name in sorted(set(SEQUENCE)):  # what each call reports on a handle that has made no other
        h = _handle(awfm, ix)
        fresh[name] = _search(h, name, oi, monkeypatch)
        h.destroy()
    print(f"fresh handles: {fresh}")
    assert fresh["A"][0] and fresh["C"][0], "A and C are forced through their lookup kernels"
    nq_b = len(_call("B")[1]) - 1
    assert _call("B")[0].size == 21 * nq_b and np.all(np.isin(_call("B")[0], np.frombuffer(b"acgt", np.uint8)))
    assert fresh["B"] == (False, nq_b, (0, 0)), "B runs no lookup kernel and orders every one of its k-mers"
    g = _handle(awfm, ix)
    streams = [torch.cuda.Stream() for _ in range(num_streams)] if num_streams > 1 else []
    for i, name in enumerate(SEQUENCE):
        stream = streams[i % num_streams].cuda_stream if streams else 0
        got = _search(g, name, oi, monkeypatch, stream=stream)
        print(f"call {i} ({name}, stream {i % num_streams}): {got}")
        assert got == fresh[name], f"call {i} ({name}) after {SEQUENCE[:i]!r}: the report differs from a fresh handle's"
    for s in streams:
        g.stream_retire(s.cuda_stream)
    torch.cuda.synchronize()
    g.destroy()
    ix.dealloc()
