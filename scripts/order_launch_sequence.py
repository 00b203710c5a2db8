#!/usr/bin/env python3
"""A fixed list of calls that takes a batch through every driver of csrc/awfm_gpu_ordered.hip, one stream, a wait after each:
meant to run under a kernel trace (rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 scripts/order_launch_sequence.py),
whose ordered list of (kernel, grid, workgroup, LDS) scripts/order_launch_list.py prints -- two libraries launch the same
kernels the same way when their lists are equal line for line (profiles/order_launchers_refactor/).

The text is tests/test_gpu_second_window.py's: 200 000 letters, seed table 8, deeper table 12, set_ordered(1); the amino index is
test_gpu_parity.py's (150 000 letters, seed table 3, deeper table 5)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from avxwindowfmindex_amd import api, synth  # noqa: E402

N, Q = 200000, 70013
dev = torch.device("cuda")


def knobs(**values):
    for name in ("AWFM_GPU_LOOKUP_FIRST", "AWFM_GPU_MIXED_LOOKUP", "AWFM_GPU_AMINO_LOOKUP", "AWFM_GPU_EXACT_LOOKUP"):
        os.environ.pop(name, None)
    for name, value in values.items():
        os.environ["AWFM_GPU_" + name] = value


def outputs(nq):
    return torch.full((nq * 2,), 7, dtype=torch.int64, device=dev), torch.full((nq,), 7, dtype=torch.int32, device=dev)


def upload(chars):
    """the characters on the device, with room behind them"""
    return torch.from_numpy(np.concatenate([np.ascontiguousarray(chars).reshape(-1), np.zeros(64, np.uint8)])).to(dev)


def batch(seed, nq, K, txt, alphabet=synth.DNA_ALPHABET):
    """7/8 random k-mers, 1/8 drawn from the text, permuted"""
    q = np.concatenate([synth.random_queries(seed, nq - nq // 8, K, alphabet), synth.planted_queries(seed + 1, nq // 8, K, txt)])
    return q[np.random.default_rng(seed).permutation(nq)].copy()


def main():
    txt = synth.text(N + 7, N, synth.DNA_ALPHABET).copy()
    ix = api.create_index(txt, api.AwFmAlphabetDna, 8, 8)
    g = api.GpuIndex(ix)
    g.set_ordered(1)
    g.set_deep_seed(12)
    q21 = batch(11, Q, 21, txt)
    d21 = upload(q21)
    calls = 0

    def done():
        nonlocal calls
        torch.cuda.synchronize()
        calls += 1

    for first in ("0", "1"):  # fixed 21-mers through the ordering passes, and through lookupSearchKernel
        knobs(LOOKUP_FIRST=first)
        r, c = outputs(Q)
        g.search_hits(d21.data_ptr(), 0, 21, Q, r.data_ptr(), c.data_ptr())
        done()
    knobs(LOOKUP_FIRST="1")
    q32 = batch(13, 2048, 32, txt)  # the largest batch of 32-mers whose records fit 8 bytes
    d32 = upload(q32)
    r, c = outputs(2048)
    g.search_hits(d32.data_ptr(), 0, 32, 2048, r.data_ptr(), c.data_ptr())
    done()
    knobs()
    d_packed = torch.from_numpy(api.pack_kmers(q21).view(np.int64)).to(dev)  # a packed batch
    d_scratch = torch.zeros(Q * 21 + 64, dtype=torch.uint8, device=dev)
    r, c = outputs(Q)
    g.search_hits_packed(d_packed.data_ptr(), 21, Q, r.data_ptr(), c.data_ptr(), d_scratch.data_ptr())
    done()
    knobs(MIXED_LOOKUP="1")  # a CSR batch through mixedLookupSearchKernel
    chars, offsets = synth.mixed_queries(17, Q, txt, synth.DNA_ALPHABET, 8, 30)
    d_chars = upload(chars)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    r, c = outputs(Q)
    g.search_hits(d_chars.data_ptr(), d_off.data_ptr(), 0, Q, r.data_ptr(), c.data_ptr())
    done()
    knobs(LOOKUP_FIRST="0")
    r, c = outputs(Q)
    g.search_hits(d21.data_ptr(), 0, 21, Q, 0, c.data_ptr())  # counts only
    done()
    d_kmers = torch.zeros(Q, dtype=torch.int32, device=dev)
    d_num = torch.zeros(1, dtype=torch.int32, device=dev)
    r, c = outputs(Q)
    g.search_hits_compact(d21.data_ptr(), 0, 21, Q, d_kmers.data_ptr(), r.data_ptr(), Q, d_num.data_ptr())  # the sparse list
    done()
    r, c = outputs(Q)
    g.search_hits_in_order(d21.data_ptr(), 0, 21, Q, d_kmers.data_ptr(), r.data_ptr())  # results in search order
    done()
    # the sharded calls, one shard: order, search the ordered records, the general kernel over the rest
    q21x = q21.copy()
    q21x[7::97, 3] = ord("x")
    d21x = upload(q21x)
    buckets = g.order_buckets(21, Q)
    d_rec = torch.zeros(Q, dtype=torch.int64, device=dev)
    d_bs = torch.zeros(buckets + 3, dtype=torch.int32, device=dev)
    r, c = outputs(Q)
    g.order_kmers(d21x.data_ptr(), 21, Q, 0, Q, d_rec.data_ptr(), d_bs.data_ptr())
    done()
    g.search_ordered_records(d_rec.data_ptr(), d_bs.data_ptr(), 0, buckets, 21, Q, d_kmers.data_ptr(), r.data_ptr())
    done()
    g.search_general_records(d21x.data_ptr(), 21, Q, 0, Q, d_rec.data_ptr(), d_bs.data_ptr(), d_kmers.data_ptr(), r.data_ptr())
    done()
    knobs(EXACT_LOOKUP="1")  # awfmGpuSearch through exactLookupSearchKernel
    r, c = outputs(Q)
    g.search(d21.data_ptr(), 0, 21, Q, r.data_ptr(), c.data_ptr())
    done()
    g.destroy()
    ix.dealloc()
    # an amino batch through aminoLookupSearchKernel
    knobs(AMINO_LOOKUP="1")
    atxt = synth.text(910, 150000, synth.AMINO_ALPHABET).copy()
    aix = api.create_index(atxt, api.AwFmAlphabetAmino, 8, 3)
    ag = api.GpuIndex(aix)
    ag.set_deep_seed(5)
    aq = batch(19, 40009, 10, atxt, synth.AMINO_ALPHABET)
    d_aq = upload(aq)
    r, c = outputs(40009)
    ag.search_hits(d_aq.data_ptr(), 0, 10, 40009, r.data_ptr(), c.data_ptr())
    done()
    ag.destroy()
    aix.dealloc()
    print(f"order_launch_sequence: {calls} calls")


if __name__ == "__main__":
    main()
