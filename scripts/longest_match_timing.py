#!/usr/bin/env python3
"""Times awfmGpuLongestSuffixMatches on the 3.1 Gbp synthetic index bench.py uses, inputs resident on the device, device events
around every one of --steps calls after --warmup, each leg alternating call by call with its comparator in one process;
spreads as min / median / max.

  floor21 / floor64   every query matches in full (planted 21-mers / 64-mers).  Comparator: awfmGpuSearch (exact ranges) on the
                      same batch and image; where that picks its exact-lookup kernel it is timed a second time with the
                      general searchKernel ($AWFM_GPU_EXACT_LOOKUP=0, as the parity tests select it).  Bar (against the general
                      kernel, which does the same walk): median <= comparator's median x (1 + its own (max - min) / median) x
                      the ratio of the two calls' compulsory bytes.
  reads               reads of 128 characters with 5 % substitutions, windows ending at every 4th position, cap 64 (overlapping
                      (start, end) pairs into the read buffer).  Comparator: what a caller of awfmGpuSearch can do -- bisect the
                      match length, 7 passes for a cap of 64; awfmGpuSearch takes CSR offsets, i.e. queries that tile their
                      buffer, so every pass re-gathers the candidate suffixes into a compact buffer and rebuilds the offsets
                      with torch.  It runs on the first --bisect-queries windows (the gathers need 8 bytes of index per
                      character); the new call is timed on the same windows beside it, and the results are checked equal.
                      The search passes and the gathers are timed apart.  Bar: the new call wins against the search passes alone
                      by more than the summed spreads.
  random              random 24-mers: the fall-back from an empty table entry on nearly every query; reported, no bar.

Compulsory bytes of a call: per query its characters, 16 bytes of (start, end) where given, the table entry (8), one 128-B line
per block read of the walk -- the steps beyond the depth the walk started at (a table's, or 1), two per pair read, plus the step that fails when the match is
shorter than the query -- and the outputs (24, or 20 for awfmGpuSearch); a lower bound (a wide range reads two lines per step).
--one-leg NAME runs a single leg without its comparator (for a profiler).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def count(text):
    return int(float(text))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--queries", type=count, default=100_000_000)
    p.add_argument("--bisect-queries", type=count, default=1 << 24)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--one-leg", default=None, choices=["floor21", "floor64", "reads", "random"])
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    N, n = args.queries, args.text_len
    result = {"queries": N, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK}

    def timed_pair(*fns):
        """device ms of --steps calls of every fn, the fns taking turns call by call"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        stream_obj.synchronize()
        out = [[] for _ in fns]
        for _ in range(args.steps):
            for k, fn in enumerate(fns):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream_obj)
                fn()
                b.record(stream_obj)
                stream_obj.synchronize()
                out[k].append(a.elapsed_time(b))
        return out

    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    result["index_build_s"] = round(time.time() - t0, 2)
    result["image"] = g.describe()
    D, pair = g.deep_seed_k or args.seed_k, bool(g.has_pair_image)

    d_len = torch.empty(N, dtype=torch.int32, device=dev)
    d_ranges = torch.empty(N * 2, dtype=torch.int64, device=dev)
    d_counts = torch.empty(N, dtype=torch.int32, device=dev)
    d_counts2 = torch.empty(N, dtype=torch.int32, device=dev)
    d_ranges2 = torch.empty(N * 2, dtype=torch.int64, device=dev)

    def line_bytes(lengths, query_lengths):
        """128-B lines of the walk: steps beyond the depth it started at -- the deeper table's where the match is that long, else
        the index's own table's, else 1 (r_1) --, two per pair read, plus the failing step of a partial match"""
        got = lengths.long()
        began = torch.where(got >= D, D, torch.where(got >= args.seed_k, args.seed_k, 1))
        steps = torch.clamp(got - began, min=0) + (got < query_lengths).long()
        reads = (steps + 1) // 2 if pair else steps
        return int(reads.sum().item()) * 128

    def rate(leg, bytes_moved):
        leg["compulsory_bytes"] = bytes_moved
        leg["fraction_of_hbm_peak"] = round(bytes_moved / (leg["new_call"]["median_ms"] * 1e-3) / HBM_PEAK, 4)

    def match(chars, starts, ends, fixed, count_, lengths=d_len, ranges=d_ranges, counts=d_counts):
        g.longest_suffix_matches(chars.data_ptr(), starts.data_ptr() if starts is not None else 0, ends.data_ptr() if ends is not None else 0,
                                 fixed, count_, 0, lengths.data_ptr(), ranges.data_ptr(), counts.data_ptr(), stream=stream)

    # ---- floor: every query matches in full ----
    for K in (21, 64):
        name = f"floor{K}"
        if args.one_leg not in (None, name):
            continue
        d_chars = torch.empty(N * K, dtype=torch.uint8, device=dev)
        assert L.awfmGpuSynthPlantedQueries(d_chars.data_ptr(), 0, N, K, 103 + K, d_text.data_ptr(), n, None) == 1
        torch.cuda.synchronize()

        def new_call():
            match(d_chars, None, None, K, N)

        def search():
            g.search(d_chars.data_ptr(), 0, K, N, d_ranges2.data_ptr(), d_counts2.data_ptr(), stream=stream)

        if args.one_leg:
            result[name] = {"new_call": summary(timed_pair(new_call)[0])}
            continue
        os.environ.pop("AWFM_GPU_EXACT_LOOKUP", None)
        ours, theirs = timed_pair(new_call, search)
        exact = bool(g.last_search_was_exact_lookup())
        leg = {"new_call": summary(ours), "awfmGpuSearch_default": summary(theirs), "awfmGpuSearch_default_is_exact_lookup": exact,
               "every_query_matches_in_full": bool((d_len == K).all()),
               "equal_to_awfmGpuSearch_default": torch.equal(d_ranges, d_ranges2) and torch.equal(d_counts, d_counts2)}
        general = theirs
        leg["general_kernel_selected"] = not exact
        if exact:
            os.environ["AWFM_GPU_EXACT_LOOKUP"] = "0"
            ours, general = timed_pair(new_call, search)
            leg["general_kernel_selected"] = not g.last_search_was_exact_lookup()
            leg["equal_to_awfmGpuSearch_general_kernel"] = torch.equal(d_ranges, d_ranges2) and torch.equal(d_counts, d_counts2)
            if not leg["equal_to_awfmGpuSearch_general_kernel"]:
                differ = torch.nonzero((d_ranges != d_ranges2).view(N, 2).any(1)).flatten()
                leg["first_differences"] = [(int(i), d_ranges.view(N, 2)[i].tolist(), d_ranges2.view(N, 2)[i].tolist()) for i in differ[:4]]
                leg["queries_that_differ"] = int(differ.numel())
            os.environ.pop("AWFM_GPU_EXACT_LOOKUP", None)
            leg["new_call"] = summary(ours)
        leg["awfmGpuSearch_general_kernel"] = summary(general)
        lines = line_bytes(d_len, torch.full_like(d_len, K))
        ours_bytes, theirs_bytes = N * (K + 8 + 24) + lines, N * (K + 8 + 20) + lines
        rate(leg, ours_bytes)
        cmp_ = leg["awfmGpuSearch_general_kernel"]
        if not leg["general_kernel_selected"]:  # no comparator to set the bar against
            leg["bar"] = None
            result[name] = leg
            del d_chars
            continue
        spread = (cmp_["max_ms"] - cmp_["min_ms"]) / cmp_["median_ms"]
        bound = cmp_["median_ms"] * (1.0 + spread) * ours_bytes / theirs_bytes
        leg["bar"] = {"comparator_spread": round(spread, 4), "bytes_ratio": round(ours_bytes / theirs_bytes, 4), "bound_ms": round(bound, 4),
                      "met": leg["new_call"]["median_ms"] <= bound, "ratio_to_general_kernel": round(leg["new_call"]["median_ms"] / cmp_["median_ms"], 4)}
        result[name] = leg
        del d_chars

    # ---- the reads ----
    if args.one_leg in (None, "reads"):
        R, M, CAP = N // 32, 128, 64
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        d_reads = torch.empty(R * M + 64, dtype=torch.uint8, device=dev)
        letters = torch.tensor(list(b"acgt"), dtype=torch.uint8, device=dev)
        for begin in range(0, R, 1 << 18):
            r = min(1 << 18, R - begin)
            at = torch.randint(0, n - M, (r, 1), device=dev, generator=gen)
            piece = d_text[at + torch.arange(M, device=dev)]
            swap = torch.rand((r, M), device=dev, generator=gen) < 0.05
            piece = torch.where(swap, letters[torch.randint(0, 4, (r, M), device=dev, generator=gen)], piece)
            d_reads[begin * M:(begin + r) * M] = piece.reshape(-1)
        e = torch.arange(4, M + 1, 4, device=dev)
        base = (torch.arange(R, device=dev) * M).unsqueeze(1)
        d_ends = (base + e).reshape(-1).contiguous()
        d_starts = (base + torch.clamp(e - CAP, min=0)).reshape(-1).contiguous()
        W = d_ends.numel()
        torch.cuda.synchronize()

        def new_all():
            match(d_reads, d_starts, d_ends, 0, W)

        leg = {"windows": W, "new_call": summary(timed_pair(new_all)[0])}
        hist = torch.bincount(d_len[:W].long(), minlength=CAP + 1)
        leg["match_length_histogram"] = hist.cpu().tolist()
        rate(leg, W * 40 + R * M + W * 8 + line_bytes(d_len[:W], (d_ends - d_starts)))
        if not args.one_leg:
            B = min(args.bisect_queries, W)
            b_starts, b_ends = d_starts[:B].contiguous(), d_ends[:B].contiguous()
            b_len = torch.empty(B, dtype=torch.int32, device=dev)
            times = {"gather": [], "search": []}
            final = {}

            def new_part():
                match(d_reads, b_starts, b_ends, 0, B, lengths=b_len)

            def bisect():
                """lo: a suffix of that length occurs (0: trivially); hi: one of that length does not (query length + 1: trivially)"""
                with torch.cuda.stream(stream_obj):
                    lo = torch.zeros(B, dtype=torch.int64, device=dev)
                    hi = (b_ends - b_starts) + 1
                    gather_ms = search_ms = 0.0
                    for _ in range(7):
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                        ev[0].record(stream_obj)
                        mid = (lo + hi) // 2
                        off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
                        off[1:] = torch.cumsum(mid, 0)
                        owner = torch.repeat_interleave(torch.arange(B, device=dev), mid)
                        src = (b_ends - mid)[owner] + (torch.arange(owner.numel(), device=dev) - off[owner])
                        buf = torch.cat([d_reads[src], torch.zeros(8, dtype=torch.uint8, device=dev)])
                        ev[1].record(stream_obj)
                        g.search(buf.data_ptr(), off.data_ptr(), 0, B, 0, d_counts2.data_ptr(), stream=stream)
                        ev[2].record(stream_obj)
                        found = (d_counts2[:B] > 0) | (mid == 0)
                        lo = torch.where(found, mid, lo)
                        hi = torch.where(found, hi, mid)
                        stream_obj.synchronize()
                        gather_ms += ev[0].elapsed_time(ev[1])
                        search_ms += ev[1].elapsed_time(ev[2])
                        del owner, src, buf
                    final["lo"] = lo
                    times["gather"].append(gather_ms)
                    times["search"].append(search_ms)

            steps = args.steps
            for fn in (new_part, bisect):
                fn()
            stream_obj.synchronize()
            times = {"gather": [], "search": []}
            ours = []
            for _ in range(steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream_obj)
                new_part()
                b.record(stream_obj)
                stream_obj.synchronize()
                ours.append(a.elapsed_time(b))
                bisect()
            equal = torch.equal(final["lo"], b_len.long())
            new_s, search_s, gather_s = summary(ours), summary(times["search"]), summary(times["gather"])
            spreads = (new_s["max_ms"] - new_s["min_ms"]) + (search_s["max_ms"] - search_s["min_ms"])
            leg["bisection"] = {"windows": B, "passes": 7, "new_call_same_windows": new_s, "awfmGpuSearch_passes": search_s,
                                "torch_gathers_and_offsets": gather_s, "results_equal": equal,
                                "speedup_over_search_passes": round(search_s["median_ms"] / new_s["median_ms"], 3),
                                "speedup_over_passes_and_gathers": round((search_s["median_ms"] + gather_s["median_ms"]) / new_s["median_ms"], 3),
                                "summed_spreads_ms": round(spreads, 4),
                                "bar_met": search_s["median_ms"] - new_s["median_ms"] > spreads}
        result["reads"] = leg
        del d_reads, d_starts, d_ends

    # ---- random strings ----
    if args.one_leg in (None, "random"):
        K = 24
        d_chars = torch.empty(N * K, dtype=torch.uint8, device=dev)
        assert L.awfmGpuSynthRandomQueries(d_chars.data_ptr(), 0, N, K, 9, 0, None) == 1
        torch.cuda.synchronize()
        leg = {"new_call": summary(timed_pair(lambda: match(d_chars, None, None, K, N))[0])}
        leg["match_length_histogram"] = torch.bincount(d_len.long(), minlength=K + 1).cpu().tolist()
        rate(leg, N * (K + 8 + 24) + line_bytes(d_len, torch.full_like(d_len, K)))
        result["random"] = leg

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
