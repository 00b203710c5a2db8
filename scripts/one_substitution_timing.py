#!/usr/bin/env python3
"""Times awfmGpuOneSubstitutionSearch on the 3.1 Gbp synthetic index bench.py uses (pair image, deeper table 16), inputs resident
on the device, device events around every one of --steps calls after --warmup, each leg alternating call by call with its
comparator in one process; spreads as min / median / max.

  planted21 / planted32   k-mers drawn from the text with exactly one position replaced by another letter
  random21                random 21-mers

Comparator: what a caller runs without the call -- all 3m + 1 strings within Hamming distance 1 of every k-mer enumerated with
torch, awfmGpuSearchHits on that batch, awfmGpuCompactHits on its results.  The whole path is timed, and its search and compact
passes apart.  The records of the two sides are checked equal (as sorted (query, edit, range) lists).  Bar, on both 21-mer legs:
the new call's median lies below the comparator's whole-path median by more than the two sides' summed (max - min).  Peak device
bytes of a side: what it allocates beyond the index and the k-mers -- outputs, temporaries, and the growth of the image's own
scratch.  Prints one JSON line and writes it to --out; any failure ends the run."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NONE = 0xFFFFFFFF


def count(text):
    return int(float(text))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--queries", type=count, default=1 << 22)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--device-seed-k", type=int, default=16)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--legs", nargs="+", default=["planted21", "random21", "planted32"])
    p.add_argument("--out", default=os.path.join("profiles", "one_substitution", "timing.json"))
    args = p.parse_args()

    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    N, n = args.queries, args.text_len
    result = {"queries": N, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}

    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    g.set_pair_image(1)
    if g.deep_seed_k != args.device_seed_k:
        g.set_deep_seed(args.device_seed_k)
    torch.cuda.synchronize()
    result["index_build_s"] = round(time.time() - t0, 2)
    result["image"] = g.describe()
    assert g.has_pair_image and g.deep_seed_k == args.device_seed_k
    letters = torch.tensor(list(b"acgt"), dtype=torch.uint8, device=dev)
    code_of = torch.zeros(256, dtype=torch.int64, device=dev)
    code_of[letters.long()] = torch.arange(4, device=dev)

    def sides(fns):
        """device ms of --steps calls of every fn (each returns nothing or a dict of extra timings), the fns taking turns"""
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

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before, image_before = torch.cuda.memory_allocated(), g.device_bytes
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before + (g.device_bytes - image_before)
        return peak, keep

    bars = []
    for leg_name in args.legs:
        K = int(leg_name[-2:])
        V = 3 * K + 1
        d_chars = torch.empty(N * K, dtype=torch.uint8, device=dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(K)
        if leg_name.startswith("planted"):
            assert L.awfmGpuSynthPlantedQueries(d_chars.data_ptr(), 0, N, K, 103 + K, d_text.data_ptr(), n, None) == 1
            torch.cuda.synchronize()
            q2 = d_chars.view(N, K)
            at = torch.randint(0, K, (N,), device=dev, generator=gen)
            rows = torch.arange(N, device=dev)
            old = code_of[q2[rows, at].long()]
            q2[rows, at] = letters[(old + torch.randint(1, 4, (N,), device=dev, generator=gen)) % 4]
        else:
            assert L.awfmGpuSynthRandomQueries(d_chars.data_ptr(), 0, N, K, 9, 0, None) == 1
        torch.cuda.synchronize()

        # ---- the new call: sized by a counting call, then timed with its lists ----
        d_total = torch.zeros(1, dtype=torch.int64, device=dev)
        g.one_substitution_search(d_chars.data_ptr(), 0, K, N, True, 0, 0, 0, 0, d_total.data_ptr(), 0, 0, stream=stream)
        stream_obj.synchronize()
        records = int(d_total.item())
        cap = records + 1024
        ours = {}

        def new_alloc():
            ours["q"] = torch.empty(cap, dtype=torch.int32, device=dev)
            ours["e"] = torch.empty(cap, dtype=torch.int32, device=dev)
            ours["r"] = torch.empty(cap * 2, dtype=torch.int64, device=dev)
            ours["var"] = torch.empty(N, dtype=torch.int32, device=dev)
            ours["occ"] = torch.empty(N, dtype=torch.int64, device=dev)
            new_call()

        def new_call():
            g.one_substitution_search(d_chars.data_ptr(), 0, K, N, True, ours["q"].data_ptr(), ours["e"].data_ptr(), ours["r"].data_ptr(), cap,
                                      d_total.data_ptr(), ours["var"].data_ptr(), ours["occ"].data_ptr(), stream=stream)

        new_peak, _ = peak_of(new_alloc)

        # ---- the comparator: enumerate, search, compact ----
        theirs, parts = {}, {"enumerate": [], "search": [], "compact": []}

        def enumerate_strings():
            q2 = d_chars.view(N, K)
            out = q2.unsqueeze(1).expand(N, V, K).contiguous()
            alt = letters[(code_of[q2.long()].unsqueeze(2) + 1 + torch.arange(3, device=dev)) % 4]  # [N, K, 3]
            out[:, :3 * K].view(N, K, 3, K).diagonal(dim1=1, dim2=3).copy_(alt.permute(0, 2, 1))
            return out

        def old_path():
            with torch.cuda.stream(stream_obj):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                ev[0].record(stream_obj)
                strings = enumerate_strings()
                M = N * V
                d_ranges = torch.empty(M * 2, dtype=torch.int64, device=dev)
                d_counts = torch.empty(M, dtype=torch.int32, device=dev)
                d_flags = torch.empty(M + 1, dtype=torch.int64, device=dev)
                d_scratch = torch.empty(api.GpuIndex.scan_scratch_bytes(M), dtype=torch.uint8, device=dev)
                d_kmers = torch.empty(cap, dtype=torch.int32, device=dev)
                d_hits = torch.empty(cap * 2, dtype=torch.int64, device=dev)
                d_num = torch.zeros(1, dtype=torch.int32, device=dev)
                ev[1].record(stream_obj)
                g.search_hits(strings.data_ptr(), 0, K, M, d_ranges.data_ptr(), d_counts.data_ptr(), stream=stream)
                ev[2].record(stream_obj)
                g.compact_hits(d_counts.data_ptr(), d_ranges.data_ptr(), M, d_flags.data_ptr(), d_scratch.data_ptr(), d_kmers.data_ptr(),
                               d_hits.data_ptr(), cap, d_num.data_ptr(), stream=stream)
                ev[3].record(stream_obj)
                stream_obj.synchronize()
                for k, name in enumerate(("enumerate", "search", "compact")):
                    parts[name].append(ev[k].elapsed_time(ev[k + 1]))
                theirs.update(kmers=d_kmers, hits=d_hits, num=d_num)

        old_peak, _ = peak_of(old_path)
        parts = {"enumerate": [], "search": [], "compact": []}
        new_ms, old_ms = sides([new_call, old_path])
        for name in parts:
            parts[name] = parts[name][-args.steps:]

        # ---- equal results ----
        assert int(d_total.item()) == records and int(theirs["num"].item()) == records, (records, int(theirs["num"].item()))
        key_new = (ours["q"][:records].long() & 0xFFFFFFFF) << 32 | (ours["e"][:records].long() & 0xFFFFFFFF)
        order_new = torch.argsort(key_new)
        idx = theirs["kmers"][:records].long() & 0xFFFFFFFF
        query, v = idx // V, idx % V
        pos = torch.clamp(v // 3, max=K - 1)
        own = code_of[d_chars.view(N, K)[query, pos].long()]
        edit = torch.where(v == 3 * K, torch.full_like(v, NONE), pos * 32 + (own + 1 + v % 3) % 4)
        key_old = query << 32 | edit
        order_old = torch.argsort(key_old)
        equal = (torch.equal(key_new[order_new], key_old[order_old]) and
                 torch.equal(ours["r"][:2 * records].view(records, 2)[order_new], theirs["hits"][:2 * records].view(records, 2)[order_old]))
        assert equal, leg_name

        new_s, old_s = summary(new_ms), summary(old_ms)
        spreads = (new_s["max_ms"] - new_s["min_ms"]) + (old_s["max_ms"] - old_s["min_ms"])
        leg = {"k": K, "strings_per_kmer": V, "records": records, "occurrences": int(ours["occ"].sum().item()),
               "new_call": new_s, "comparator_whole_path": old_s, "comparator_enumerate": summary(parts["enumerate"]),
               "comparator_search": summary(parts["search"]), "comparator_compact": summary(parts["compact"]),
               "results_equal": bool(equal), "new_call_peak_device_bytes": int(new_peak), "comparator_peak_device_bytes": int(old_peak),
               "summed_spreads_ms": round(spreads, 4), "speedup_over_whole_path": round(old_s["median_ms"] / new_s["median_ms"], 3),
               "speedup_over_search_pass_alone": round(summary(parts["search"])["median_ms"] / new_s["median_ms"], 3)}
        if K == 21:
            leg["bar_met"] = bool(old_s["median_ms"] - new_s["median_ms"] > spreads)
            bars.append(leg["bar_met"])
        result[leg_name] = leg
        del d_chars, ours, theirs
        torch.cuda.empty_cache()

    result["bar_met_on_both_21_mer_legs"] = bool(len(bars) == 2 and all(bars))
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
