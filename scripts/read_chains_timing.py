#!/usr/bin/env python3
"""Times awfmGpuReadChains on the 3.1 Gbp synthetic index bench.py uses, on the batch scripts/read_candidates_timing.py uses:
located, mapped and clustered hits resident on the device.  Device events around every one of --steps calls after --warmup, the
sides taking turns call by call in one process; spreads as min / median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions; the longest match ending at every
              4th position, cap 64, minLength 16 (awfmGpuLongestSuffixMatches); hit offsets, awfmGpuLocate,
              awfmGpuLocalPositions against a record table of --records equal records and awfmGpuReadCandidates (4 slots,
              maxHitsPerSeed 32, band 8, minVotes 2), all before the clock starts.
  new call    awfmGpuReadChains on those slots with every output, lookback 64, gapPenalty 1.
  candidates  awfmGpuReadCandidates on the same batch in the same process: both calls stream the same hits, so the ratio is what
              the sort's payload and the recurrence cost.  Reported, no bar.
  host twin   awfmReadChains on --threads (16) threads over the same arrays copied to the host: what a caller has today.  Wall
              clock.  Every output of the new call is compared with it, all reads, in the same run.
  bar         the new call's median lies below the host twin's median by more than the sum of the two sides' max - min.
  floor       a device-to-device copy of the bytes the call must read and write (inputs and slots once, outputs once); no bar.
  long read   the same batch, and again with ONE more read of 4096 hits that all lie in one slot on one diagonal with growing
              seed ends: 4096 sequential steps of one wave, the longest recurrence a read can hold.

Prints one JSON line and writes it to --out (default profiles/read_chains/timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 150, 4, 64, 16, 32, 8, 2, 4, 64, 1
CANDIDATE_FIELDS = (("sequences", "int32"), ("diagonals", "int64"), ("votes", "int32"), ("diagonalSpans", "int32"), ("readBegins", "int32"),
                    ("readEnds", "int32"))
CHAIN_FIELDS = (("chainScores", "int32"), ("chainAnchors", "int32"), ("chainReadBegins", "int32"), ("chainReadEnds", "int32"),
                ("chainBeginDiagonals", "int64"), ("chainEndDiagonals", "int64"))


def count(text):
    return int(float(text))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--reads", type=count, default=1 << 20)
    p.add_argument("--records", type=int, default=24)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join("profiles", "read_chains", "timing.json"))
    args = p.parse_args()

    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    R, n, M = args.reads, args.text_len, READ_LENGTH
    result = {"reads": R, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "parameters": {"read_length": M, "step": STEP, "cap": CAP, "min_length": MIN_LENGTH, "max_hits_per_seed": MAX_HITS_PER_SEED,
                             "band": BAND, "min_votes": MIN_VOTES, "slots": SLOTS, "lookback": LOOKBACK, "gap_penalty": GAP_PENALTY,
                             "records": args.records, "host_threads": args.threads}}

    def timed(*fns, host=()):
        """ms of --steps calls of every fn, the fns taking turns call by call: device events, wall clock for the fns in `host`"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        stream_obj.synchronize()
        out = [[] for _ in fns]
        for _ in range(args.steps):
            for k, fn in enumerate(fns):
                if fn in host:
                    t = time.perf_counter()
                    fn()
                    out[k].append((time.perf_counter() - t) * 1e3)
                    continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream_obj)
                fn()
                b.record(stream_obj)
                stream_obj.synchronize()
                out[k].append(a.elapsed_time(b))
        return out

    # ---- the index, the reads, their seeds, located and mapped: all before the clock starts ----
    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    g.set_record_table(np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64))
    result["index_build_s"] = round(time.time() - t0, 2)
    result["image"] = g.describe()

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
    del d_text
    e = torch.arange(STEP, M + 1, STEP, device=dev)
    per_read = e.numel()
    base = (torch.arange(R, device=dev) * M).unsqueeze(1)
    d_ends = (base + e).reshape(-1).contiguous()
    d_starts = (base + torch.clamp(e - CAP, min=0)).reshape(-1).contiguous()
    S = d_ends.numel()
    d_seed_ends = e.to(torch.int32).repeat(R).contiguous()
    d_read_offsets = (torch.arange(R + 1, device=dev) * per_read).contiguous()
    d_lengths = torch.empty(S, dtype=torch.int32, device=dev)
    d_ranges = torch.empty(S * 2, dtype=torch.int64, device=dev)
    d_counts = torch.empty(S, dtype=torch.int32, device=dev)
    d_hit_offsets = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_scan = torch.zeros(api.GpuIndex.scan_scratch_bytes(S), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.longest_suffix_matches(d_reads.data_ptr(), d_starts.data_ptr(), d_ends.data_ptr(), 0, S, MIN_LENGTH, d_lengths.data_ptr(),
                             d_ranges.data_ptr(), d_counts.data_ptr(), stream=stream)
    H = g.hit_offsets_from_counts(d_counts.data_ptr(), S, d_hit_offsets.data_ptr(), d_scan.data_ptr(), stream=stream)
    d_positions = torch.empty(max(H, 1), dtype=torch.int64, device=dev)
    d_sequences = torch.empty(max(H, 1), dtype=torch.int32, device=dev)
    d_illegal = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), S, H, d_positions.data_ptr(), stream=stream)
    g.local_positions(d_positions.data_ptr(), H, d_sequences.data_ptr(), d_positions.data_ptr(), d_num_illegal=d_illegal.data_ptr(), stream=stream)
    stream_obj.synchronize()
    del d_reads, d_starts, d_ends, d_ranges, d_scan
    torch.cuda.empty_cache()
    result.update(seeds=S, hits=H, illegal_hits=int(d_illegal.item()), largest_seed=int(d_counts.max().item()),
                  seeds_above_max_hits=int((d_counts.long() > MAX_HITS_PER_SEED).sum().item()))

    # ---- the candidates, and the new call on their slots ----
    def candidates_on(reads, cin):
        out = {name: torch.empty(reads * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CANDIDATE_FIELDS}
        out["numCandidates"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["keptHits"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["numOverflowed"] = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(api.read_candidates_scratch_bytes(reads), dtype=torch.uint8, device=dev)
        cout = api.candidate_outputs(**{name: t.data_ptr() for name, t in out.items()})
        torch.cuda.synchronize()

        def call():
            g.read_candidates(cin, reads, cout, scratch.data_ptr(), max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, min_votes=MIN_VOTES,
                              max_candidates=SLOTS, stream=stream)
        return call, out, (cout, scratch)

    def chains_on(reads, cin, slots):
        out = {name: torch.empty(reads * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CHAIN_FIELDS}
        out["bestSlots"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["keptHits"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["numOverflowed"] = torch.zeros(1, dtype=torch.int64, device=dev)
        scratch = torch.empty(api.read_chains_scratch_bytes(reads), dtype=torch.uint8, device=dev)
        cout = api.chain_outputs(**{name: t.data_ptr() for name, t in out.items()})
        torch.cuda.synchronize()

        def call():
            g.read_chains(cin, reads, slots[0].data_ptr(), slots[1].data_ptr(), slots[2].data_ptr(), cout, scratch.data_ptr(),
                          max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, max_candidates=SLOTS, lookback=LOOKBACK, gap_penalty=GAP_PENALTY,
                          stream=stream)
        return call, out, (cout, scratch)

    cin = api.candidate_inputs(d_read_offsets.data_ptr(), S, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), H,
                               d_positions.data_ptr(), d_sequences.data_ptr())
    candidates, cand_out, keep1 = candidates_on(R, cin)
    candidates()
    stream_obj.synchronize()
    slots = [cand_out["sequences"].clone(), cand_out["diagonals"].clone(), cand_out["diagonalSpans"].clone()]
    new_call, new_out, keep2 = chains_on(R, cin, slots)

    # ---- the host twin on the same arrays ----
    host_in = [t.cpu().numpy() for t in (d_read_offsets, d_seed_ends, d_lengths, d_hit_offsets, d_positions[:H], d_sequences[:H])]
    host_slots = [t.cpu().numpy() for t in slots]
    host_out = {name: np.zeros(R * SLOTS, getattr(np, dtype)) for name, dtype in CHAIN_FIELDS}
    host_out.update(bestSlots=np.zeros(R, np.int32), keptHits=np.zeros(R, np.int32), numOverflowed=np.zeros(1, np.int64))
    hin = api.candidate_inputs(host_in[0].ctypes.data, S, host_in[1].ctypes.data, host_in[2].ctypes.data, 0, host_in[3].ctypes.data, H,
                               host_in[4].ctypes.data, host_in[5].ctypes.data)
    hout = api.chain_outputs(**{name: a.ctypes.data for name, a in host_out.items()})

    def host_twin():
        rc = L.awfmReadChains(C.byref(hin), R, MAX_HITS_PER_SEED, BAND, SLOTS, host_slots[0].ctypes.data, host_slots[1].ctypes.data,
                              host_slots[2].ctypes.data, LOOKBACK, GAP_PENALTY, C.byref(hout), args.threads)
        assert rc == _lib.AwFmSuccess, rc

    ours, theirs, cands = timed(new_call, host_twin, candidates, host=(host_twin,))
    calls = args.steps + args.warmup
    equal = {name: bool(np.array_equal(new_out[name].cpu().numpy(), host_out[name])) for name in host_out if name != "numOverflowed"}
    equal["numOverflowed"] = int(new_out["numOverflowed"].item()) == int(host_out["numOverflowed"][0])
    new_s, host_s, cand_s = summary(ours), summary(theirs), summary(cands)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (host_s["max_ms"] - host_s["min_ms"])
    anchors = new_out["chainAnchors"].view(R, SLOTS)
    best = new_out["bestSlots"].long()
    chained = best >= 0
    result.update(new_call=new_s, host_twin=host_s, candidates_call=cand_s, results_equal=all(equal.values()), results_equal_by_output=equal,
                  reads_compared=R, overflowed_reads=int(new_out["numOverflowed"].item()) // calls,
                  reads_with_a_chain=int(chained.sum().item()), largest_read_kept_hits=int(new_out["keptHits"].max().item()),
                  mean_anchors_of_the_best_chain=round(float(anchors[chained, best[chained]].float().mean().item()), 2),
                  new_call_over_candidates=round(new_s["median_ms"] / cand_s["median_ms"], 3),
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(host_s["median_ms"] / new_s["median_ms"], 3),
                       "met": host_s["median_ms"] - new_s["median_ms"] > spreads})

    # ---- the floor: the bytes the call must read and write, copied once ----
    must = 8 * (R + 1) + 8 * S + 8 * (S + 1) + 12 * H + R * SLOTS * 16 + R * (SLOTS * 32 + 8)
    src, dst = torch.empty(must, dtype=torch.uint8, device=dev), torch.empty(must, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream_obj):
            dst.copy_(src)

    floor = summary(timed(copy)[0])
    result["floor"] = {"bytes": must, "copy": floor, "new_call_over_copy": round(new_s["median_ms"] / floor["median_ms"], 2)}
    del src, dst

    # ---- one more read: 4096 hits in one slot, one diagonal, every seed ending one character after the one before ----
    X, base = 4096, 1 << 20
    extra = torch.arange(X, device=dev)
    l_read_offsets = torch.cat([d_read_offsets, torch.tensor([S + X], device=dev)])
    l_seed_ends = torch.cat([d_seed_ends, (CAP + extra).to(torch.int32)])
    l_lengths = torch.cat([d_lengths, torch.full((X,), CAP, dtype=torch.int32, device=dev)])
    l_hit_offsets = torch.cat([d_hit_offsets, H + 1 + extra])
    l_positions = torch.cat([d_positions[:H], base + extra])
    l_sequences = torch.cat([d_sequences[:H], torch.zeros(X, dtype=torch.int32, device=dev)])
    l_slots = [torch.cat([slots[0], torch.tensor([0, -1, -1, -1], dtype=torch.int32, device=dev)]),
               torch.cat([slots[1], torch.tensor([base, 0, 0, 0], dtype=torch.int64, device=dev)]),
               torch.cat([slots[2], torch.zeros(SLOTS, dtype=torch.int32, device=dev)])]
    lin = api.candidate_inputs(l_read_offsets.data_ptr(), S + X, l_seed_ends.data_ptr(), l_lengths.data_ptr(), 0, l_hit_offsets.data_ptr(), H + X,
                               l_positions.data_ptr(), l_sequences.data_ptr())
    longer, long_out, keep3 = chains_on(R + 1, lin, l_slots)
    a, b = timed(new_call, longer)
    result["single_slot_read"] = {"hits_of_the_one_read": X, "without_it": summary(a), "with_it": summary(b),
                                  "its_chain": {"score": int(long_out["chainScores"][R * SLOTS].item()),
                                                "anchors": int(long_out["chainAnchors"][R * SLOTS].item()),
                                                "expected_score": CAP + X - 1, "expected_anchors": X}}

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
