#!/usr/bin/env python3
"""Times awfmGpuAlignChainsAffine on the 3.1 Gbp synthetic index bench.py uses, on the batch scripts/align_chains_timing.py uses:
located, mapped, clustered, chained and verified hits resident on the device, the text uploaded with awfmGpuIndexSetText.  Device
events around every one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as min /
median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions; the longest match ending at every
              4th position, cap 64, minLength 16; hit offsets, awfmGpuLocate, awfmGpuLocalPositions against a record table of
              --records equal records, awfmGpuReadCandidates (4 slots, maxHitsPerSeed 32, band 8, minVotes 2), awfmGpuReadChains
              (lookback 64, gapPenalty 1) and awfmGpuVerifyChains (bandPad 8, maxDrift 15), all before the clock starts.
  new call    awfmGpuAlignChainsAffine on verification's bestSlots with every output, scoring (1, 4, 6, 1), bandPad 8, maxDrift
              15, maxOps 32, maxRows 150.
  host twin   awfmAlignChainsAffine on --threads (16) threads over the same arrays copied to the host: what a caller has today.
              Wall clock.  Every output of the new call is compared with it, all reads, in the same run (the rows of ops up to
              each read's numOps; truncated rows not at all).
  bar         the new call's median lies below the host twin's median by more than the sum of the two sides' max - min.
  unit call   awfmGpuAlignChains on the same batch in the same process, as context.  Reported, no bar.

Prints one JSON line and writes it to --out (default profiles/align_affine/timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 150, 4, 64, 16, 32, 8, 2, 4, 64, 1
BAND_PAD, MAX_DRIFT, MAX_OPS, SCORING = 8, 15, 32, (1, 4, 6, 1)
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
    p.add_argument("--out", default=os.path.join("profiles", "align_affine", "timing.json"))
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
                             "records": args.records, "host_threads": args.threads, "band_pad": BAND_PAD, "max_drift": MAX_DRIFT,
                             "max_ops": MAX_OPS, "max_rows": READ_LENGTH, "scoring": list(SCORING)}}

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
    host_text = d_text.cpu().numpy()
    torch.cuda.synchronize()
    g.set_text(host_text)
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
    torch.cuda.empty_cache()
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
    stream_obj.synchronize()
    g.local_positions(d_positions.data_ptr(), H, d_sequences.data_ptr(), d_positions.data_ptr(), d_num_illegal=d_illegal.data_ptr(), stream=stream)
    stream_obj.synchronize()
    del d_starts, d_ends, d_ranges, d_scan
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
    chains_call, chain_out, keep2 = chains_on(R, cin, slots)
    chains_call()
    stream_obj.synchronize()

    # ---- the new call on those chains, and the host twin on the same arrays ----
    d_char_offsets = (torch.arange(R + 1, device=dev) * M).contiguous()
    slot_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    d_slots = dict({name: chain_out[name].clone() for name in slot_names}, sequences=slots[0])
    new_out = {"editDistances": torch.empty(R * SLOTS, dtype=torch.int32, device=dev), "bestSlots": torch.empty(R, dtype=torch.int32, device=dev),
               "numUnverified": torch.zeros(1, dtype=torch.int64, device=dev)}
    vin = api.verify_inputs(d_reads.data_ptr(), R * M, d_char_offsets.data_ptr(), **{name: t.data_ptr() for name, t in d_slots.items()})
    vout = api.verify_outputs(**{name: t.data_ptr() for name, t in new_out.items()})
    torch.cuda.synchronize()

    def verify_call():
        g.verify_chains(vin, R, vout, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, stream=stream)

    verify_call()
    stream_obj.synchronize()
    d_best = new_out["bestSlots"].clone()
    unit_fields = (("editDistances", "int32", R), ("textBegins", "int64", R), ("textEnds", "int64", R), ("numOps", "int32", R), ("ops", "int32", R * MAX_OPS),
                   ("numUnaligned", "int64", 1), ("numTruncated", "int64", 1))
    unit_out = {name: torch.zeros(size, dtype=getattr(torch, dtype), device=dev) for name, dtype, size in unit_fields}
    d_unit_trace = torch.empty(g.align_chains_scratch_bytes(M), dtype=torch.uint8, device=dev)
    uout = api.align_outputs(**{name: t.data_ptr() for name, t in unit_out.items()})

    def unit_call():
        g.align_chains(vin, d_best.data_ptr(), R, uout, d_unit_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                       max_ops=MAX_OPS, max_rows=M, stream=stream)

    affine_fields = (("scores", "int32", R), ("editDistances", "int32", R), ("readBegins", "int32", R), ("readEnds", "int32", R), ("textBegins", "int64", R),
                     ("textEnds", "int64", R), ("numOps", "int32", R), ("ops", "int32", R * MAX_OPS), ("numUnaligned", "int64", 1), ("numTruncated", "int64", 1))
    affine_out = {name: torch.zeros(size, dtype=getattr(torch, dtype), device=dev) for name, dtype, size in affine_fields}
    scratch_bytes = g.align_chains_affine_scratch_bytes(M)
    d_trace = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    aout = api.affine_outputs(**{name: t.data_ptr() for name, t in affine_out.items()})
    costs = api.align_scoring(*SCORING)
    torch.cuda.synchronize()

    def new_call():
        g.align_chains_affine(vin, d_best.data_ptr(), R, aout, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                              scoring=costs, max_ops=MAX_OPS, max_rows=M, stream=stream)

    host_chars, host_offsets = d_reads[:R * M].cpu().numpy(), d_char_offsets.cpu().numpy()
    host_slots = {name: t.cpu().numpy() for name, t in d_slots.items()}
    host_best = d_best.cpu().numpy()
    host_ends = np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64)
    host_out = {name: np.zeros(size, getattr(np, dtype)) for name, dtype, size in affine_fields}
    hin = api.verify_inputs(host_chars.ctypes.data, R * M, host_offsets.ctypes.data, **{name: a.ctypes.data for name, a in host_slots.items()})
    hout = api.affine_outputs(**{name: a.ctypes.data for name, a in host_out.items()})

    def host_twin():
        rc = L.awfmAlignChainsAffine(C.byref(hin), host_best.ctypes.data, R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(costs), MAX_OPS, host_text.ctypes.data, n,
                                     host_ends.ctypes.data, args.records, api.AwFmAlphabetDna, C.byref(hout), args.threads)
        assert rc == _lib.AwFmSuccess, rc

    ours, theirs, unit_ms = timed(new_call, host_twin, unit_call, host=(host_twin,))
    got = {name: t.cpu().numpy() for name, t in affine_out.items()}
    equal = {name: bool(np.array_equal(got[name], host_out[name])) for name in host_out if name != "ops"}
    # the rows of ops: the runs of every read that is not truncated (what lies behind them is not written by either side)
    counts = got["numOps"].astype(np.int64)
    live = (np.arange(MAX_OPS)[None, :] < counts[:, None]) & (counts[:, None] <= MAX_OPS)
    equal["ops"] = bool(np.array_equal(got["ops"].reshape(R, MAX_OPS)[live], host_out["ops"].reshape(R, MAX_OPS)[live]))
    new_s, host_s, unit_s = summary(ours), summary(theirs), summary(unit_ms)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (host_s["max_ms"] - host_s["min_ms"])
    scores = got["scores"].astype(np.int64) & 0xFFFFFFFF
    aligned = (scores > 0) & (scores < 0xFFFFFFFC)
    clipped = aligned & ((got["readBegins"] > 0) | (got["readEnds"].astype(np.int64) < M))
    unit_distances = unit_out["editDistances"].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    calls = args.steps + args.warmup
    result.update(new_call=new_s, host_twin=host_s, unit_call=unit_s, results_equal=all(equal.values()), results_equal_by_output=equal,
                  reads_compared=R, scratch_bytes=scratch_bytes, reads_aligned=int(aligned.sum()), reads_unused=int((scores == 0xFFFFFFFF).sum()),
                  reads_score_zero=int((scores == 0).sum()), reads_clipped=int(clipped.sum()), reads_unaligned=int(got["numUnaligned"][0]) // calls,
                  reads_truncated=int(got["numTruncated"][0]) // calls, reads_overhanging_in_unit_call=int((unit_distances == 0xFFFFFFFB).sum()),
                  mean_score=round(float(scores[aligned].mean()), 3), mean_distance=round(float(got["editDistances"][aligned].mean()), 3),
                  mean_runs=round(float(counts[aligned].mean()), 3), most_runs=int(counts.max()),
                  new_call_over_unit_call=round(new_s["median_ms"] / unit_s["median_ms"], 3),
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(host_s["median_ms"] / new_s["median_ms"], 3),
                       "met": bool(host_s["median_ms"] - new_s["median_ms"] > spreads)})

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
