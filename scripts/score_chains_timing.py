#!/usr/bin/env python3
"""Times awfmGpuScoreChainsAffine on the 3.1 Gbp synthetic index bench.py uses, on the batch scripts/align_affine_timing.py uses:
located, mapped, clustered and chained hits resident on the device, the text uploaded with awfmGpuIndexSetText.  Device events
around every one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as min / median /
max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions; the longest match ending at every
              4th position, cap 64, minLength 16; hit offsets, awfmGpuLocate, awfmGpuLocalPositions against a record table of
              --records equal records, awfmGpuReadCandidates (4 slots, maxHitsPerSeed 32, band 8, minVotes 2) and
              awfmGpuReadChains (lookback 64, gapPenalty 1), all before the clock starts.
  new call    awfmGpuScoreChainsAffine with every output, scoring (1, 4, 6, 1), bandPad 8, maxDrift 15, minScore 30, mapqCap 60.
  comparator  what a caller runs today for the same numbers: four awfmGpuAlignChainsAffine calls, one per constant slot array,
              ops NULL, maxRows 150 -- timed as the calls alone, and again with the torch reduction that derives the best and the
              second score from the four score arrays (no duplicate rule, no mapping quality).
  bar         the new call's median lies below the comparator's calls-alone median by more than the sum of the two sides' max - min.
  parity      every output of the new call against awfmScoreChainsAffine on --threads (16) threads over the same arrays copied to
              the host, all reads, in the same run; and its three per-slot outputs against the comparator's.
  context     awfmGpuVerifyChains and ONE awfmGpuAlignChainsAffine call (verification's bestSlots, every output) on the batch in
              the same process, and the host twin's wall clock.  Reported, no bar.

Prints one JSON line and writes it to --out (default profiles/score_chains/timing.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 150, 4, 64, 16, 32, 8, 2, 4, 64, 1
BAND_PAD, MAX_DRIFT, MAX_OPS, SCORING, MIN_SCORE, MAPQ_CAP = 8, 15, 32, (1, 4, 6, 1), 30, 60
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
    p.add_argument("--out", default=os.path.join("profiles", "score_chains", "timing.json"))
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
                             "max_ops": MAX_OPS, "max_rows": READ_LENGTH, "scoring": list(SCORING), "min_score": MIN_SCORE, "mapq_cap": MAPQ_CAP}}

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

    # ---- the sides ----
    costs = api.align_scoring(*SCORING)
    score_fields = (("slotScores", "int32", R * SLOTS), ("slotReadEnds", "int32", R * SLOTS), ("slotTextEnds", "int64", R * SLOTS), ("bestSlots", "int32", R),
                    ("bestScores", "int32", R), ("secondSlots", "int32", R), ("secondScores", "int32", R), ("mappingQualities", "uint8", R),
                    ("numUnscored", "int64", 1), ("numMapped", "int64", 1))
    score_out = {name: torch.zeros(size, dtype=getattr(torch, dtype), device=dev) for name, dtype, size in score_fields}
    sout = api.slot_score_outputs(**{name: t.data_ptr() for name, t in score_out.items()})

    def new_call():
        g.score_chains_affine(vin, R, sout, max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=costs, min_score=MIN_SCORE,
                              mapq_cap=MAPQ_CAP, stream=stream)

    # the comparator: a constant slot array and score-only outputs per slot, one trace arena (the calls follow each other)
    per_slot_fields = (("scores", "int32"), ("readEnds", "int32"), ("textEnds", "int64"))
    d_constant = [torch.full((R,), j, dtype=torch.int32, device=dev) for j in range(SLOTS)]
    per_slot = [{name: torch.zeros(R, dtype=getattr(torch, dtype), device=dev) for name, dtype in per_slot_fields} for _ in range(SLOTS)]
    per_slot_out = [api.affine_outputs(**{name: t.data_ptr() for name, t in out.items()}) for out in per_slot]
    scratch_bytes = g.align_chains_affine_scratch_bytes(M)
    d_trace = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)

    def four_calls():
        for j in range(SLOTS):
            g.align_chains_affine(vin, d_constant[j].data_ptr(), R, per_slot_out[j], d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD,
                                  max_drift=MAX_DRIFT, scoring=costs, max_ops=MAX_OPS, max_rows=M, stream=stream)

    reduced = {}

    def four_calls_and_reduction():
        four_calls()
        with torch.cuda.stream(stream_obj):
            scores = torch.stack([out["scores"] for out in per_slot], 1).long() & 0xFFFFFFFF
            scores = torch.where((scores < 0xFFFFFFFC) & (scores >= max(MIN_SCORE, 1)), scores, torch.zeros_like(scores))
            best, best_slot = scores.max(1)
            rest = scores.scatter(1, best_slot.unsqueeze(1), 0)
            reduced["best"], reduced["second"] = best, rest.max(1)[0]

    # one affine call as it is used behind the new one, and verification
    affine_fields = (("scores", "int32", R), ("editDistances", "int32", R), ("readBegins", "int32", R), ("readEnds", "int32", R), ("textBegins", "int64", R),
                     ("textEnds", "int64", R), ("numOps", "int32", R), ("ops", "int32", R * MAX_OPS), ("numUnaligned", "int64", 1), ("numTruncated", "int64", 1))
    affine_out = {name: torch.zeros(size, dtype=getattr(torch, dtype), device=dev) for name, dtype, size in affine_fields}
    aout = api.affine_outputs(**{name: t.data_ptr() for name, t in affine_out.items()})
    torch.cuda.synchronize()

    def one_affine_call():
        g.align_chains_affine(vin, d_best.data_ptr(), R, aout, d_trace.data_ptr(), max_candidates=SLOTS, band_pad=BAND_PAD, max_drift=MAX_DRIFT,
                              scoring=costs, max_ops=MAX_OPS, max_rows=M, stream=stream)

    ours, theirs, theirs_reduced, affine_ms, verify_ms = timed(new_call, four_calls, four_calls_and_reduction, one_affine_call, verify_call)

    # ---- parity: the host twin on the same arrays, all reads ----
    host_chars, host_offsets = d_reads[:R * M].cpu().numpy(), d_char_offsets.cpu().numpy()
    host_slots = {name: t.cpu().numpy() for name, t in d_slots.items()}
    host_ends = np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64)
    host_out = {name: np.zeros(size, getattr(np, dtype)) for name, dtype, size in score_fields}
    hin = api.verify_inputs(host_chars.ctypes.data, R * M, host_offsets.ctypes.data, **{name: a.ctypes.data for name, a in host_slots.items()})
    hout = api.slot_score_outputs(**{name: a.ctypes.data for name, a in host_out.items()})
    host_ms = []
    for _ in range(3):
        for a in host_out.values():
            a[...] = 0
        t = time.perf_counter()
        rc = L.awfmScoreChainsAffine(C.byref(hin), R, SLOTS, BAND_PAD, MAX_DRIFT, C.byref(costs), MIN_SCORE, MAPQ_CAP, host_text.ctypes.data, n,
                                     host_ends.ctypes.data, args.records, api.AwFmAlphabetDna, C.byref(hout), args.threads)
        host_ms.append((time.perf_counter() - t) * 1e3)
        assert rc == _lib.AwFmSuccess, rc
    calls = args.steps + args.warmup
    got = {name: t.cpu().numpy() for name, t in score_out.items()}
    counters = {"numUnscored": int(got["numUnscored"][0]), "numMapped": int(got["numMapped"][0])}
    equal = {name: bool(np.array_equal(got[name], host_out[name])) for name in host_out if name not in counters}
    equal.update({name: counters[name] == calls * int(host_out[name][0]) for name in counters})
    same_as_comparator = {}
    for new_name, old_name in (("slotScores", "scores"), ("slotReadEnds", "readEnds"), ("slotTextEnds", "textEnds")):
        old = np.stack([out[old_name].cpu().numpy() for out in per_slot], 1).reshape(-1)
        same_as_comparator[new_name] = bool(np.array_equal(got[new_name], old))
    best = got["bestScores"].astype(np.int64) & 0xFFFFFFFF
    second = got["secondScores"].astype(np.int64) & 0xFFFFFFFF
    # the torch reduction knows no duplicates: it agrees with the new call on the best score everywhere, on the second where no duplicate is met
    reduction_best_equal = bool(np.array_equal(reduced["best"].cpu().numpy(), best))
    reduction_second_differs = int((reduced["second"].cpu().numpy() != second).sum())
    new_s, old_s, old_reduced_s = summary(ours), summary(theirs), summary(theirs_reduced)
    affine_s, verify_s, host_s = summary(affine_ms), summary(verify_ms), summary(host_ms)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (old_s["max_ms"] - old_s["min_ms"])
    mapped = got["bestSlots"].astype(np.int64) & 0xFFFFFFFF != 0xFFFFFFFF
    quality = got["mappingQualities"]
    scores = got["slotScores"].astype(np.int64) & 0xFFFFFFFF
    result.update(new_call=new_s, four_affine_calls=old_s, four_affine_calls_and_torch_reduction=old_reduced_s, one_affine_call=affine_s,
                  verify_call=verify_s, host_twin=host_s, results_equal=all(equal.values()), results_equal_by_output=equal, reads_compared=R,
                  per_slot_equal_to_comparator=same_as_comparator, reduction_best_equal=reduction_best_equal,
                  reads_whose_second_the_reduction_gets_wrong=reduction_second_differs, comparator_scratch_bytes=scratch_bytes,
                  slots_used=int((scores != 0xFFFFFFFF).sum()), slots_unscored=counters["numUnscored"] // calls, reads_mapped=counters["numMapped"] // calls,
                  share_mapq_cap=round(float((mapped & (quality == MAPQ_CAP)).mean()), 5), share_mapq_zero=round(float((mapped & (quality == 0)).mean()), 5),
                  share_without_best_slot=round(float((~mapped).mean()), 5), reads_with_second=int((second > 0).sum()),
                  mean_best_score=round(float(best[mapped].mean()), 3),
                  new_call_over_verify_call=round(new_s["median_ms"] / verify_s["median_ms"], 3),
                  new_call_over_one_affine_call=round(new_s["median_ms"] / affine_s["median_ms"], 3),
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(old_s["median_ms"] / new_s["median_ms"], 3),
                       "speedup_with_reduction": round(old_reduced_s["median_ms"] / new_s["median_ms"], 3),
                       "met": bool(old_s["median_ms"] - new_s["median_ms"] > spreads)})

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
