#!/usr/bin/env python3
"""Times awfmGpuPairMates and awfmGpuReverseComplementReads on the 3.1 Gbp synthetic index bench.py uses, on the batch
scripts/score_chains_timing.py uses read as PAIRS: located, mapped, clustered and chained hits resident on the device, the text
uploaded with awfmGpuIndexSetText, the slot scores written by a real awfmGpuScoreChainsAffine call.  Device events around every
one of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as min / median / max.

  workload    --reads (2^20) reads of 150 characters with 5 % substitutions as 2^19 pairs on one strand: mate B begins 150..350
              positions behind mate A (T = 300..500), except in a tenth of the pairs, whose mate B lies anywhere; seeds, hits,
              candidates (4 slots), chains and awfmGpuScoreChainsAffine (scoring (1, 4, 6, 1), minScore 30) before the clock starts.
  new call    awfmGpuPairMates with every output: minInsert 200, maxInsert 600, unpairedPenalty 17, windowPad 50, mapqCap 60.
  copy        a device-to-device copy of the call's compulsory bytes: what it must read (the three offsets a pair, four arrays a
              slot, a quality a read) into a buffer, and what it must write (five arrays a pair, five a read) from one.
  comparator  (a) what a caller writes today: a torch broadcast over the C x C candidates of every pair that produces pairSlots,
              properPairs, pairScores and the windows (no second, no qualities); it lives here and is checked equal to the new
              call on those outputs in the same run.  (b) the host twin on --threads (16) threads, one call, wall clock, every
              output compared over all pairs.
  complement  awfmGpuReverseComplementReads of the odd reads of the same read buffer against a copy of its bytes, and against
              the host twin's bytes.
  bar         the new call's median lies below (a)'s by more than the sum of the two sides' max - min.

Prints one JSON line and writes it to --out (default profiles/pair_mates/timing.json)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS, LOOKBACK, GAP_PENALTY = 150, 4, 64, 16, 32, 8, 2, 4, 64, 1
BAND_PAD, MAX_DRIFT, SCORING, MIN_SCORE, MAPQ_CAP = 8, 15, (1, 4, 6, 1), 30, 60
MIN_INSERT, MAX_INSERT, UNPAIRED_PENALTY, WINDOW_PAD, GAP_LOW, GAP_HIGH = 200, 600, 17, 50, 150, 350
CANDIDATE_FIELDS = (("sequences", "int32"), ("diagonals", "int64"), ("votes", "int32"), ("diagonalSpans", "int32"), ("readBegins", "int32"),
                    ("readEnds", "int32"))
CHAIN_FIELDS = (("chainScores", "int32"), ("chainAnchors", "int32"), ("chainReadBegins", "int32"), ("chainReadEnds", "int32"),
                ("chainBeginDiagonals", "int64"), ("chainEndDiagonals", "int64"))
PAIR_FIELDS = (("properPairs", "uint8", 1), ("pairScores", "int32", 1), ("pairSecondScores", "int32", 1), ("templateLengths", "int64", 1),
               ("pairQualities", "uint8", 1), ("pairSlots", "int32", 2), ("mappingQualities", "uint8", 2), ("windowSequences", "int32", 2),
               ("windowBegins", "int64", 2), ("windowEnds", "int64", 2))


def count(text):
    return int(float(text))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "calls": len(ms)}


def broadcast_pairing(torch, slot_scores, slot_sequences, slot_read_ends, slot_text_ends, char_offsets, slots):
    """comparator (a): pairSlots, properPairs, pairScores and the windows of every pair by a broadcast over its slots x slots
    candidates, from the flat device arrays the new call reads"""
    dev, P, old = slot_scores.device, slot_scores.numel() // (2 * slots), {}
    floor = max(MIN_SCORE, 1)
    score = (slot_scores.long() & 0xFFFFFFFF).view(P, 2, slots)
    sequence = (slot_sequences.long() & 0xFFFFFFFF).view(P, 2, slots)
    start = (slot_text_ends - (slot_read_ends.long() & 0xFFFFFFFF)).view(P, 2, slots)
    lengths = (char_offsets[1:] - char_offsets[:-1]).view(P, 2)
    counts = (score < 0xFFFFFFFC) & (score >= floor) & (lengths >= 0).unsqueeze(2)
    slot = torch.arange(slots, device=dev)
    # each mate's best slot: the largest score, ties to the lowest slot
    best_key = torch.where(counts, score * 16 + (15 - slot), torch.zeros_like(score)).max(2)[0]
    has = best_key > 0
    best = torch.where(has, 15 - (best_key & 15), torch.zeros_like(best_key))
    a, b = slot.view(1, slots, 1), slot.view(1, 1, slots)
    T = start[:, 1].unsqueeze(1) + lengths[:, 1].view(P, 1, 1) - start[:, 0].unsqueeze(2)
    concordant = counts[:, 0].unsqueeze(2) & counts[:, 1].unsqueeze(1) & (sequence[:, 0].unsqueeze(2) == sequence[:, 1].unsqueeze(1)) & \
        (T >= MIN_INSERT) & (T <= MAX_INSERT)
    value = score[:, 0].unsqueeze(2) + score[:, 1].unsqueeze(1)
    discordant = (has[:, 0] & has[:, 1]).view(P, 1, 1) & (a == best[:, 0].view(P, 1, 1)) & (b == best[:, 1].view(P, 1, 1)) & ~concordant
    value = torch.where(discordant, torch.clamp(value - UNPAIRED_PENALTY, min=0), value)
    key = torch.where(concordant | discordant, (1 << 42) | (value << 9) | (concordant.long() << 8) | ((15 - a) << 4) | (15 - b),
                      torch.zeros_like(value)).view(P, slots * slots).max(1)[0]
    won, proper = key != 0, (key & 256) != 0
    chosen = torch.stack((15 - ((key >> 4) & 15), 15 - (key & 15)), 1)
    chosen = torch.where(won.unsqueeze(1), chosen, best)
    placed = won.unsqueeze(1) | has
    single = torch.gather(score, 2, best.unsqueeze(2)).squeeze(2)
    old["pairSlots"] = torch.where(placed, chosen, torch.full_like(chosen, 0xFFFFFFFF)).to(torch.int32).view(-1)
    old["properPairs"] = proper.to(torch.uint8)
    old["pairScores"] = torch.where(won, (key >> 9) & 0x1FFFFFFFF, torch.where(has[:, 0], single[:, 0], torch.where(has[:, 1], single[:, 1],
                                    torch.zeros_like(key)))).to(torch.int32)
    # the windows: a read of a pair that is not proper, around its mate's best slot
    mate_start = torch.gather(start, 2, best.unsqueeze(2)).squeeze(2).flip(1)
    mate_sequence = torch.gather(sequence, 2, best.unsqueeze(2)).squeeze(2).flip(1)
    windowed = ~proper.unsqueeze(1) & has.flip(1)
    end_of_b = mate_start[:, 0] + lengths[:, 1]
    begins = torch.stack((end_of_b - MAX_INSERT - WINDOW_PAD, mate_start[:, 1] + MIN_INSERT - lengths[:, 1] - WINDOW_PAD), 1)
    ends = torch.stack((end_of_b - MIN_INSERT + lengths[:, 0] + WINDOW_PAD, mate_start[:, 1] + MAX_INSERT + WINDOW_PAD), 1)
    old["windowSequences"] = torch.where(windowed, mate_sequence, torch.full_like(mate_sequence, 0xFFFFFFFF)).to(torch.int32).view(-1)
    old["windowBegins"] = torch.where(windowed, torch.clamp(begins, min=0), torch.zeros_like(begins)).view(-1)
    old["windowEnds"] = torch.where(windowed, torch.clamp(ends, min=0), torch.zeros_like(ends)).view(-1)
    return old


def arguments(out):
    p = argparse.ArgumentParser()
    p.add_argument("--text-len", type=count, default=3_100_000_000)
    p.add_argument("--reads", type=count, default=1 << 20)
    p.add_argument("--records", type=int, default=24)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=out)
    return p


def prepare(args):
    """the index, the pairs, their seeds, located, mapped, chained and scored, all resident on the device: what the timed calls
    of this script and of scripts/insert_size_timing.py start from -> a namespace of them, `result` and `timed` among them"""
    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    R, n, M = args.reads & ~1, args.text_len, READ_LENGTH
    P = R // 2
    result = {"reads": R, "pairs": P, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "parameters": {"read_length": M, "step": STEP, "cap": CAP, "min_length": MIN_LENGTH, "max_hits_per_seed": MAX_HITS_PER_SEED,
                             "band": BAND, "min_votes": MIN_VOTES, "slots": SLOTS, "lookback": LOOKBACK, "gap_penalty": GAP_PENALTY,
                             "records": args.records, "host_threads": args.threads, "band_pad": BAND_PAD, "max_drift": MAX_DRIFT,
                             "scoring": list(SCORING), "min_score": MIN_SCORE, "mapq_cap": MAPQ_CAP, "min_insert": MIN_INSERT,
                             "max_insert": MAX_INSERT, "unpaired_penalty": UNPAIRED_PENALTY, "window_pad": WINDOW_PAD,
                             "mate_gap": [GAP_LOW, GAP_HIGH], "share_of_pairs_with_mate_b_anywhere": 0.1}}

    def timed(*fns):
        """ms of --steps calls of every fn by device events, the fns taking turns call by call"""
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

    # ---- the index, the pairs, their seeds, located, mapped, chained and scored: all before the clock starts ----
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

    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    d_reads = torch.empty(R * M + 64, dtype=torch.uint8, device=dev)
    letters = torch.tensor(list(b"acgt"), dtype=torch.uint8, device=dev)
    for begin in range(0, P, 1 << 17):
        r = min(1 << 17, P - begin)
        at = torch.randint(0, n - 2 * M - GAP_HIGH, (r, 1), device=dev, generator=gen)
        behind = at + torch.randint(GAP_LOW, GAP_HIGH + 1, (r, 1), device=dev, generator=gen)
        anywhere = torch.randint(0, n - M, (r, 1), device=dev, generator=gen)
        behind = torch.where(torch.rand((r, 1), device=dev, generator=gen) < 0.1, anywhere, behind)
        both = torch.stack((at, behind), 1).reshape(2 * r, 1)  # mate A, mate B, mate A, ...
        piece = d_text[both + torch.arange(M, device=dev)]
        swap = torch.rand((2 * r, M), device=dev, generator=gen) < 0.05
        piece = torch.where(swap, letters[torch.randint(0, 4, (2 * r, M), device=dev, generator=gen)], piece)
        d_reads[2 * begin * M:2 * (begin + r) * M] = piece.reshape(-1)
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
    torch.cuda.synchronize()
    g.locate(d_ranges.data_ptr(), d_hit_offsets.data_ptr(), S, H, d_positions.data_ptr(), stream=stream)
    stream_obj.synchronize()
    g.local_positions(d_positions.data_ptr(), H, d_sequences.data_ptr(), d_positions.data_ptr(), stream=stream)
    stream_obj.synchronize()
    del d_starts, d_ends, d_ranges, d_scan
    torch.cuda.empty_cache()
    result.update(seeds=S, hits=H)

    cin = api.candidate_inputs(d_read_offsets.data_ptr(), S, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), H,
                               d_positions.data_ptr(), d_sequences.data_ptr())
    cand = {name: torch.empty(R * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CANDIDATE_FIELDS}
    cand_scratch = torch.empty(api.read_candidates_scratch_bytes(R), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.read_candidates(cin, R, api.candidate_outputs(**{name: t.data_ptr() for name, t in cand.items()}), cand_scratch.data_ptr(),
                      max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, min_votes=MIN_VOTES, max_candidates=SLOTS, stream=stream)
    stream_obj.synchronize()
    chain = {name: torch.empty(R * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CHAIN_FIELDS}
    chain_scratch = torch.empty(api.read_chains_scratch_bytes(R), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.read_chains(cin, R, cand["sequences"].data_ptr(), cand["diagonals"].data_ptr(), cand["diagonalSpans"].data_ptr(),
                  api.chain_outputs(**{name: t.data_ptr() for name, t in chain.items()}), chain_scratch.data_ptr(),
                  max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, max_candidates=SLOTS, lookback=LOOKBACK, gap_penalty=GAP_PENALTY, stream=stream)
    stream_obj.synchronize()
    d_char_offsets = (torch.arange(R + 1, device=dev) * M).contiguous()
    slot_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    vin = api.verify_inputs(d_reads.data_ptr(), R * M, d_char_offsets.data_ptr(), sequences=cand["sequences"].data_ptr(),
                            **{name: chain[name].data_ptr() for name in slot_names})
    costs = api.align_scoring(*SCORING)
    scored = {"slotScores": torch.zeros(R * SLOTS, dtype=torch.int32, device=dev), "slotReadEnds": torch.zeros(R * SLOTS, dtype=torch.int32, device=dev),
              "slotTextEnds": torch.zeros(R * SLOTS, dtype=torch.int64, device=dev), "mappingQualities": torch.zeros(R, dtype=torch.uint8, device=dev)}
    torch.cuda.synchronize()
    g.score_chains_affine(vin, R, api.slot_score_outputs(**{name: t.data_ptr() for name, t in scored.items()}), max_candidates=SLOTS,
                          band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=costs, min_score=MIN_SCORE, mapq_cap=MAPQ_CAP, stream=stream)
    stream_obj.synchronize()
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if k != "args"})


def main():
    args = arguments(os.path.join("profiles", "pair_mates", "timing.json")).parse_args()
    w = prepare(args)
    np, torch, api, g, dev, stream_obj, stream, timed, result = w.np, w.torch, w.api, w.g, w.dev, w.stream_obj, w.stream, w.timed, w.result
    R, P, M, d_reads, d_char_offsets, cand, scored = w.R, w.P, w.M, w.d_reads, w.d_char_offsets, w.cand, w.scored

    # ---- the new call ----
    pin = api.pair_inputs(d_char_offsets.data_ptr(), cand["sequences"].data_ptr(), scored["slotScores"].data_ptr(), scored["slotReadEnds"].data_ptr(),
                          scored["slotTextEnds"].data_ptr(), scored["mappingQualities"].data_ptr())
    new_out = {name: torch.zeros(P * per, dtype=getattr(torch, dtype), device=dev) for name, dtype, per in PAIR_FIELDS}
    d_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    pout = api.pair_outputs(numProper=d_counters.data_ptr(), numWindows=d_counters.data_ptr() + 8, **{name: t.data_ptr() for name, t in new_out.items()})
    settings = dict(min_insert=MIN_INSERT, max_insert=MAX_INSERT, max_candidates=SLOTS, min_score=MIN_SCORE, unpaired_penalty=UNPAIRED_PENALTY,
                    window_pad=WINDOW_PAD, mapq_cap=MAPQ_CAP)

    def new_call():
        g.pair_mates(pin, P, pout, stream=stream, **settings)

    # ---- the copy of its compulsory bytes ----
    bytes_in = P * 3 * 8 + R * SLOTS * (4 + 4 + 4 + 8) + R
    bytes_out = sum(P * per * torch.empty(0, dtype=getattr(torch, dtype)).element_size() for _, dtype, per in PAIR_FIELDS)
    d_from, d_to = torch.zeros(bytes_in + bytes_out, dtype=torch.uint8, device=dev), torch.empty(bytes_in + bytes_out, dtype=torch.uint8, device=dev)

    def copy_call():
        with torch.cuda.stream(stream_obj):
            d_to.copy_(d_from)

    # ---- comparator (a): the torch broadcast a caller writes today ----
    old = {}

    def torch_call():
        with torch.cuda.stream(stream_obj):
            old.update(broadcast_pairing(torch, scored["slotScores"], cand["sequences"], scored["slotReadEnds"], scored["slotTextEnds"],
                                         d_char_offsets, SLOTS))

    ours, copies, theirs = timed(new_call, copy_call, torch_call)

    # ---- the reverse complement of the same read buffer against a copy of its bytes ----
    d_complement, d_plain = torch.empty(R * M, dtype=torch.uint8, device=dev), torch.empty(R * M, dtype=torch.uint8, device=dev)
    d_malformed = torch.zeros(1, dtype=torch.int64, device=dev)

    def complement_call():
        g.reverse_complement_reads(d_reads.data_ptr(), R * M, d_char_offsets.data_ptr(), R, d_complement.data_ptr(), api.COMPLEMENT_ODD,
                                   d_malformed.data_ptr(), stream=stream)

    def plain_copy():
        with torch.cuda.stream(stream_obj):
            d_plain.copy_(d_reads[:R * M])

    complement_ms, plain_ms = timed(complement_call, plain_copy)

    # ---- parity and comparator (b): the host twins on the same arrays, all pairs ----
    host_offsets = d_char_offsets.cpu().numpy().astype(np.uint64)
    host_slots = {"sequences": cand["sequences"], "slotScores": scored["slotScores"], "slotReadEnds": scored["slotReadEnds"],
                  "slotTextEnds": scored["slotTextEnds"]}
    host_slots = {name: t.cpu().numpy().view(dtype).reshape(R, SLOTS) for (name, t), dtype in zip(host_slots.items(), (np.uint32, np.uint32, np.uint32, np.uint64))}
    host_qualities = scored["mappingQualities"].cpu().numpy()
    t = time.perf_counter()
    want = api.pair_mates_host(host_offsets, host_slots, MIN_INSERT, MAX_INSERT, mapping_qualities=host_qualities, min_score=MIN_SCORE,
                               unpaired_penalty=UNPAIRED_PENALTY, window_pad=WINDOW_PAD, mapq_cap=MAPQ_CAP, threads=args.threads)
    host_ms = (time.perf_counter() - t) * 1e3  # (the wrapper's allocations included)
    calls = args.steps + args.warmup
    got = {name: t.cpu().numpy() for name, t in new_out.items()}
    counters = d_counters.cpu().numpy()
    equal = {name: bool(np.array_equal(got[name].view(want[name].dtype), want[name])) for name, _, _ in PAIR_FIELDS}
    equal["numProper"] = int(counters[0]) == calls * want["numProper"]
    equal["numWindows"] = int(counters[1]) == calls * want["numWindows"]
    comparator_equal = {name: bool(torch.equal(t, new_out[name])) for name, t in old.items()}
    host_complement, _ = api.reverse_complement_reads_host(d_reads[:R * M].cpu().numpy(), host_offsets, api.COMPLEMENT_ODD, threads=args.threads)
    complement_equal = bool(np.array_equal(d_complement.cpu().numpy(), host_complement)) and int(d_malformed.item()) == 0

    new_s, copy_s, old_s, complement_s, plain_s = summary(ours), summary(copies), summary(theirs), summary(complement_ms), summary(plain_ms)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (old_s["max_ms"] - old_s["min_ms"])
    scores = host_slots["slotScores"]
    counting = (scores < 0xFFFFFFFC) & (scores >= MIN_SCORE)
    result.update(new_call=new_s, copy_of_compulsory_bytes=copy_s, torch_broadcast=old_s, host_twin_ms=round(host_ms, 1),
                  reverse_complement_call=complement_s, copy_of_read_buffer=plain_s, compulsory_bytes={"in": bytes_in, "out": bytes_out},
                  read_buffer_bytes=R * M, results_equal=all(equal.values()), results_equal_by_output=equal, pairs_compared=P,
                  torch_broadcast_equal=all(comparator_equal.values()), torch_broadcast_equal_by_output=comparator_equal,
                  reverse_complement_equal=complement_equal, proper_pairs=want["numProper"], windows=want["numWindows"],
                  pairs_with_a_second=int((want["pairSecondScores"] > 0).sum()), mean_counting_slots_per_read=round(float(counting.sum(1).mean()), 4),
                  share_pair_quality_cap=round(float((want["pairQualities"] == MAPQ_CAP).mean()), 5),
                  new_call_over_copy=round(new_s["median_ms"] / copy_s["median_ms"], 3),
                  reverse_complement_over_copy=round(complement_s["median_ms"] / plain_s["median_ms"], 3),
                  host_twin_over_new_call=round(host_ms / new_s["median_ms"], 1),
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(old_s["median_ms"] / new_s["median_ms"], 3),
                       "met": bool(old_s["median_ms"] - new_s["median_ms"] > spreads)})

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
