#!/usr/bin/env python3
"""Times awfmGpuReadCandidates on the 3.1 Gbp synthetic index bench.py uses against what a caller does today with torch, both
on the same located and mapped hits resident on the device; device events around every one of --steps calls after --warmup,
the two sides taking turns call by call in one process; spreads as min / median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions; the longest match ending at every
              4th position, cap 64, minLength 16 (awfmGpuLongestSuffixMatches); hit offsets, awfmGpuLocate and
              awfmGpuLocalPositions against a record table of --records equal records, all before the clock starts.
              maxHitsPerSeed 32, band 8, minVotes 2.
  new call    awfmGpuReadCandidates with 4 slots per read and every output.
  comparator  torch on the device: a seed per hit (repeat_interleave), the filters, diagonals, ONE sort of a 64-bit key
              (read, sequence, diagonal), run boundaries by a neighbour compare, votes / span / read interval per run
              (scatter_reduce amin / amax), and the best run per read by scatter_reduce amax of (votes, -run): the first
              candidate of every read, the number of candidates and of kept hits.  Checked equal to the new call's first slot
              in the same run.
  bar         the new call's median lies below the comparator's median by more than the sum of the two sides' max - min.
  floor       a device-to-device copy of the bytes the call must read and write (inputs once, outputs once); ratio, no bar.
  repeat      the same batch with maxHitsPerSeed 0 (no read of it overflows), and again with ONE more read that is a single
              seed of --repeat-hits hits: the wave that gets it streams all of them to report the true count.

Prints one JSON line and writes it to --out (default profiles/read_candidates/timing.json)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

READ_LENGTH, STEP, CAP, MIN_LENGTH, MAX_HITS_PER_SEED, BAND, MIN_VOTES, SLOTS = 150, 4, 64, 16, 32, 8, 2, 4
NONE = 0xFFFFFFFF
SLOT_FIELDS = (("sequences", "int32"), ("diagonals", "int64"), ("votes", "int32"), ("diagonalSpans", "int32"), ("readBegins", "int32"),
               ("readEnds", "int32"))


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
    p.add_argument("--repeat-hits", type=count, default=1 << 22)
    p.add_argument("--seed-k", type=int, default=12)
    p.add_argument("--sa-ratio", type=int, default=8)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join("profiles", "read_candidates", "timing.json"))
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
    assert R <= 1 << 21 and args.records <= 64, "the comparator's key holds 21 bits of read and 6 of sequence"
    result = {"reads": R, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "parameters": {"read_length": M, "step": STEP, "cap": CAP, "min_length": MIN_LENGTH, "max_hits_per_seed": MAX_HITS_PER_SEED,
                             "band": BAND, "min_votes": MIN_VOTES, "slots": SLOTS, "records": args.records}}

    def timed(*fns):
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

    # ---- the new call ----
    def outputs(reads):
        out = {name: torch.empty(reads * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in SLOT_FIELDS}
        out["numCandidates"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["keptHits"] = torch.empty(reads, dtype=torch.int32, device=dev)
        out["numOverflowed"] = torch.zeros(1, dtype=torch.int64, device=dev)
        return out

    def new_call_on(reads, read_offsets, seeds, seed_ends, lengths, hit_offsets, hits, positions, sequences, max_hits):
        out = outputs(reads)
        scratch = torch.empty(api.read_candidates_scratch_bytes(reads), dtype=torch.uint8, device=dev)
        cin = api.candidate_inputs(read_offsets.data_ptr(), seeds, seed_ends.data_ptr(), lengths.data_ptr(), 0, hit_offsets.data_ptr(), hits,
                                   positions.data_ptr(), sequences.data_ptr())
        cout = api.candidate_outputs(**{name: t.data_ptr() for name, t in out.items()})
        torch.cuda.synchronize()

        def call():
            g.read_candidates(cin, reads, cout, scratch.data_ptr(), max_hits_per_seed=max_hits, band=BAND, min_votes=MIN_VOTES,
                              max_candidates=SLOTS, stream=stream)
        nbytes = scratch.numel() + sum(t.numel() * t.element_size() for t in out.values())
        return call, out, nbytes, (cin, cout, scratch)

    new_call, new_out, new_bytes, keep = new_call_on(R, d_read_offsets, S, d_seed_ends, d_lengths, d_hit_offsets, H, d_positions, d_sequences,
                                                     MAX_HITS_PER_SEED)

    # ---- the comparator ----
    final = {}

    def comparator():
        with torch.cuda.stream(stream_obj):
            counts = d_counts.long()
            lengths, seed_ends = d_lengths.long(), d_seed_ends.long()
            usable = (counts <= MAX_HITS_PER_SEED) & (lengths <= seed_ends)
            seed = torch.repeat_interleave(torch.arange(S, device=dev), counts)  # (the hits are all of every seed's, in order)
            keep_hit = usable[seed] & (d_sequences[:H] != -1)
            seed = seed[keep_hit]
            sequence = d_sequences[:H][keep_hit].long()
            anchor = (seed_ends - lengths)[seed]
            diagonal = d_positions[:H][keep_hit] - anchor
            read = seed // per_read
            key = (read << 42) | (sequence << 36) | (diagonal + CAP * 4)  # diagonals of local positions: above -READ_LENGTH, below 2^36
            key, order = torch.sort(key)
            anchor, end = anchor[order], seed_ends[seed][order]
            head = torch.ones_like(key, dtype=torch.bool)
            head[1:] = ((key[1:] >> 36) != (key[:-1] >> 36)) | (key[1:] - key[:-1] > BAND)
            run = torch.cumsum(head, 0) - 1
            first = torch.nonzero(head).flatten()
            runs = first.numel()
            votes = torch.diff(first, append=torch.tensor([key.numel()], device=dev))
            last = first + votes - 1
            begin = torch.full((runs,), 1 << 40, dtype=torch.int64, device=dev).scatter_reduce(0, run, anchor, "amin")
            finish = torch.zeros(runs, dtype=torch.int64, device=dev).scatter_reduce(0, run, end, "amax")
            run_read = key[first] >> 42
            enough = votes >= MIN_VOTES
            score = torch.where(enough, (votes << 40) | ((1 << 40) - 1 - torch.arange(runs, device=dev)), 0)
            best = torch.zeros(R, dtype=torch.int64, device=dev).scatter_reduce(0, run_read, score, "amax")
            has = best > 0
            winner = ((1 << 40) - 1 - (best & ((1 << 40) - 1)))[has]
            final.update(has=has, sequence=(key[first[winner]] >> 36) & 63, diagonal=(key[first[winner]] & ((1 << 36) - 1)) - CAP * 4,
                         votes=votes[winner], span=key[last[winner]] - key[first[winner]], begin=begin[winner], end=finish[winner],
                         candidates=torch.bincount(run_read[enough], minlength=R), kept=torch.bincount(read, minlength=R))

    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    comparator()
    stream_obj.synchronize()
    result["peak_device_bytes"] = {"new_call_scratch_and_outputs": new_bytes, "comparator": torch.cuda.max_memory_allocated() - before}

    ours, theirs = timed(new_call, comparator)
    slot0 = {name: new_out[name].view(R, SLOTS)[:, 0] for name, _ in SLOT_FIELDS}
    has = final["has"]
    equal = {"which_reads_have_a_candidate": torch.equal(slot0["sequences"] != -1, has),
             "sequences": torch.equal(slot0["sequences"][has].long(), final["sequence"]),
             "diagonals": torch.equal(slot0["diagonals"][has], final["diagonal"]),
             "votes": torch.equal(slot0["votes"][has].long(), final["votes"]),
             "diagonalSpans": torch.equal(slot0["diagonalSpans"][has].long(), final["span"]),
             "readBegins": torch.equal(slot0["readBegins"][has].long(), final["begin"]),
             "readEnds": torch.equal(slot0["readEnds"][has].long(), final["end"]),
             "numCandidates": torch.equal(new_out["numCandidates"].long(), final["candidates"]),
             "keptHits": torch.equal(new_out["keptHits"].long(), final["kept"])}
    new_s, cmp_s = summary(ours), summary(theirs)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (cmp_s["max_ms"] - cmp_s["min_ms"])
    result.update(new_call=new_s, comparator=cmp_s, results_equal=all(equal.values()), results_equal_by_output=equal,
                  overflowed_reads=int(new_out["numOverflowed"].item()) // (args.steps + args.warmup),
                  reads_with_a_candidate=int(has.sum().item()), largest_read_kept_hits=int(new_out["keptHits"].max().item()),
                  reads_of_the_workgroup_tier=int((new_out["keptHits"] > 256).sum().item()),
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(cmp_s["median_ms"] / new_s["median_ms"], 3),
                       "met": cmp_s["median_ms"] - new_s["median_ms"] > spreads})
    final.clear()

    # ---- the floor: the bytes the call must read and write, copied once ----
    must = 8 * (R + 1) + 8 * S + 8 * (S + 1) + 12 * H + R * (SLOTS * 28 + 8)
    src, dst = torch.empty(must, dtype=torch.uint8, device=dev), torch.empty(must, dtype=torch.uint8, device=dev)

    def copy():
        with torch.cuda.stream(stream_obj):
            dst.copy_(src)

    floor = summary(timed(copy)[0])
    result["floor"] = {"bytes": must, "copy": floor, "new_call_over_copy": round(new_s["median_ms"] / floor["median_ms"], 2)}
    del src, dst

    # ---- one read that is a repeat, no filter ----
    X = args.repeat_hits
    plain, plain_out, _, keep2 = new_call_on(R, d_read_offsets, S, d_seed_ends, d_lengths, d_hit_offsets, H, d_positions, d_sequences, 0)
    r_read_offsets = torch.cat([d_read_offsets, torch.tensor([S + 1], device=dev)])
    r_seed_ends = torch.cat([d_seed_ends, torch.tensor([CAP], dtype=torch.int32, device=dev)])
    r_lengths = torch.cat([d_lengths, torch.tensor([CAP], dtype=torch.int32, device=dev)])
    r_hit_offsets = torch.cat([d_hit_offsets, torch.tensor([H + X], device=dev)])
    r_positions = torch.cat([d_positions[:H], torch.randint(0, n // args.records - M, (X,), device=dev, generator=gen)])
    r_sequences = torch.cat([d_sequences[:H], torch.zeros(X, dtype=torch.int32, device=dev)])
    repeat, repeat_out, _, keep3 = new_call_on(R + 1, r_read_offsets, S + 1, r_seed_ends, r_lengths, r_hit_offsets, H + X, r_positions, r_sequences, 0)
    a, b = timed(plain, repeat)
    result["repeat"] = {"hits_of_the_one_read": X, "without_it": summary(a), "with_it": summary(b),
                        "its_kept_hits_reported": int(repeat_out["keptHits"][R].item()) & 0xFFFFFFFF,
                        "overflowed_without_it": int(plain_out["numOverflowed"].item()) // (args.steps + args.warmup),
                        "overflowed_with_it": int(repeat_out["numOverflowed"].item()) // (args.steps + args.warmup)}

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
