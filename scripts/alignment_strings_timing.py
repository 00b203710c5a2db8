#!/usr/bin/env python3
"""Times awfmGpuAlignmentStrings on the 3.1 Gbp synthetic index bench.py uses, on the batch scripts/align_affine_timing.py uses:
located, mapped, clustered, chained, verified and affine-aligned reads resident on the device, the text uploaded with
awfmGpuIndexSetText.  Both sides end with the strings in host memory; they take turns call by call in one process, --steps calls
after --warmup; spreads as min / median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions, through
              scripts/align_affine_timing.py's pipeline up to awfmGpuAlignChainsAffine (scoring (1, 4, 6, 1), maxOps 32), all
              before the clock starts.
  new path    awfmGpuAlignmentStrings (classic CIGAR and MD) with arenas of 64 bytes per read, then a download of the two offsets
              arrays and of the used part of the two arenas into page-locked memory.  Wall clock, the last copy waited for.
  today       what a caller does without the call: a download of numOps, ops, textBegins, slots and sequences, then the host twin
              awfmAlignmentStrings on --threads (16) threads over a host copy of the text.  Wall clock.  Every byte of the new
              path's output is compared with it in the same run.
  bar         the new path's median lies below today's median by more than the sum of the two sides' max - min.
  beside it   (expectations, no bars) the device call alone by device events; its ratio to a device-to-device copy of its
              compulsory bytes -- the used runs of ops, 20 bytes of inputs per read, 16 bytes of offsets per read and the
              strings written; the 128-byte text lines of the mismatches and deletions are named separately --; the mean string
              lengths; the share of waves that took the direct tier.

Prints one JSON line and writes it to --out (default profiles/alignment_strings/timing.json)."""
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
    p.add_argument("--out", default=os.path.join("profiles", "alignment_strings", "timing.json"))
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

    new_call()
    stream_obj.synchronize()
    del d_trace
    torch.cuda.empty_cache()

    # ---- the strings: the new path, and what a caller does today ----
    ARENA, TILE = 64, 8192
    inputs = {"sequences": slots[0], "slots": d_best, "textBegins": affine_out["textBegins"], "numOps": affine_out["numOps"], "ops": affine_out["ops"]}
    sin = api.string_inputs(*(inputs[name].data_ptr() for name in ("sequences", "slots", "textBegins", "numOps", "ops")))
    d_str = {"cigarOffsets": torch.zeros(R + 1, dtype=torch.int64, device=dev), "mdOffsets": torch.zeros(R + 1, dtype=torch.int64, device=dev),
             "cigarChars": torch.zeros(R * ARENA, dtype=torch.uint8, device=dev), "mdChars": torch.zeros(R * ARENA, dtype=torch.uint8, device=dev)}
    d_str_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    string_scratch_bytes = g.alignment_strings_scratch_bytes(R)
    d_string_scratch = torch.empty(string_scratch_bytes, dtype=torch.uint8, device=dev)
    sout = api.string_outputs(cigarCapacity=R * ARENA, mdCapacity=R * ARENA, numSkipped=d_str_counters.data_ptr(), numOverflow=d_str_counters.data_ptr() + 8,
                              **{name: t.data_ptr() for name, t in d_str.items()})
    pinned = {name: torch.empty(t.numel(), dtype=t.dtype).pin_memory() for name, t in d_str.items()}
    torch.cuda.synchronize()

    def device_call():
        g.alignment_strings(sin, R, sout, d_string_scratch.data_ptr(), max_candidates=SLOTS, max_ops=MAX_OPS, classic=True, stream=stream)

    used = {}

    def new_path():
        device_call()
        with torch.cuda.stream(stream_obj):
            for name in ("cigarOffsets", "mdOffsets"):
                pinned[name].copy_(d_str[name], non_blocking=True)
            stream_obj.synchronize()  # the totals say how much of the arenas is used
            for name in ("cigar", "md"):
                used[name] = min(int(pinned[name + "Offsets"][R]), R * ARENA)
                pinned[name + "Chars"][:used[name]].copy_(d_str[name + "Chars"][:used[name]], non_blocking=True)
            stream_obj.synchronize()

    host_in = {name: torch.empty(t.numel(), dtype=t.dtype).pin_memory() for name, t in inputs.items()}
    host_ends = np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64)
    host_str = {"cigarOffsets": np.zeros(R + 1, np.uint64), "mdOffsets": np.zeros(R + 1, np.uint64), "cigarChars": np.zeros(R * ARENA, np.uint8),
                "mdChars": np.zeros(R * ARENA, np.uint8)}
    host_counters = np.zeros(2, np.uint64)
    hout = api.string_outputs(cigarCapacity=R * ARENA, mdCapacity=R * ARENA, numSkipped=host_counters.ctypes.data, numOverflow=host_counters.ctypes.data + 8,
                              **{name: a.ctypes.data for name, a in host_str.items()})
    hin = api.string_inputs(*(host_in[name].data_ptr() for name in ("sequences", "slots", "textBegins", "numOps", "ops")))

    def today():
        with torch.cuda.stream(stream_obj):
            for name, t in inputs.items():
                host_in[name].copy_(t, non_blocking=True)
            stream_obj.synchronize()
        rc = L.awfmAlignmentStrings(C.byref(hin), R, SLOTS, MAX_OPS, api.STRINGS_CIGAR_M, host_text.ctypes.data, n, host_ends.ctypes.data, args.records,
                                    api.AwFmAlphabetDna, C.byref(hout), args.threads)
        assert rc == _lib.AwFmSuccess, rc

    ours, theirs = timed(new_path, today, host=(new_path, today))
    calls = args.steps + args.warmup
    got = {name: t.numpy() for name, t in pinned.items()}
    totals = {name: int(host_str[name + "Offsets"][R]) for name in ("cigar", "md")}
    equal = {name: bool(np.array_equal(got[name].view(np.uint64), host_str[name])) for name in ("cigarOffsets", "mdOffsets")}
    for name in ("cigar", "md"):
        size = min(totals[name], R * ARENA)
        equal[name + "Chars"] = bool(used[name] == size and np.array_equal(got[name + "Chars"][:size], host_str[name + "Chars"][:size]))
    device_counters = d_str_counters.cpu().numpy()
    equal["numSkipped"] = bool(int(device_counters[0]) == int(host_counters[0]))
    equal["numOverflow"] = bool(int(device_counters[1]) == int(host_counters[1]))

    # the device call alone, beside a device-to-device copy of its compulsory bytes
    counts = affine_out["numOps"].cpu().numpy().astype(np.int64)
    with_strings = np.diff(host_str["cigarOffsets"].astype(np.int64)) > 0
    used_runs = int(np.minimum(counts, MAX_OPS)[with_strings].sum())
    compulsory = 4 * used_runs + 20 * R + 16 * (R + 1) + totals["cigar"] + totals["md"]
    d_from = torch.zeros(compulsory, dtype=torch.uint8, device=dev)
    d_to = torch.empty(compulsory, dtype=torch.uint8, device=dev)

    def copy_call():
        with torch.cuda.stream(stream_obj):
            d_to.copy_(d_from, non_blocking=True)

    call_ms, copy_ms = timed(device_call, copy_call)
    ops_host = affine_out["ops"].cpu().numpy().reshape(R, MAX_OPS)
    live = (np.arange(MAX_OPS)[None, :] < counts[:, None]) & with_strings[:, None]
    text_characters = int((ops_host[live] >> 4)[np.isin(ops_host[live] & 15, (2, 8))].sum())
    spans = {name: np.diff(host_str[name + "Offsets"].astype(np.int64)[::64]) for name in ("cigar", "md")}  # (whole waves; the last one may be short)
    new_s, host_s, call_s, copy_s = summary(ours), summary(theirs), summary(call_ms), summary(copy_ms)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (host_s["max_ms"] - host_s["min_ms"])
    aligned = int(with_strings.sum())
    result.update(new_path=new_s, today=host_s, device_call=call_s, device_copy_of_compulsory_bytes=copy_s, results_equal=all(equal.values()),
                  results_equal_by_output=equal, reads_compared=R, arena_bytes_per_read=ARENA, scratch_bytes=string_scratch_bytes,
                  reads_with_strings=aligned, reads_skipped=int(host_counters[0]) // calls, reads_overflowed=int(host_counters[1]) // calls,
                  cigar_bytes=totals["cigar"], md_bytes=totals["md"], mean_cigar_length=round(totals["cigar"] / max(aligned, 1), 3),
                  mean_md_length=round(totals["md"] / max(aligned, 1), 3), used_runs=used_runs, compulsory_bytes=compulsory,
                  text_characters_read=text_characters, text_line_bytes_at_most=128 * text_characters,
                  device_call_over_copy=round(call_s["median_ms"] / copy_s["median_ms"], 3),
                  waves=int(sum(s.size for s in spans.values())), waves_direct=int(sum(int((s > TILE).sum()) for s in spans.values())),
                  downloaded_bytes_new_path=16 * (R + 1) + min(totals["cigar"], R * ARENA) + min(totals["md"], R * ARENA),
                  downloaded_bytes_today=sum(t.numel() * t.element_size() for t in inputs.values()),
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
