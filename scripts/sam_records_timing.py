#!/usr/bin/env python3
"""Times awfmGpuSamRecords on the 3.1 Gbp synthetic index bench.py uses, on the batch scripts/align_affine_timing.py uses: located,
mapped, clustered, chained, verified and affine-aligned reads resident on the device, their slot scores (mapping quality, second
score) and their classic CIGAR and MD strings made there too.  All sides end with SAM text in host memory; they take turns call
by call in one process, --steps calls after --warmup; spreads as min / median / max.

  workload    --reads (2^20) reads of 150 characters cut from the text with 5 % substitutions, through
              scripts/alignment_strings_timing.py's pipeline up to awfmGpuAlignmentStrings, plus awfmGpuScoreChainsAffine, all
              before the clock starts.  Reads 2p and 2p + 1 are taken as mates (AWFM_SAM_PAIRED); properPairs is a drawn array
              (the batch is not a paired library); no names, no qualities, no baseFlags; record names chr1 .. chr24.
  new path    awfmGpuSamRecords with an arena of 512 bytes per read, then a download of lineOffsets and of the used part of the
              arena into page-locked memory.  Wall clock, the last copy waited for.
  comparator  what a caller does at the parent commit, from calls that exist there: a download of sequences, slots, scores,
              editDistances, textBegins and the two string arenas with their offsets, then scripts/sam_records_comparator.c --
              the snprintf loop at the end of examples/read_sam.c with its per-read header lookup, on --threads (16) threads.
              The index here has no FASTA trailer, so the lookup is the comparator's own table lookup of the same shape as
              awFmGetHeaderStringFromSequenceNumber, not that function.  Wall clock.  Its lines are compared with the
              device's on the fields both produce: RNAME, POS, CIGAR, SEQ, NM, AS and MD of every aligned read, SEQ of the
              others.
  host twin   the same downloads (plus textEnds, mapping qualities, second scores, properPairs), then awfmSamRecords on
              --threads threads.  Wall clock.  Every byte of the new path's output is compared with it.
  bar         the new path's median lies below the comparator's median by more than the sum of the two sides' max - min.
  beside it   (expectations, no bars) the device call alone by device events; its ratio to a device-to-device copy of its
              compulsory bytes -- every input read once, lineOffsets and the lines written once; awfmGpuAlignmentStrings alone in
              this build (the alternating run against the parent commit's build is NOT made here: its files are untouched).

Prints one JSON line and writes it to --out (default profiles/sam_records/timing.json)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
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
    p.add_argument("--out", default=os.path.join("profiles", "sam_records", "timing.json"))
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

    # ---- slot scores (mapping quality, second score) and the strings, still before the clock ----
    d_second = torch.zeros(R, dtype=torch.int32, device=dev)
    d_mapq = torch.zeros(R, dtype=torch.uint8, device=dev)
    g.score_chains_affine(vin, R, api.slot_score_outputs(secondScores=d_second.data_ptr(), mappingQualities=d_mapq.data_ptr()), max_candidates=SLOTS,
                          band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=costs, min_score=0, mapq_cap=60, stream=stream)
    ARENA, LINE_ARENA = 64, 512
    string_in = {"sequences": slots[0], "slots": d_best, "textBegins": affine_out["textBegins"], "numOps": affine_out["numOps"], "ops": affine_out["ops"]}
    sin = api.string_inputs(*(string_in[name].data_ptr() for name in ("sequences", "slots", "textBegins", "numOps", "ops")))
    d_str = {"cigarOffsets": torch.zeros(R + 1, dtype=torch.int64, device=dev), "mdOffsets": torch.zeros(R + 1, dtype=torch.int64, device=dev),
             "cigarChars": torch.zeros(R * ARENA, dtype=torch.uint8, device=dev), "mdChars": torch.zeros(R * ARENA, dtype=torch.uint8, device=dev)}
    d_str_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    d_string_scratch = torch.empty(g.alignment_strings_scratch_bytes(R), dtype=torch.uint8, device=dev)
    sout = api.string_outputs(cigarCapacity=R * ARENA, mdCapacity=R * ARENA, numSkipped=d_str_counters.data_ptr(), numOverflow=d_str_counters.data_ptr() + 8,
                              **{name: t.data_ptr() for name, t in d_str.items()})
    torch.cuda.synchronize()

    def strings_call():
        g.alignment_strings(sin, R, sout, d_string_scratch.data_ptr(), max_candidates=SLOTS, max_ops=MAX_OPS, classic=True, stream=stream)

    strings_call()
    stream_obj.synchronize()
    assert int(d_str_counters[1].item()) == 0, "the string arenas are complete"
    totals = {name: int(d_str[name + "Offsets"][R].item()) for name in ("cigar", "md")}

    # ---- the records: the new path, the comparator, the host twin ----
    names = [b"chr%d" % (i + 1) for i in range(args.records)]
    name_offsets = np.concatenate(([0], np.cumsum([len(x) for x in names]))).astype(np.uint64)
    name_chars = np.frombuffer(b"".join(names), np.uint8).copy()
    d_name_offsets, d_name_chars = torch.from_numpy(name_offsets.view(np.int64)).to(dev), torch.from_numpy(name_chars).to(dev)
    d_proper = (torch.rand(R // 2, device=dev, generator=gen) < 0.9).to(torch.uint8)
    device_in = {"readChars": d_reads, "readOffsets": d_char_offsets, "recordNameOffsets": d_name_offsets, "recordNameChars": d_name_chars,
                 "sequences": slots[0], "slots": d_best, "scores": affine_out["scores"], "editDistances": affine_out["editDistances"],
                 "textBegins": affine_out["textBegins"], "textEnds": affine_out["textEnds"], "cigarOffsets": d_str["cigarOffsets"],
                 "cigarChars": d_str["cigarChars"], "mdOffsets": d_str["mdOffsets"], "mdChars": d_str["mdChars"], "mappingQualities": d_mapq,
                 "secondScores": d_second, "properPairs": d_proper}
    sam_in = api.sam_inputs(R * M, args.records, **{name: t.data_ptr() for name, t in device_in.items()})
    d_line_offsets = torch.zeros(R + 1, dtype=torch.int64, device=dev)
    d_lines = torch.zeros(R * LINE_ARENA, dtype=torch.uint8, device=dev)
    d_sam_counters = torch.zeros(2, dtype=torch.int64, device=dev)
    sam_scratch_bytes = g.sam_records_scratch_bytes(R)
    d_sam_scratch = torch.empty(sam_scratch_bytes, dtype=torch.uint8, device=dev)
    sam_out = api.sam_outputs(lineOffsets=d_line_offsets.data_ptr(), lineChars=d_lines.data_ptr(), lineCapacity=R * LINE_ARENA,
                              numUnaligned=d_sam_counters.data_ptr(), numOverflow=d_sam_counters.data_ptr() + 8)
    pinned_offsets = torch.empty(R + 1, dtype=torch.int64).pin_memory()
    pinned_lines = torch.empty(R * LINE_ARENA, dtype=torch.uint8).pin_memory()
    torch.cuda.synchronize()

    def device_call():
        g.sam_records(sam_in, R, sam_out, d_sam_scratch.data_ptr(), max_candidates=SLOTS, paired=True, stream=stream)

    used = {}

    def new_path():
        device_call()
        with torch.cuda.stream(stream_obj):
            pinned_offsets.copy_(d_line_offsets, non_blocking=True)
            stream_obj.synchronize()  # the total says how much of the arena is used
            used["lines"] = min(int(pinned_offsets[R]), R * LINE_ARENA)
            pinned_lines[:used["lines"]].copy_(d_lines[:used["lines"]], non_blocking=True)
            stream_obj.synchronize()

    # what either host side downloads: the reads are the caller's own and already on the host
    host_reads = d_reads[:R * M].cpu().numpy()
    host_read_offsets = np.arange(R + 1, dtype=np.uint64) * np.uint64(M)
    parent_names = ("sequences", "slots", "scores", "editDistances", "textBegins", "cigarOffsets", "mdOffsets")
    twin_names = parent_names + ("textEnds", "mappingQualities", "secondScores", "properPairs")
    host_in = {name: torch.empty(device_in[name].numel(), dtype=device_in[name].dtype).pin_memory() for name in twin_names}
    host_in.update({name: torch.empty(R * ARENA, dtype=torch.uint8).pin_memory() for name in ("cigarChars", "mdChars")})

    def download(which):
        with torch.cuda.stream(stream_obj):
            for name in which:
                host_in[name].copy_(device_in[name], non_blocking=True)
            for name in ("cigar", "md"):  # the used part of the two arenas (their totals are known from the strings call)
                host_in[name + "Chars"][:totals[name]].copy_(d_str[name + "Chars"][:totals[name]], non_blocking=True)
            stream_obj.synchronize()

    # the comparator: compiled here from scripts/sam_records_comparator.c, which uses nothing of the library
    here = os.path.dirname(os.path.abspath(__file__))
    build_dir = tempfile.mkdtemp()
    comparator_path = os.path.join(build_dir, "sam_records_comparator.so")
    subprocess.check_call(["gcc", "-std=gnu11", "-O2", "-fPIC", "-shared", "-pthread", os.path.join(here, "sam_records_comparator.c"), "-o", comparator_path])
    comparator = C.CDLL(comparator_path)

    class NameTable(C.Structure):
        _fields_ = [("offsets", C.c_void_p), ("chars", C.c_void_p), ("numRecords", C.c_uint64)]

    class ComparatorInputs(C.Structure):
        _fields_ = [("readChars", C.c_void_p), ("readOffsets", C.c_void_p), ("sequences", C.c_void_p), ("slots", C.c_void_p), ("scores", C.c_void_p),
                    ("editDistances", C.c_void_p), ("textBegins", C.c_void_p), ("cigarOffsets", C.c_void_p), ("cigarChars", C.c_void_p),
                    ("mdOffsets", C.c_void_p), ("mdChars", C.c_void_p), ("numReads", C.c_uint64), ("maxCandidates", C.c_uint32), ("lookup", C.c_void_p),
                    ("lookupUser", C.c_void_p), ("out", C.c_void_p), ("stride", C.c_uint64), ("written", C.c_void_p), ("firstRead", C.c_void_p)]

    table = NameTable(name_offsets.ctypes.data, name_chars.ctypes.data, args.records)
    comparator_lines = np.zeros(R * LINE_ARENA, np.uint8)
    written, first_read = np.zeros(args.threads, np.uint64), np.zeros(args.threads, np.uint64)
    cin2 = ComparatorInputs(host_reads.ctypes.data, host_read_offsets.ctypes.data, *(host_in[name].data_ptr() for name in ("sequences", "slots", "scores", "editDistances", "textBegins", "cigarOffsets", "cigarChars", "mdOffsets", "mdChars")),
                            R, SLOTS, C.cast(comparator.samComparatorTableLookup, C.c_void_p).value, C.addressof(table), comparator_lines.ctypes.data,
                            LINE_ARENA, written.ctypes.data, first_read.ctypes.data)
    comparator.samComparator.argtypes = [C.POINTER(ComparatorInputs), C.c_uint]
    comparator.samComparator.restype = C.c_int

    def parent_path():
        download(parent_names)
        assert comparator.samComparator(C.byref(cin2), args.threads) == 1

    twin_offsets, twin_lines, twin_counters = np.zeros(R + 1, np.uint64), np.zeros(R * LINE_ARENA, np.uint8), np.zeros(2, np.uint64)
    twin_in = api.sam_inputs(R * M, args.records, readChars=host_reads.ctypes.data, readOffsets=host_read_offsets.ctypes.data,
                             recordNameOffsets=name_offsets.ctypes.data, recordNameChars=name_chars.ctypes.data,
                             **{name: t.data_ptr() for name, t in host_in.items()})
    twin_out = api.sam_outputs(lineOffsets=twin_offsets.ctypes.data, lineChars=twin_lines.ctypes.data, lineCapacity=R * LINE_ARENA,
                               numUnaligned=twin_counters.ctypes.data, numOverflow=twin_counters.ctypes.data + 8)

    def twin_path():
        download(twin_names)
        rc = L.awfmSamRecords(C.byref(twin_in), R, SLOTS, api.SAM_PAIRED, C.byref(twin_out), args.threads)
        assert rc == _lib.AwFmSuccess, rc

    ours, theirs, twins = timed(new_path, parent_path, twin_path, host=(new_path, parent_path, twin_path))
    calls = args.steps + args.warmup
    got_offsets, total = pinned_offsets.numpy().view(np.uint64), int(twin_offsets[R])
    device_counters = d_sam_counters.cpu().numpy()
    equal = {"lineOffsets": bool(np.array_equal(got_offsets, twin_offsets)),
             "lineChars": bool(used["lines"] == total and np.array_equal(pinned_lines.numpy()[:total], twin_lines[:total])),
             "numUnaligned": bool(int(device_counters[0]) == int(twin_counters[0])), "numOverflow": bool(int(device_counters[1]) == int(twin_counters[1]))}
    # the comparator's lines against the device's, on the fields both produce
    device_lines = pinned_lines.numpy()[:total].tobytes().split(b"\n")[:-1]
    parent_lines = b"".join(comparator_lines[int(first_read[t]) * LINE_ARENA:int(first_read[t]) * LINE_ARENA + int(written[t])].tobytes()
                            for t in range(args.threads)).split(b"\n")[:-1]
    different, aligned = int(len(device_lines) != R or len(parent_lines) != R), 0
    for mine, theirs_line in zip(device_lines, parent_lines):
        a, b = mine.split(b"\t"), theirs_line.split(b"\t")
        if b[1] == b"4":
            different += not (int(a[1]) & 4 and a[5] == b[5] == b"*" and a[9] == b[9] and len(a) == 11)
            continue
        aligned += 1
        different += not (a[2:4] == b[2:4] and a[5] == b[5] and a[9] == b[9] and a[11:13] == b[11:13] and a[14:] == b[13:] and not int(a[1]) & 4)
    equal["comparator_shared_fields"] = different == 0

    # the device call alone, beside a device-to-device copy of its compulsory bytes; and the strings call alone in this build
    per_read = 4 * 5 + 8 * 5 + 1 + 8  # sequences (one entry), slots, scores, editDistances, secondScores; textBegins, textEnds, three offsets; mapq; lineOffsets
    compulsory = per_read * R + R // 2 + R * M + totals["cigar"] + totals["md"] + int(name_chars.size) + total
    d_from = torch.zeros(compulsory, dtype=torch.uint8, device=dev)
    d_to = torch.empty(compulsory, dtype=torch.uint8, device=dev)

    def copy_call():
        with torch.cuda.stream(stream_obj):
            d_to.copy_(d_from, non_blocking=True)

    call_ms, copy_ms, strings_ms = timed(device_call, copy_call, strings_call)
    lengths = np.diff(twin_offsets.astype(np.int64))
    new_s, parent_s, twin_s, call_s, copy_s, strings_s = (summary(x) for x in (ours, theirs, twins, call_ms, copy_ms, strings_ms))
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (parent_s["max_ms"] - parent_s["min_ms"])
    result.update(new_path=new_s, comparator=parent_s, host_twin=twin_s, device_call=call_s, device_copy_of_compulsory_bytes=copy_s,
                  results_equal=all(equal.values()), results_equal_by_output=equal, reads_compared=R, reads_aligned=aligned,
                  reads_unaligned=int(twin_counters[0]) // calls, reads_overflowed=int(twin_counters[1]) // calls, line_bytes=total,
                  mean_line_length=round(total / R, 3), longest_line=int(lengths.max()), lines_direct=int((lengths + 3 > 2048).sum()),
                  arena_bytes_per_read=LINE_ARENA, scratch_bytes=sam_scratch_bytes, compulsory_bytes=compulsory,
                  device_call_over_copy=round(call_s["median_ms"] / copy_s["median_ms"], 3),
                  downloaded_bytes_new_path=8 * (R + 1) + total,
                  downloaded_bytes_comparator=sum(host_in[name].numel() * host_in[name].element_size() for name in parent_names) + totals["cigar"] + totals["md"],
                  comparator_header_lookup="a table of %d names through a function pointer (the timed index has no FASTA trailer)" % args.records,
                  paired=True, proper_pairs="drawn, 90 % set", qualities=False, names=False,
                  alignment_strings={"this_build": strings_s, "parent_build_alternating": "not measured: awfm_strings_kernel.h and awfm_gpu_strings.hip are unchanged",
                                     "committed_profile_median_ms": 0.3416},
                  bar={"summed_spreads_ms": round(spreads, 4), "speedup": round(parent_s["median_ms"] / new_s["median_ms"], 3),
                       "met": bool(parent_s["median_ms"] - new_s["median_ms"] > spreads)})

    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
