#!/usr/bin/env python3
"""Times awfmGpuChooseStrands (paired) and awfmGpuOrientReads on the 3.1 Gbp synthetic index bench.py uses, on the batch of
scripts/pair_mates_timing.py held on BOTH strands: 2^19 pairs of an inward-facing library, 2^20 reads of 150 characters as
sequenced -- every pair from a random strand of its fragment --, their reverse complements in the second half of the buffer
(awfmGpuReverseComplementReads, ALL), hence 2^21 rows; seeds, hits, candidates (4 slots), chains and the slot scores of a real
awfmGpuScoreChainsAffine call on the 2^21 rows, all resident on the device before the clock starts.  Device events around every one
of --steps calls after --warmup, the sides taking turns call by call in one process; spreads as min / median / max.

  new call    awfmGpuChooseStrands with AWFM_STRANDS_PAIRED and every output: minInsert 200, maxInsert 600, unpairedPenalty 17,
              windowPad 50, mapqCap 60.
  comparator  the same work as a caller writes it without the call: torch gathers that build the two same-strand tables
              (F(m1), V(m2)) and (V(m1), F(m2)) -- the second with the interval mirrored, [2 n - maxInsert, 2 n - minInsert] for
              reads of n characters, so that mate A is m1 in both and the tie rules agree --, two awfmGpuPairMates calls, and a torch
              selection over the two winners and the discordant pair of the reads' bests over both strands that yields strands,
              strandSlots, properPairs, pairScores and the windows by row.  Equality with the new call on those outputs is ASSERTED.
  orient      awfmGpuOrientReads with qualities and all nine columns, against a device-to-device copy of the bytes it writes.
  host twins  awfmChooseStrands and awfmOrientReads on --threads threads, every output over the whole batch: ASSERTED equal.
  bar         the new call's median lies below the comparator's by more than the sum of the two sides' max - min.  The ratio of
              the orient call to the copy is an expectation, not a bar.

Prints one JSON line and writes it to --out (default profiles/strands/timing.json)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pair_mates_timing import (BAND, BAND_PAD, CANDIDATE_FIELDS, CAP, CHAIN_FIELDS, GAP_HIGH, GAP_LOW, GAP_PENALTY, LOOKBACK, MAPQ_CAP,  # noqa: E402
                               MAX_DRIFT, MAX_HITS_PER_SEED, MAX_INSERT, MIN_INSERT, MIN_LENGTH, MIN_SCORE, MIN_VOTES, READ_LENGTH, SCORING, SLOTS,
                               STEP, UNPAIRED_PENALTY, WINDOW_PAD, arguments, summary)

NONE = 0xFFFFFFFF
READ_FIELDS = (("strands", "uint8"), ("strandSlots", "int32"), ("bestScores", "int32"), ("secondScores", "int32"), ("mappingQualities", "uint8"),
               ("baseFlags", "int16"))
ROW_FIELDS = (("rowSlots", "int32"), ("windowSequences", "int32"), ("windowBegins", "int64"), ("windowEnds", "int64"))
PAIR_FIELDS = (("properPairs", "uint8"), ("pairScores", "int32"), ("pairSecondScores", "int32"), ("templateLengths", "int64"), ("pairQualities", "uint8"))
COUNTERS = ("numReverse", "numProper", "numWindows", "numMalformed")
COMPARED = ("strands", "strandSlots", "properPairs", "pairScores", "windowSequences", "windowBegins", "windowEnds")
COLUMNS = (("sequences", "int32"), ("chainAnchors", "int32"), ("chainReadBegins", "int32"), ("chainReadEnds", "int32"), ("chainBeginDiagonals", "int64"),
           ("chainEndDiagonals", "int64"), ("slotScores", "int32"), ("slotReadEnds", "int32"), ("slotTextEnds", "int64"))


def selection(torch, first, second, scores, sequences, read_ends, text_ends, R, C, M):
    """the comparator's last step: from the two pairings' properPairs, pairScores and pairSlots and the flat slot arrays of the
    2R rows -> strands, strandSlots, properPairs, pairScores and the windows by row, as the new call defines them"""
    dev, P, floor = scores.device, R // 2, max(MIN_SCORE, 1)

    def per_read(flat):  # [2R * C] -> [R, 2C], strand slot u = sigma C + j
        return torch.cat((flat[:R * C].view(R, C), flat[R * C:].view(R, C)), 1)

    score, sequence = per_read(scores).long() & NONE, per_read(sequences).long() & NONE
    start = per_read(text_ends) - (per_read(read_ends).long() & NONE)
    u = torch.arange(2 * C, device=dev)
    counts = (score < 0xFFFFFFFC) & (score >= floor)
    best_key = torch.where(counts, score * 32 + (31 - u), torch.zeros_like(score)).max(1)[0]
    has = best_key > 0
    best = torch.where(has, 31 - (best_key & 31), torch.zeros_like(best_key))
    best_score = (best_key >> 5).view(P, 2)
    best_start = torch.gather(start, 1, best.unsqueeze(1)).view(P, 2)
    best_sequence = torch.gather(sequence, 1, best.unsqueeze(1)).view(P, 2)
    has, best = has.view(P, 2), best.view(P, 2)
    sigma = (best >= C).long()
    both = has[:, 0] & has[:, 1]
    T = torch.where(sigma[:, 0] == 0, best_start[:, 1] + M - best_start[:, 0], best_start[:, 0] + M - best_start[:, 1])
    concordant = both & (sigma[:, 0] != sigma[:, 1]) & (best_sequence[:, 0] == best_sequence[:, 1]) & (T >= MIN_INSERT) & (T <= MAX_INSERT)
    exists = 1 << 44
    discordant = torch.where(both & ~concordant, exists | (torch.clamp(best_score[:, 0] + best_score[:, 1] - UNPAIRED_PENALTY, min=0) << 11) |
                             ((31 - best[:, 0]) << 5) | (31 - best[:, 1]), torch.zeros_like(T))
    keys = [discordant]
    for pairing, first_strand in ((first, 0), (second, 1)):  # mate A is m1, on strand first_strand; mate B is m2, on the other
        slots = (pairing["pairSlots"].long() & NONE).view(P, 2)
        u1, u2 = slots[:, 0] + first_strand * C, slots[:, 1] + (1 - first_strand) * C
        key = exists | ((pairing["pairScores"].long() & NONE) << 11) | 1024 | ((31 - u1) << 5) | (31 - u2)
        keys.append(torch.where(pairing["properPairs"] != 0, key, torch.zeros_like(key)))
    win = torch.stack(keys, 1).max(1)[0]
    won, proper = win != 0, (win & 1024) != 0
    chosen = torch.stack((31 - ((win >> 5) & 31), 31 - (win & 31)), 1)
    chosen = torch.where(won.unsqueeze(1), chosen, best)
    placed = won.unsqueeze(1) | has
    strand = torch.where(placed, (chosen >= C).long(), torch.zeros_like(chosen))
    out = {"strands": strand.to(torch.uint8).view(-1),
           "strandSlots": torch.where(placed, chosen - strand * C, torch.full_like(chosen, NONE)).to(torch.int32).view(-1),
           "properPairs": proper.to(torch.uint8),
           "pairScores": torch.where(won, (win >> 11) & 0x1FFFFFFFF, torch.where(has[:, 0], best_score[:, 0], torch.where(has[:, 1], best_score[:, 1],
                                     torch.zeros_like(win)))).to(torch.int32)}
    # the windows by row: a read of a pair that is not proper, around its mate's best strand slot, on the other strand
    mate_start, mate_sequence, mate_sigma = best_start.flip(1), best_sequence.flip(1), sigma.flip(1)
    windowed = ~proper.unsqueeze(1) & has.flip(1)
    E = mate_start + M
    begins = torch.where(mate_sigma == 0, mate_start + MIN_INSERT - M - WINDOW_PAD, E - MAX_INSERT - WINDOW_PAD)
    ends = torch.where(mate_sigma == 0, mate_start + MAX_INSERT + WINDOW_PAD, E - MIN_INSERT + M + WINDOW_PAD)
    rows = (torch.arange(R, device=dev).view(P, 2) + R * (1 - mate_sigma))[windowed]
    out["windowSequences"] = torch.full((2 * R,), -1, dtype=torch.int32, device=dev)
    out["windowBegins"], out["windowEnds"] = torch.zeros(2 * R, dtype=torch.int64, device=dev), torch.zeros(2 * R, dtype=torch.int64, device=dev)
    out["windowSequences"][rows] = mate_sequence[windowed].to(torch.int32)
    out["windowBegins"][rows] = torch.clamp(begins[windowed], min=0)
    out["windowEnds"][rows] = torch.clamp(ends[windowed], min=0)
    return out


def prepare(args):
    """the index, the pairs as sequenced on both strands, the 2R rows, their seeds, located, mapped, chained and scored, all
    resident on the device -> a dict of what the timed calls start from"""
    import numpy as np
    import torch
    from avxwindowfmindex_amd import _lib, api
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream_obj = torch.cuda.Stream()
    stream = stream_obj.cuda_stream
    R, n, M = args.reads & ~1, args.text_len, READ_LENGTH
    P, rows = R // 2, 2 * R
    t0 = time.time()
    d_text = torch.empty(n, dtype=torch.uint8, device=dev)
    assert L.awfmGpuSynthText(d_text.data_ptr(), 0, n, 2, 0, None) == 1
    torch.cuda.synchronize()
    ix = api.gpu_create_index(d_text.data_ptr(), api.AwFmAlphabetDna, args.sa_ratio, args.seed_k, on_device_length=n, device=0)
    g = api.GpuIndex(ix, acquire=True)
    g.set_record_table(np.array([(r + 1) * n // args.records - 1 for r in range(args.records)], np.uint64))
    build_s = round(time.time() - t0, 2)
    host_text = d_text.cpu().numpy()
    torch.cuda.synchronize()
    g.set_text(host_text)
    del host_text

    # the pairs as sequenced: the left read is the fragment's first M characters, the right read the reverse complement of its last
    # M; a pair from the forward strand is (left, right), one from the reverse strand (right, left); 5 % substitutions
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    d_reads = torch.empty(rows * M + 64, dtype=torch.uint8, device=dev)
    letters = torch.tensor(list(b"acgt"), dtype=torch.uint8, device=dev)
    complement = torch.arange(256, dtype=torch.uint8, device=dev)
    for a, b in zip(b"acgtACGT", b"tgcaTGCA"):
        complement[a] = b
    for begin in range(0, P, 1 << 17):
        r = min(1 << 17, P - begin)
        at = torch.randint(0, n - 2 * M - GAP_HIGH, (r, 1), device=dev, generator=gen)
        behind = at + torch.randint(GAP_LOW, GAP_HIGH + 1, (r, 1), device=dev, generator=gen)
        anywhere = torch.randint(0, n - M, (r, 1), device=dev, generator=gen)
        behind = torch.where(torch.rand((r, 1), device=dev, generator=gen) < 0.1, anywhere, behind)
        pieces = []
        for where in (at, behind):
            piece = d_text[where + torch.arange(M, device=dev)]
            swap = torch.rand((r, M), device=dev, generator=gen) < 0.05
            pieces.append(torch.where(swap, letters[torch.randint(0, 4, (r, M), device=dev, generator=gen)], piece))
        left, right = pieces[0], complement[pieces[1].long()].flip(1)
        forward = torch.rand((r, 1), device=dev, generator=gen) < 0.5
        both = torch.stack((torch.where(forward, left, right), torch.where(forward, right, left)), 1)
        d_reads[2 * begin * M:2 * (begin + r) * M] = both.reshape(-1)
    del d_text
    torch.cuda.empty_cache()
    d_char_offsets = (torch.arange(rows + 1, device=dev) * M).contiguous()
    g.reverse_complement_reads(d_reads.data_ptr(), R * M, d_char_offsets.data_ptr(), R, d_reads.data_ptr() + R * M, api.COMPLEMENT_ALL, stream=stream)
    stream_obj.synchronize()

    e = torch.arange(STEP, M + 1, STEP, device=dev)
    per_read = e.numel()
    base = (torch.arange(rows, device=dev) * M).unsqueeze(1)
    d_ends = (base + e).reshape(-1).contiguous()
    d_starts = (base + torch.clamp(e - CAP, min=0)).reshape(-1).contiguous()
    S = d_ends.numel()
    d_seed_ends = e.to(torch.int32).repeat(rows).contiguous()
    d_read_offsets = (torch.arange(rows + 1, device=dev) * per_read).contiguous()
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
    cin = api.candidate_inputs(d_read_offsets.data_ptr(), S, d_seed_ends.data_ptr(), d_lengths.data_ptr(), 0, d_hit_offsets.data_ptr(), H,
                               d_positions.data_ptr(), d_sequences.data_ptr())
    cand = {name: torch.empty(rows * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CANDIDATE_FIELDS}
    cand_scratch = torch.empty(api.read_candidates_scratch_bytes(rows), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.read_candidates(cin, rows, api.candidate_outputs(**{name: t.data_ptr() for name, t in cand.items()}), cand_scratch.data_ptr(),
                      max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, min_votes=MIN_VOTES, max_candidates=SLOTS, stream=stream)
    stream_obj.synchronize()
    chain = {name: torch.empty(rows * SLOTS, dtype=getattr(torch, dtype), device=dev) for name, dtype in CHAIN_FIELDS}
    chain_scratch = torch.empty(api.read_chains_scratch_bytes(rows), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g.read_chains(cin, rows, cand["sequences"].data_ptr(), cand["diagonals"].data_ptr(), cand["diagonalSpans"].data_ptr(),
                  api.chain_outputs(**{name: t.data_ptr() for name, t in chain.items()}), chain_scratch.data_ptr(),
                  max_hits_per_seed=MAX_HITS_PER_SEED, band=BAND, max_candidates=SLOTS, lookback=LOOKBACK, gap_penalty=GAP_PENALTY, stream=stream)
    stream_obj.synchronize()
    slot_names = ("chainAnchors", "chainReadBegins", "chainReadEnds", "chainBeginDiagonals", "chainEndDiagonals")
    vin = api.verify_inputs(d_reads.data_ptr(), rows * M, d_char_offsets.data_ptr(), sequences=cand["sequences"].data_ptr(),
                            **{name: chain[name].data_ptr() for name in slot_names})
    scored = {"slotScores": torch.zeros(rows * SLOTS, dtype=torch.int32, device=dev), "slotReadEnds": torch.zeros(rows * SLOTS, dtype=torch.int32, device=dev),
              "slotTextEnds": torch.zeros(rows * SLOTS, dtype=torch.int64, device=dev)}
    torch.cuda.synchronize()
    g.score_chains_affine(vin, rows, api.slot_score_outputs(**{name: t.data_ptr() for name, t in scored.items()}), max_candidates=SLOTS,
                          band_pad=BAND_PAD, max_drift=MAX_DRIFT, scoring=api.align_scoring(*SCORING), min_score=MIN_SCORE, mapq_cap=MAPQ_CAP, stream=stream)
    stream_obj.synchronize()
    columns = dict({"sequences": cand["sequences"]}, **{name: chain[name] for name in slot_names}, **scored)
    return dict(np=np, torch=torch, api=api, g=g, dev=dev, stream_obj=stream_obj, stream=stream, R=R, P=P, M=M, rows=rows, seeds=S, hits=H,
                build_s=build_s, d_reads=d_reads, d_char_offsets=d_char_offsets, vin=vin, columns=columns, keep=(ix, cand, chain))


def main():
    args = arguments(os.path.join("profiles", "strands", "timing.json")).parse_args()
    w = prepare(args)
    np, torch, api, g, dev, stream_obj, stream = w["np"], w["torch"], w["api"], w["g"], w["dev"], w["stream_obj"], w["stream"]
    R, P, M, rows, C, columns, d_offsets = w["R"], w["P"], w["M"], w["rows"], SLOTS, w["columns"], w["d_char_offsets"]
    result = {"reads": R, "pairs": P, "rows": rows, "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
              "index_build_s": w["build_s"], "seeds": w["seeds"], "hits": w["hits"],
              "parameters": {"read_length": M, "slots": C, "min_score": MIN_SCORE, "mapq_cap": MAPQ_CAP, "min_insert": MIN_INSERT, "max_insert": MAX_INSERT,
                             "unpaired_penalty": UNPAIRED_PENALTY, "window_pad": WINDOW_PAD, "mate_gap": [GAP_LOW, GAP_HIGH], "host_threads": args.threads,
                             "share_of_pairs_from_the_reverse_strand": 0.5, "share_of_pairs_with_the_right_read_anywhere": 0.1}}

    def timed(*fns):
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

    # ---- the new call ----
    sin = api.strand_inputs(d_offsets.data_ptr(), columns["sequences"].data_ptr(), columns["slotScores"].data_ptr(), columns["slotReadEnds"].data_ptr(),
                            columns["slotTextEnds"].data_ptr())
    new_out = {name: torch.zeros(R, dtype=getattr(torch, dtype), device=dev) for name, dtype in READ_FIELDS}
    new_out.update({name: torch.zeros(rows, dtype=getattr(torch, dtype), device=dev) for name, dtype in ROW_FIELDS})
    new_out.update({name: torch.zeros(P, dtype=getattr(torch, dtype), device=dev) for name, dtype in PAIR_FIELDS})
    d_counters = torch.zeros(4, dtype=torch.int64, device=dev)
    sout = api.strand_outputs(**{name: t.data_ptr() for name, t in new_out.items()}, **{name: d_counters.data_ptr() + 8 * k for k, name in enumerate(COUNTERS)})
    settings = dict(min_insert=MIN_INSERT, max_insert=MAX_INSERT, max_candidates=C, min_score=MIN_SCORE, unpaired_penalty=UNPAIRED_PENALTY,
                    window_pad=WINDOW_PAD, mapq_cap=MAPQ_CAP)

    def new_call():
        g.choose_strands(sin, R, sout, paired=True, stream=stream, **settings)

    # ---- the comparator: gathers, two awfmGpuPairMates calls, a selection ----
    reads = torch.arange(R, device=dev).view(P, 2)
    table_rows = [torch.stack((reads[:, 0], reads[:, 1] + R), 1).reshape(-1), torch.stack((reads[:, 0] + R, reads[:, 1]), 1).reshape(-1)]
    d_table_offsets = (torch.arange(R + 1, device=dev) * M).contiguous()  # (reads of one length: every table has these offsets)
    intervals = [(MIN_INSERT, MAX_INSERT), (2 * M - MAX_INSERT, 2 * M - MIN_INSERT)]
    pairings = [{"properPairs": torch.zeros(P, dtype=torch.uint8, device=dev), "pairScores": torch.zeros(P, dtype=torch.int32, device=dev),
                 "pairSlots": torch.zeros(R, dtype=torch.int32, device=dev)} for _ in range(2)]
    old, kept = {}, []

    def comparator_call():
        with torch.cuda.stream(stream_obj):
            kept.clear()
            for index, interval, pairing in zip(table_rows, intervals, pairings):
                table = {name: columns[name].view(rows, C).index_select(0, index).contiguous() for name in ("sequences", "slotScores", "slotReadEnds", "slotTextEnds")}
                kept.append(table)
                pin = api.pair_inputs(d_table_offsets.data_ptr(), table["sequences"].data_ptr(), table["slotScores"].data_ptr(),
                                      table["slotReadEnds"].data_ptr(), table["slotTextEnds"].data_ptr())
                g.pair_mates(pin, P, api.pair_outputs(**{name: t.data_ptr() for name, t in pairing.items()}), interval[0], interval[1], max_candidates=C,
                             min_score=MIN_SCORE, unpaired_penalty=UNPAIRED_PENALTY, window_pad=WINDOW_PAD, mapq_cap=MAPQ_CAP, stream=stream)
            old.update(selection(torch, pairings[0], pairings[1], columns["slotScores"], columns["sequences"], columns["slotReadEnds"],
                                 columns["slotTextEnds"], R, C, M))

    ours, theirs = timed(new_call, comparator_call)
    comparator_equal = {name: bool(torch.equal(old[name], new_out[name])) for name in COMPARED}
    assert all(comparator_equal.values()), comparator_equal

    # ---- orient against a copy of the bytes it writes ----
    d_qualities = torch.randint(33, 127, (rows * M,), dtype=torch.uint8, device=dev)
    oriented = {"readChars": torch.zeros(R * M, dtype=torch.uint8, device=dev), "qualities": torch.zeros(R * M, dtype=torch.uint8, device=dev),
                "readOffsets": torch.zeros(R + 1, dtype=torch.int64, device=dev), "numMalformed": torch.zeros(1, dtype=torch.int64, device=dev)}
    oriented.update({name: torch.zeros(R * C, dtype=getattr(torch, dtype), device=dev) for name, dtype in COLUMNS})
    oin = api.orient_inputs(w["vin"], new_out["strands"].data_ptr(), d_qualities.data_ptr(),
                            **{name: columns[name].data_ptr() for name in ("slotScores", "slotReadEnds", "slotTextEnds")})
    oout = api.orient_outputs(oriented["readChars"].data_ptr(), R * M, oriented["readOffsets"].data_ptr(),
                              **{name: t.data_ptr() for name, t in oriented.items() if name not in ("readChars", "readOffsets")})
    written = sum(t.numel() * t.element_size() for name, t in oriented.items() if name != "numMalformed")
    d_from, d_to = torch.zeros(written, dtype=torch.uint8, device=dev), torch.empty(written, dtype=torch.uint8, device=dev)

    def orient_call():
        g.orient_reads(oin, R, oout, max_candidates=C, stream=stream)

    def copy_call():
        with torch.cuda.stream(stream_obj):
            d_to.copy_(d_from)

    orient_ms, copy_ms = timed(orient_call, copy_call)

    # ---- the host twins on the same arrays, the whole batch ----
    calls = args.steps + args.warmup
    host_offsets = d_offsets.cpu().numpy().astype(np.uint64)
    dtypes = {"int32": np.uint32, "int64": np.uint64, "uint8": np.uint8, "int16": np.uint16}
    host_columns = {name: columns[name].cpu().numpy().view(np.int64 if "Diagonals" in name else dtypes[dtype]).reshape(rows, C) for name, dtype in COLUMNS}
    t = time.perf_counter()
    want = api.choose_strands_host(host_offsets, host_columns, paired=True, min_insert=MIN_INSERT, max_insert=MAX_INSERT, min_score=MIN_SCORE,
                                   unpaired_penalty=UNPAIRED_PENALTY, window_pad=WINDOW_PAD, mapq_cap=MAPQ_CAP, threads=args.threads)
    host_ms = (time.perf_counter() - t) * 1e3  # (the wrapper's allocations included)
    equal = {}
    for name, dtype in READ_FIELDS + ROW_FIELDS + PAIR_FIELDS:
        equal[name] = bool(np.array_equal(new_out[name].cpu().numpy().view(want[name].dtype), want[name]))
    counters = d_counters.cpu().numpy()
    for k, name in enumerate(COUNTERS):
        equal[name] = int(counters[k]) == calls * want[name]
    host_chars = w["d_reads"][:rows * M].cpu().numpy()
    want_oriented = api.orient_reads_host(host_chars, host_offsets, want["strands"], slots=host_columns, qualities=d_qualities.cpu().numpy(), threads=args.threads)
    orient_equal = {}
    for name, tensor in oriented.items():
        if name == "numMalformed":
            orient_equal[name] = int(tensor.item()) == calls * want_oriented[name] == 0
        else:
            have = tensor.cpu().numpy()
            orient_equal[name] = bool(np.array_equal(have.view(np.asarray(want_oriented[name]).dtype), np.asarray(want_oriented[name]).reshape(-1)))
    assert all(equal.values()), equal
    assert all(orient_equal.values()), orient_equal

    new_s, old_s, orient_s, copy_s = summary(ours), summary(theirs), summary(orient_ms), summary(copy_ms)
    spreads = (new_s["max_ms"] - new_s["min_ms"]) + (old_s["max_ms"] - old_s["min_ms"])
    result.update(new_call=new_s, comparator=old_s, orient_call=orient_s, copy_of_written_bytes=copy_s, written_bytes=written,
                  host_twin_ms=round(host_ms, 1), results_equal=True, results_equal_by_output=equal, orient_equal_by_output=orient_equal,
                  comparator_equal_by_output=comparator_equal, reads_compared=R, proper_pairs=want["numProper"], windows=want["numWindows"],
                  reads_on_the_reverse_strand=want["numReverse"], malformed=want["numMalformed"],
                  pairs_with_a_second=int((want["pairSecondScores"] > 0).sum()),
                  orient_over_copy=round(orient_s["median_ms"] / copy_s["median_ms"], 3),
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
